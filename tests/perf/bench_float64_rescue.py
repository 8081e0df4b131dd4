"""RT_FLAG_F64_RESCUE (f64_sparse=True, f64_rescue=True) against what a user had before it: the map-free handle without the flag
while no stream overflows, the dense float64 handle once k streams do -- on the same device-resident complex128 input, in one
process; not part of pytest, and apart from bench.py, which measures the float32 headline.

    python tests/perf/bench_float64_rescue.py [--repeats 5] [--calls 10] [--warmup 2] [--out profiles/f64_rescue_bench.jsonl]

Shape: 4 096 streams x 300 kS, nperseg 256, 300 kS/s; k of the streams carry white noise 3 dB over the -90 dBW threshold (every
one of them overflows the largest hot_capacity), k = 0, 1, 16, 256, 4 096.  The handles run interleaved, repeat by repeat; a repeat
is `calls` calls (two in flight) between two HIP events on the stream all handles launch on.  One JSON line per k:
  k = 0   the flag handle against the map-free handle without the flag (the same launches by construction): the flag handle's
          slowest repeat beside the other's fastest and slowest;
  k > 0   the flag handle against the dense handle: every repeat's time, the medians, the time per rescued stream (the flag
          handle's median over its k = 0 median, per call and stream);
and a last line with the k at which the flag handle stops being faster than the dense one: the first measured k where it is
not, and the crossing interpolated between the two measured k around it."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from pyradiotracking_amd.analyze import BatchSignalAnalyzer  # noqa: E402

STREAMS, SAMPLES, NPERSEG, FS = 4096, 300000, 256, 300000
KS = (0, 1, 16, 256, 4096)
SIGMA_CLEAN = 1e-6
SIGMA_LOUD = float(np.sqrt(10 ** -8.7 * FS / 2))  # density 2 sigma^2 / fs = -87 dBW


def one_repeat(b, iq, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    b.enqueue(iq)
    n = 0
    for k in range(calls):
        if k + 1 < calls:
            b.enqueue(iq)  # two calls in flight
        n += len(b.fetch_records())
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--hot-capacity", type=int, default=8192)
    ap.add_argument("--streams", type=int, default=STREAMS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    S, n = a.streams, SAMPLES
    g = torch.Generator(device="cuda").manual_seed(NPERSEG)
    iq = torch.randn((S, n), dtype=torch.complex128, device="cuda", generator=g) * (SIGMA_CLEAN * np.sqrt(2.0))
    stream = torch.cuda.current_stream().cuda_stream
    kw = dict(precision="float64", sample_rate=FS, fft_nperseg=NPERSEG, sdr_callback_length=n, hip_stream=stream)
    devices = [str(i) for i in range(S)]
    handles = {"dense": BatchSignalAnalyzer(devices, **kw),
               "plain": BatchSignalAnalyzer(devices, f64_sparse=True, hot_capacity=a.hot_capacity, **kw),
               "rescue": BatchSignalAnalyzer(devices, f64_sparse=True, f64_rescue=True, hot_capacity=a.hot_capacity, **kw)}
    lines, med, loud = [], {}, 0
    try:
        for k in [v for v in KS if v <= S]:
            iq[loud:k] *= SIGMA_LOUD / SIGMA_CLEAN  # (the first k streams are loud)
            loud = k
            torch.cuda.synchronize()
            names = ("dense", "plain", "rescue") if k == 0 else ("dense", "rescue")
            for _ in range(a.warmup):
                for name in names:
                    handles[name].enqueue(iq)
                    handles[name].fetch_records()
            info = handles["rescue"].call_info()
            ms = {name: [] for name in names}
            for _ in range(a.repeats):
                for name in names:
                    ms[name].append(round(one_repeat(handles[name], iq, a.calls)[0], 3))
            med[k] = {name: float(np.median(v)) for name, v in ms.items()}
            out = {"metric": "float64_rescue", "streams": S, "samples": n, "nperseg": NPERSEG, "loud_streams": k, "repeats": a.repeats,
                   "calls_per_repeat": a.calls, "hot_capacity": a.hot_capacity, "n_dense_streams": int(info.n_dense_streams),
                   "fell_back": int(info.fell_back), "dense_ms": ms["dense"], "rescue_ms": ms["rescue"]}
            if k == 0:
                out["plain_ms"] = ms["plain"]
                out["plain_spread_ms"] = [min(ms["plain"]), max(ms["plain"])]
                out["rescue_slowest_ms"] = max(ms["rescue"])
                out["rescue_slowest_within_plain_spread"] = bool(max(ms["rescue"]) <= max(ms["plain"]))
            else:
                out["ratio_medians_dense_over_rescue"] = round(med[k]["dense"] / med[k]["rescue"], 3)
                out["ms_per_rescued_stream_and_call"] = round((med[k]["rescue"] - med[0]["rescue"]) / (k * a.calls), 5)
                recs = {}
                for name in names:
                    handles[name].enqueue(iq)
                    recs[name] = handles[name].fetch_records()
                out["records"] = int(len(recs["dense"]))
                out["records_equal"] = bool(len(recs["dense"]) == len(recs["rescue"]) and all(
                    np.array_equal(recs["dense"][f], recs["rescue"][f]) for f in ("stream", "fi", "start", "end", "shadowed")))
            lines.append(json.dumps(out))
            print(lines[-1], flush=True)
        ks = sorted(med)
        slower = [k for k in ks if k > 0 and med[k]["rescue"] >= med[k]["dense"]]
        last = {"metric": "float64_rescue_break_even", "streams": S, "first_measured_k_not_faster": slower[0] if slower else None}
        if slower and ks.index(slower[0]) > 0:
            k1, k0 = slower[0], ks[ks.index(slower[0]) - 1]
            d0, d1 = med[k0]["dense"] - med[k0]["rescue"], med[k1]["dense"] - med[k1]["rescue"]  # the flag handle's lead: > 0, then <= 0
            last["interpolated_k"] = int(round(k0 + (k1 - k0) * d0 / (d0 - d1)))
        lines.append(json.dumps(last))
        print(lines[-1], flush=True)
    finally:
        for b in handles.values():
            b.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
