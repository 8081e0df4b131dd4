"""The map-free float64 path (f64_sparse=True, RT_FLAG_F64_SPARSE) against the dense float64 handle, on the same device-resident
complex128 input, in one process -- not part of pytest, and apart from bench.py, which measures the float32 headline.

    python tests/perf/bench_float64_sparse.py [--repeats 5] [--calls 10] [--warmup 2] [--out profiles/f64_sparse_bench.jsonl]

Shapes: 256 streams x 2.048 MS at nperseg 256 and 4096 (those of profiles/f64_bench_float64.jsonl), and 4 096 streams x 300 kS at
nperseg 256, 300 kS/s (the reference's defaults), clean and with the noise floor 6 dB under the threshold.  The two handles run
interleaved, repeat by repeat; a repeat is `calls` calls (two in flight) between two HIP events on the stream both handles
launch on.  After the timed region the records of one more call are compared.  One JSON line per shape: every repeat's time, the
sparse handle's slowest against the dense handle's fastest (the bar: > 1), MS/s and the share of the HBM peak that 16 B per sample
are.  A sparse handle that cannot hold a shape (RT_E_HOT_OVERFLOW) is reported as such, with the dense figures."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from pyradiotracking_amd import _native  # noqa: E402
from pyradiotracking_amd.analyze import BatchSignalAnalyzer  # noqa: E402

HBM_BYTES_PER_S = 8.0e12  # MI355X peak
SHAPES = [
    dict(name="256x2048000_n256", streams=256, samples=2048000, nperseg=256, fs=2048000, sigma=1e-6),
    dict(name="256x2048000_n4096", streams=256, samples=2048000, nperseg=4096, fs=2048000, sigma=1e-6),
    dict(name="4096x300000_n256_clean", streams=4096, samples=300000, nperseg=256, fs=300000, sigma=1e-6),
    # white noise whose density 2 sigma^2 / fs sits 6 dB under the -90 dBW threshold
    dict(name="4096x300000_n256_noise_6dB_under", streams=4096, samples=300000, nperseg=256, fs=300000, sigma=float(np.sqrt(10 ** -9.6 * 300000 / 2))),
]


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


def run(shape, repeats, calls, warmup, hot_capacity):
    S, n, nperseg = shape["streams"], shape["samples"], shape["nperseg"]
    g = torch.Generator(device="cuda").manual_seed(nperseg)
    iq = torch.randn((S, n), dtype=torch.complex128, device="cuda", generator=g) * (shape["sigma"] * np.sqrt(2.0))
    stream = torch.cuda.current_stream().cuda_stream
    kw = dict(precision="float64", sample_rate=shape["fs"], fft_nperseg=nperseg, sdr_callback_length=n, hip_stream=stream)
    devices = [str(i) for i in range(S)]
    handles = {"dense": BatchSignalAnalyzer(devices, **kw), "sparse": BatchSignalAnalyzer(devices, f64_sparse=True, hot_capacity=hot_capacity, **kw)}
    out = {"metric": "float64_sparse_vs_dense", "shape": shape["name"], "streams": S, "samples": n, "nperseg": nperseg, "repeats": repeats,
           "calls_per_repeat": calls, "hot_capacity": hot_capacity}
    overflow = False
    try:
        for _ in range(warmup):
            for name, b in handles.items():
                b.enqueue(iq)
                try:
                    b.fetch_records()
                except _native.NativeError as e:
                    if name != "sparse" or e.code != _native.RT_E_HOT_OVERFLOW:
                        raise
                    overflow = True
        ms = {"dense": [], "sparse": []}
        for _ in range(repeats):
            for name, b in handles.items():
                if name == "sparse" and overflow:
                    continue
                ms[name].append(round(one_repeat(b, iq, calls)[0], 3))
        rate = lambda t: S * n * calls / (t * 1e-3) / 1e6  # noqa: E731
        out["dense_ms"] = ms["dense"]
        out["dense_msamples_per_s_best"] = round(rate(min(ms["dense"])), 1)
        out["sparse_overflow"] = overflow
        if not overflow:
            out["sparse_ms"] = ms["sparse"]
            out["sparse_msamples_per_s_worst"] = round(rate(max(ms["sparse"])), 1)
            out["sparse_msamples_per_s_best"] = round(rate(min(ms["sparse"])), 1)
            out["ratio_sparse_slowest_vs_dense_fastest"] = round(min(ms["dense"]) / max(ms["sparse"]), 3)
            out["ratio_medians"] = round(float(np.median(ms["dense"]) / np.median(ms["sparse"])), 3)
            out["sparse_hbm_fraction_16B"] = round(rate(float(np.median(ms["sparse"]))) * 1e6 * 16 / HBM_BYTES_PER_S, 3)
            recs = {}
            for name, b in handles.items():
                b.enqueue(iq)
                recs[name] = b.fetch_records()
            out["records"] = int(len(recs["dense"]))
            out["records_equal"] = bool(len(recs["dense"]) == len(recs["sparse"]) and all(
                np.array_equal(recs["dense"][f], recs["sparse"][f]) for f in ("stream", "fi", "start", "end", "shadowed")))
    finally:
        for b in handles.values():
            b.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--hot-capacity", type=int, default=8192)
    ap.add_argument("--shapes", nargs="*", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for shape in SHAPES:
        if a.shapes and shape["name"] not in a.shapes:
            continue
        line = json.dumps(run(shape, a.repeats, a.calls, a.warmup, a.hot_capacity))
        print(line, flush=True)
        lines.append(line)
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
