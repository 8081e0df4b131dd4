"""Cost of per-stream detection settings (``rt_set_stream_settings``) -- not part of pytest, and apart from bench.py, whose runs
never call the entry.  bench.py's pipelined loop (two calls in flight) on one box, three ways: ``uniform`` (scalar keywords: the
entry is never called, the kernels see a null pointer), ``table`` (per-device sequences holding the default values: the same
records, every stream's SNR threshold and duration gates read from the per-stream table) and ``mixed`` (values that differ:
3 / 5 / 8 dB, minima of 8 / 10 / 15 ms, maxima of 40 / 30 / 25 ms in turn -- other records, the line reports the counts).  The
three alternate ``--rounds`` times per workload and the best round of each is kept, so that all see the same clocks.

    python tests/perf/bench_stream_settings.py [--workloads config2 defaults_noise_floor] [--rounds 3] [--out FILE]

Prints (and with --out appends) one JSON line per workload: MS/s of the three, and the throughput lost against ``uniform``."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from oracle import analyze_oracle as oracle  # noqa: E402
from pyradiotracking_amd import synth  # noqa: E402
from pyradiotracking_amd.analyze import BatchSignalAnalyzer, default_lanes  # noqa: E402

# bench.py's geometries (its WORKLOADS / OTHER_CONFIGS), same generator
WORKLOADS = {
    "config2": dict(streams=256, sample_rate=2048000, samples=2048000, nperseg=256, window="hamming", steps=200, what="BASELINE config 2 (bench.py's headline)"),
    "defaults_noise_floor": dict(streams=4096, sample_rate=300000, samples=300000, nperseg=256, window="hamming", steps=40, noise_dbw=-88.0,
                                 what="the reference's defaults with the noise floor at -88 dBW, 2 dB over the threshold (AUTO climbs)"),
}


def make_input(w):
    win = oracle.window_coefficients(w["window"], w["nperseg"])
    kw = {}
    if "noise_dbw" in w:
        kw["noise_sigma"] = float((10.0 ** (w["noise_dbw"] / 10.0) * w["sample_rate"] / 2.0) ** 0.5)
    return synth.make_batch_device(w["streams"], w["samples"], w["sample_rate"], win, seed=1, **kw)


KINDS = ("uniform", "table", "mixed")


def settings(w, kind):
    """``uniform``: scalars, the entry is never called; ``table``: per-device sequences of the default values (the same records,
    read from the per-stream table); ``mixed``: settings that differ from stream to stream."""
    if kind == "uniform":
        return {}
    n = w["streams"]
    if kind == "table":
        return dict(snr_threshold_db=[5.0] * n, signal_min_duration_ms=[8.0] * n, signal_max_duration_ms=[40.0] * n)
    cycle = lambda vals: [vals[i % len(vals)] for i in range(n)]
    return dict(snr_threshold_db=cycle([5.0, 3.0, 8.0]), signal_min_duration_ms=cycle([8.0, 10.0, 15.0]), signal_max_duration_ms=cycle([40.0, 30.0, 25.0]))


def timed(w, iq, kind, settle=20):
    b = BatchSignalAnalyzer([str(i) for i in range(w["streams"])], sample_rate=w["sample_rate"], fft_nperseg=w["nperseg"],
                            fft_window=w["window"], sdr_callback_length=w["samples"], lanes=default_lanes(w["nperseg"], w["streams"]),
                            **settings(w, kind))
    steps = w["steps"]

    def loop(n):
        b.enqueue(iq)
        n_rec = 0
        for k in range(n):
            if k + 1 < n:
                b.enqueue(iq)  # two calls in flight
            n_rec += len(b.fetch_records())
        return n_rec

    loop(settle)  # (warm-up: AUTO settles on its level, clocks ramp)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n_rec = loop(steps)
    dt = time.perf_counter() - t0
    info = b.call_info()
    b.close()
    return w["streams"] * w["samples"] * steps / dt / 1e6, dt / steps * 1e3, n_rec, int(info.mode_used)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=list(WORKLOADS))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    for name in a.workloads:
        w = WORKLOADS[name]
        iq = make_input(w)
        best = {k: None for k in KINDS}
        for _ in range(a.rounds):
            for kind in KINDS:
                r = timed(w, iq, kind)
                if best[kind] is None or r[0] > best[kind][0]:
                    best[kind] = r
        off, tab, on = best["uniform"], best["table"], best["mixed"]
        line = {"metric": "stream_settings_cost", "workload": name, "what": w["what"], "streams": w["streams"], "samples": w["samples"],
                "nperseg": w["nperseg"], "steps": w["steps"], "rounds": a.rounds,
                "msamples_per_s_uniform": round(off[0], 1), "msamples_per_s_table": round(tab[0], 1), "msamples_per_s_mixed": round(on[0], 1),
                "ms_per_step_uniform": round(off[1], 4), "ms_per_step_table": round(tab[1], 4), "ms_per_step_mixed": round(on[1], 4),
                "throughput_lost_pct_table": round(100.0 * (1.0 - tab[0] / off[0]), 2),
                "throughput_lost_pct_mixed": round(100.0 * (1.0 - on[0] / off[0]), 2),
                "records_uniform": off[2], "records_table": tab[2], "records_mixed": on[2],
                "mode_used_uniform": off[3], "mode_used_table": tab[3], "mode_used_mixed": on[3]}
        del iq
        torch.cuda.empty_cache()
        print(json.dumps(line), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
