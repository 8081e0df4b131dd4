"""What rt_set_input_stats costs a call -- not part of pytest, and apart from bench.py.  One device-resident batch (bench.py's
wire-format generator: noise sigma 0.012, pulses at -62 .. -48 dBW, threshold -80 dBW) as uint8 pairs and as complex64, at the
reference's defaults (4 096 streams x 300 kS) and at BASELINE config 2 (256 streams x 2.048 MS); bench.py's pipelined loop (two
calls in flight) on an analyzer with the feature on -- every fetch followed by ``fetch_input_stats`` -- and on one without, the
two alternating ``--rounds`` times in one process so that both see the same clocks.

    python tests/perf/bench_input_stats.py [--workloads defaults config2] [--formats uint8 complex64] [--rounds 3] [--out FILE]

Prints (and with --out appends) one JSON line per workload and format: ms per call of every repeat, the SLOWEST repeat with the
feature on against the FASTEST without (the cost, stated the unkind way round), the medians, the bytes the statistics kernel reads
per call, and the records per call of both (they must agree: the analysis is the same)."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from oracle import analyze_oracle as oracle  # noqa: E402
from pyradiotracking_amd import synth  # noqa: E402
from pyradiotracking_amd.analyze import BatchSignalAnalyzer, default_lanes, input_levels  # noqa: E402

WORKLOADS = {
    "defaults": dict(streams=4096, sample_rate=300000, samples=300000, nperseg=256, window="hamming", steps=40,
                     what="the reference's defaults (4 096 streams x 300 kS, nperseg 256)"),
    "config2": dict(streams=256, sample_rate=2048000, samples=2048000, nperseg=256, window="hamming", steps=100, what="BASELINE config 2 geometry (bench.py's headline)"),
}
FORMATS = ("uint8", "complex64")
SAMPLE_BYTES = {"uint8": 2, "complex64": 8}


def make_inputs(w, formats):
    win = oracle.window_coefficients(w["window"], w["nperseg"])
    iq = synth.make_batch_device(w["streams"], w["samples"], w["sample_rate"], win, seed=1, noise_sigma=0.012, peak_dbw=(-62.0, -48.0))
    out = {}
    if "uint8" in formats:
        out["uint8"] = synth.quantize_u8_device(iq)
    if "complex64" in formats:
        out["complex64"] = iq
    torch.cuda.synchronize()
    return out


def timed(w, x, fmt, stats, settle=5):
    lanes = w.get("lanes", default_lanes(w["nperseg"], w["streams"]))
    b = BatchSignalAnalyzer([str(i) for i in range(w["streams"])], sample_rate=w["sample_rate"], fft_nperseg=w["nperseg"],
                            fft_window=w["window"], sdr_callback_length=w["samples"], lanes=lanes, signal_threshold_dbw=-80.0, input_stats=stats)
    put = {"uint8": b.enqueue_bytes, "complex64": b.enqueue}[fmt]
    last = [None]

    def loop(n):
        put(x)
        n_rec = 0
        for k in range(n):
            if k + 1 < n:
                put(x)  # two calls in flight
            n_rec += len(b.fetch_records())
            if stats:
                last[0] = b.fetch_input_stats()
        return n_rec

    loop(settle)  # (warm-up: AUTO settles on its level, clocks ramp)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n_rec = loop(w["steps"])
    dt = time.perf_counter() - t0
    b.close()
    return dt / w["steps"] * 1e3, n_rec // w["steps"], last[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=list(WORKLOADS))
    ap.add_argument("--formats", nargs="+", default=list(FORMATS))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=0, help="override the workloads' steps (a profiler run wants few)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    for name in a.workloads:
        w = dict(WORKLOADS[name])
        if a.steps:
            w["steps"] = a.steps
        inputs = make_inputs(w, a.formats)
        for fmt in a.formats:
            ms = {True: [], False: []}
            rec = {}
            rows = None
            for _ in range(a.rounds):
                for stats in (True, False):
                    t, n, got = timed(w, inputs[fmt], fmt, stats)
                    ms[stats].append(round(t, 4))
                    rec[stats] = n
                    rows = got if got is not None else rows
            assert rec[True] == rec[False], ("records per call differ", rec)
            lv = input_levels(rows)
            on_slow, off_fast = max(ms[True]), min(ms[False])
            line = {"metric": "input_stats_cost", "workload": name, "what": w["what"], "format": fmt, "streams": w["streams"], "samples": w["samples"],
                    "nperseg": w["nperseg"], "steps": w["steps"], "rounds": a.rounds, "ms_per_call_on": ms[True], "ms_per_call_off": ms[False],
                    "slowest_on_ms": on_slow, "fastest_off_ms": off_fast, "slowest_on_over_fastest_off": round(on_slow / off_fast, 4),
                    "median_on_ms": statistics.median(ms[True]), "median_off_ms": statistics.median(ms[False]),
                    "stats_bytes_per_call": w["streams"] * w["samples"] * SAMPLE_BYTES[fmt], "records_per_call": rec[True],
                    "mean_power_dbfs": round(float(lv["power_dbfs"].mean()), 3), "max_rail_fraction": float(lv["rail_fraction"].max())}
            print(json.dumps(line), flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(json.dumps(line) + "\n")
        del inputs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
