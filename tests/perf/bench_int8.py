"""Throughput of the four input formats on the same signal -- not part of pytest, and apart from bench.py.  One device-resident
batch (bench.py's wire-format generator: noise sigma 0.012, pulses at -62 .. -48 dBW, threshold -80 dBW) as int8 pairs
(``enqueue_int8``), as the complex64 array those pairs convert to exactly (``enqueue``: what the int8 rate is judged against on
the same values), as uint8 pairs (``enqueue_bytes``: the same 2 bytes a sample) and as int16 pairs (``enqueue_int16``) of the same
signal; bench.py's pipelined loop (two calls in flight) for each.  The four alternate ``--rounds`` times per workload on one box
and the best round of each is kept, so that all see the same clocks.

    python tests/perf/bench_int8.py [--workloads config2 defaults] [--rounds 3] [--out FILE]

Prints (and with --out appends) one JSON line per workload: MS/s and ms per step of each format, the records per step (int8 and
complex64 must agree -- the same values -- and the run fails if they do not), and the int8 rate relative to the complex64 and
uint8 rates."""
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

# bench.py's geometries
WORKLOADS = {
    "config2": dict(streams=256, sample_rate=2048000, samples=2048000, nperseg=256, window="hamming", steps=100, what="BASELINE config 2 geometry (bench.py's headline)"),
    "defaults": dict(streams=4096, sample_rate=300000, samples=300000, nperseg=256, window="hamming", steps=40,
                     what="the reference's defaults (4 096 streams x 300 kS, nperseg 256)"),
}
FORMATS = ("int8", "uint8", "int16", "complex64")


def make_inputs(w):
    win = oracle.window_coefficients(w["window"], w["nperseg"])
    iq = synth.make_batch_device(w["streams"], w["samples"], w["sample_rate"], win, seed=1, noise_sigma=0.012, peak_dbw=(-62.0, -48.0))
    i8 = synth.quantize_i8_device(iq)
    u8 = synth.quantize_u8_device(iq)
    i16 = synth.quantize_i16_device(iq)
    del iq
    c64 = torch.view_as_complex((i8.to(torch.float32) * (2.0 ** -7)).reshape(w["streams"], w["samples"], 2).contiguous())  # exact
    torch.cuda.synchronize()
    return {"int8": i8, "uint8": u8, "int16": i16, "complex64": c64}


def timed(w, x, fmt, settle=5):
    lanes = w.get("lanes", default_lanes(w["nperseg"], w["streams"]))
    b = BatchSignalAnalyzer([str(i) for i in range(w["streams"])], sample_rate=w["sample_rate"], fft_nperseg=w["nperseg"],
                            fft_window=w["window"], sdr_callback_length=w["samples"], lanes=lanes, signal_threshold_dbw=-80.0)
    put = {"int8": b.enqueue_int8, "uint8": b.enqueue_bytes, "int16": b.enqueue_int16, "complex64": b.enqueue}[fmt]
    steps = w["steps"]

    def loop(n):
        put(x)
        n_rec = 0
        for k in range(n):
            if k + 1 < n:
                put(x)  # two calls in flight
            n_rec += len(b.fetch_records())
        return n_rec

    loop(settle)  # (warm-up: AUTO settles on its level, clocks ramp)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n_rec = loop(steps)
    dt = time.perf_counter() - t0
    info = b.call_info()
    b.close()
    return w["streams"] * w["samples"] * steps / dt / 1e6, dt / steps * 1e3, n_rec // steps, int(info.mode_used)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=list(WORKLOADS))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=0, help="override the workloads' steps (a profiler run wants few)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    for name in a.workloads:
        w = dict(WORKLOADS[name])
        if a.steps:
            w["steps"] = a.steps
        inputs = make_inputs(w)
        best = {f: None for f in FORMATS}
        for _ in range(a.rounds):
            for f in FORMATS:
                r = timed(w, inputs[f], f)
                if best[f] is None or r[0] > best[f][0]:
                    best[f] = r
            assert best["int8"][2] == best["complex64"][2], ("records per step differ", best["int8"][2], best["complex64"][2])
        line = {"metric": "input_format_rates", "workload": name, "what": w["what"], "streams": w["streams"], "samples": w["samples"],
                "nperseg": w["nperseg"], "steps": w["steps"], "rounds": a.rounds}
        for f in FORMATS:
            line["msamples_per_s_" + f] = round(best[f][0], 1)
            line["ms_per_step_" + f] = round(best[f][1], 4)
            line["records_per_step_" + f] = best[f][2]
            line["mode_used_" + f] = best[f][3]
        line["int8_over_complex64"] = round(best["int8"][0] / best["complex64"][0], 4)
        line["int8_over_uint8"] = round(best["int8"][0] / best["uint8"][0], 4)
        line["int8_over_int16"] = round(best["int8"][0] / best["int16"][0], 4)
        del inputs
        torch.cuda.empty_cache()
        print(json.dumps(line), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
