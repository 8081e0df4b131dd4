"""Cost of the cells behind every record (``record_cells=True``, RT_FLAG_RECORD_CELLS) -- not part of pytest, and apart from
bench.py, whose plain run keeps the flag off.  bench.py's pipelined loop (two calls in flight) on one box, with the flag and a
``fetch_record_cells()`` after every ``fetch_records()``, and without them; the two alternate ``--rounds`` times per workload
and the best round of each is kept, so that both see the same clocks.

    python tests/perf/bench_record_cells.py [--workloads config2 defaults ...] [--rounds 3] [--out FILE]

``--no-fetch`` keeps the flag but leaves the ``fetch_record_cells()`` out: what the gather kernels cost without the copy.
Prints (and with --out appends) one JSON line per workload: MS/s without and with the flag, the throughput lost, and the
records and cells fetched per step."""
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
    "defaults": dict(streams=4096, sample_rate=300000, samples=300000, nperseg=256, window="hamming", steps=40,
                     what="the reference's defaults (300 kS/s, nperseg 256, -90 dBW), clean input"),
    "defaults_noise_floor": dict(streams=4096, sample_rate=300000, samples=300000, nperseg=256, window="hamming", steps=40, noise_dbw=-88.0,
                                 what="the reference's defaults with the noise floor at -88 dBW, 2 dB over the threshold (AUTO climbs)"),
    "config5_share": dict(streams=1024, sample_rate=3200000, samples=3200000, nperseg=4096, window="hamming", steps=20, trains=True, lanes=1,
                          what="BASELINE config 5, one GPU's share (nperseg 4096, tag trains)"),
    "nperseg300": dict(streams=1024, sample_rate=300000, samples=300000, nperseg=300, window="hann", steps=20,
                       what="nperseg 300: Bluestein's algorithm on the dense path"),
    "float64_n256": dict(streams=256, sample_rate=2048000, samples=2048000, nperseg=256, window="hamming", steps=5, precision="float64",
                         what="a float64 handle at config 2's geometry (complex128)"),
}


def make_input(w):
    win = oracle.window_coefficients(w["window"], w["nperseg"])
    kw = dict(trains=w.get("trains", False))
    if "noise_dbw" in w:
        kw["noise_sigma"] = float((10.0 ** (w["noise_dbw"] / 10.0) * w["sample_rate"] / 2.0) ** 0.5)
    iq = synth.make_batch_device(w["streams"], w["samples"], w["sample_rate"], win, seed=1, **kw)
    if w.get("precision") == "float64":
        iq = iq.to(torch.complex128)
    return iq


def timed(w, iq, flag, settle=5, fetch=True):
    lanes = w.get("lanes", 1 if w.get("precision") == "float64" else default_lanes(w["nperseg"], w["streams"]))
    b = BatchSignalAnalyzer([str(i) for i in range(w["streams"])], sample_rate=w["sample_rate"], fft_nperseg=w["nperseg"],
                            fft_window=w["window"], sdr_callback_length=w["samples"], lanes=lanes, record_cells=flag,
                            precision=w.get("precision", "float32"))
    steps = w["steps"]

    def loop(n):
        b.enqueue(iq)
        n_rec = n_cells = 0
        for k in range(n):
            if k + 1 < n:
                b.enqueue(iq)  # two calls in flight
            n_rec += len(b.fetch_records())
            if flag and fetch:
                n_cells += len(b.fetch_record_cells()[1])
        return n_rec, n_cells

    loop(settle)  # (warm-up: AUTO settles on its level, clocks ramp)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n_rec, n_cells = loop(steps)
    dt = time.perf_counter() - t0
    info = b.call_info()
    b.close()
    return w["streams"] * w["samples"] * steps / dt / 1e6, dt / steps * 1e3, n_rec, int(info.mode_used), n_cells


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=list(WORKLOADS))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-fetch", action="store_true", help="with the flag, but without fetch_record_cells(): the gather kernels' share alone")
    a = ap.parse_args()
    for name in a.workloads:
        w = WORKLOADS[name]
        iq = make_input(w)
        best = {False: None, True: None}
        for _ in range(a.rounds):
            for flag in (False, True):
                r = timed(w, iq, flag, fetch=not a.no_fetch)
                if best[flag] is None or r[0] > best[flag][0]:
                    best[flag] = r
        off, on = best[False], best[True]
        line = {"metric": "record_cells_cost" + ("_kernels_only" if a.no_fetch else ""), "workload": name, "what": w["what"], "streams": w["streams"], "samples": w["samples"],
                "nperseg": w["nperseg"], "precision": w.get("precision", "float32"), "steps": w["steps"], "rounds": a.rounds,
                "msamples_per_s_off": round(off[0], 1), "msamples_per_s_on": round(on[0], 1),
                "ms_per_step_off": round(off[1], 4), "ms_per_step_on": round(on[1], 4),
                "throughput_lost_pct": round(100.0 * (1.0 - on[0] / off[0]), 2), "records_off": off[2], "records_on": on[2],
                "cells_per_step": on[4] // w["steps"], "mode_used": on[3]}
        del iq
        torch.cuda.empty_cache()
        print(json.dumps(line), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
