"""What chaining buys a recording, and what its copy costs (``rt_set_chain``) -- not part of pytest, and apart from bench.py, whose
runs never call the entry.  One recording of ``--buffers`` one-second buffers at the reference's defaults (300 kS/s, nperseg 256),
from complex64 and from the uint8 wire format, in device memory; one process, the variants timed ``--rounds`` times in alternation
so that all see the same clocks.

(a) ``chained``: a handle of ``buffers`` streams with ``rt_set_chain(buffers)``, the whole recording in ONE call, against
    ``sequential``: a one-stream plain handle, ``buffers`` calls with two in flight (bench.py's loop).  MS/s of both and the ratio,
    from the SLOWEST chained repeat and the FASTEST sequential one.
(b) the price of the copy: ``independent``, the same buffers as a plain handle of ``buffers`` independent streams in one call,
    against ``chained`` (slowest chained over fastest independent), beside the derived share 2 K N 4 / (B 8) of the scan's traffic.

    python tests/perf/bench_chain.py [--buffers 256] [--rounds 5] [--steps 100] [--inputs c64 u8] [--out FILE]

Prints (and with --out appends, default profiles/chain_bench.jsonl) one JSON line per input.  For the kernel's own time run it
under ``rocprofv3 --kernel-trace --stats -- python tests/perf/bench_chain.py --rounds 1 --out ''`` and read ``chain_tails``."""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, HERE)

FS, SAMPLES, NPERSEG, WINDOW = 300000, 300000, 256, "hamming"


def make_input(buffers, kind):
    from oracle import analyze_oracle as oracle
    from pyradiotracking_amd import synth

    win = oracle.window_coefficients(WINDOW, NPERSEG)
    if kind == "u8":
        iq = synth.make_batch_device(buffers, SAMPLES, FS, win, seed=1, noise_sigma=0.012, peak_dbw=(-62.0, -48.0))
        return synth.quantize_u8_device(iq)
    return synth.make_batch_device(buffers, SAMPLES, FS, win, seed=1)


def analyzer(n_streams, kind, links=0):
    from pyradiotracking_amd.analyze import BatchSignalAnalyzer

    kw = dict(sample_rate=FS, fft_nperseg=NPERSEG, fft_window=WINDOW, sdr_callback_length=SAMPLES, lanes=1)
    if kind == "u8":
        kw["signal_threshold_dbw"] = -80.0
    b = BatchSignalAnalyzer([str(i) for i in range(n_streams)], **kw)
    if links:
        b.native.set_chain(links)
    return b


def timed(variant, iq, kind, buffers, steps, settle=2):
    """(seconds per pass over the recording, records per pass)"""
    import torch

    enq = (lambda b, x: b.enqueue_bytes(x)) if kind == "u8" else (lambda b, x: b.enqueue(x))
    if variant == "sequential":
        b = analyzer(1, kind)

        def one_pass():
            n = 0
            enq(b, iq[0:1])
            for k in range(buffers):
                if k + 1 < buffers:
                    enq(b, iq[k + 1:k + 2])  # two calls in flight
                n += len(b.fetch_records())
            return n
        steps = max(1, steps // 4)
    else:
        b = analyzer(buffers, kind, buffers if variant == "chained" else 0)

        def one_pass():
            enq(b, iq)
            return len(b.fetch_records())
    for _ in range(settle):
        one_pass()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n_rec = 0
    for _ in range(steps):
        n_rec += one_pass()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    b.close()
    return dt, n_rec / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--buffers", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--inputs", nargs="+", default=["u8", "c64"])
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "chain_bench.jsonl"))
    a = ap.parse_args()
    import torch

    from pyradiotracking_amd import _native

    if _native.device_count() < 1:
        raise SystemExit("bench_chain needs a GPU: nothing is measured without one")
    variants = ("chained", "independent", "sequential")
    for kind in a.inputs:
        iq = make_input(a.buffers, kind)
        torch.cuda.synchronize()
        s = {v: [] for v in variants}
        rec = {}
        for _ in range(a.rounds):
            for v in variants:
                dt, r = timed(v, iq, kind, a.buffers, a.steps)
                s[v].append(dt)
                rec[v] = r
        msamples = a.buffers * SAMPLES / 1e6
        K = int(40e-3 * FS / NPERSEG) + 2  # tail columns at the reference's defaults (rt_core.h: tail_cols)
        line = {"metric": "chain", "input": kind, "buffers": a.buffers, "samples_per_buffer": SAMPLES, "sample_rate": FS, "nperseg": NPERSEG,
                "rounds": a.rounds, "steps": a.steps,
                "s_per_recording": {v: [round(x, 6) for x in s[v]] for v in variants},
                "msamples_per_s_chained_slowest": round(msamples / max(s["chained"]), 1),
                "msamples_per_s_sequential_fastest": round(msamples / min(s["sequential"]), 1),
                "msamples_per_s_independent_fastest": round(msamples / min(s["independent"]), 1),
                "chained_over_sequential_rate": round(min(s["sequential"]) / max(s["chained"]), 3),
                "copy_excess_pct_slowest_chained_over_fastest_independent": round(100.0 * (max(s["chained"]) / min(s["independent"]) - 1.0), 2),
                "copy_excess_pct_best_over_best": round(100.0 * (min(s["chained"]) / min(s["independent"]) - 1.0), 2),
                "derived_copy_share_pct": round(100.0 * 2 * K * NPERSEG * 4 / (SAMPLES * (2 if kind == "u8" else 8)), 2),
                "records_per_recording": rec}
        print(json.dumps(line), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")
        del iq
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
