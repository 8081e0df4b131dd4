"""What keeping the sample tails costs a call, and how fast the gather moves snippets (``rt_set_record_iq``) -- not part of pytest,
and apart from bench.py, whose runs never call the entry.  One process, the variants timed ``--rounds`` times in alternation so that
all see the same clocks.

(a) ``cost``: the reference's defaults (300 kS/s, nperseg 256) at ``--streams`` streams x 300 kS with clean tag pulses, from
    complex64 and from the uint8 wire format in device memory, two calls in flight (bench.py's loop): a handle with the feature on
    at margin 0 against the same handle without it.  Seconds per call of both, and the excess from the SLOWEST repeat with against
    the FASTEST repeat without, beside the derived share of the tail copy -- 2 K N samples read and written per stream and call
    against the scan's B read.
(b) ``gather``: ``--gather-streams`` complex64 streams with a margin of 1024 segments, so that every record delivers its whole
    buffer (5.6 GB of snippets at the defaults): the time of ``fetch_records`` with the feature on less the time without it is
    the descriptor build, the upload and the gather; bytes / that time is quoted as a rate beside the chip's measured copy rate.

    python tests/perf/bench_record_iq.py [--streams 4096] [--rounds 5] [--steps 30] [--inputs c64 u8] [--gather-streams 96] [--out FILE]

Prints (and with --out appends, default profiles/record_iq_bench.jsonl) one JSON line per measurement.  For the kernels' own times
run it under ``rocprofv3 --kernel-trace --stats -- python tests/perf/bench_record_iq.py --rounds 1 --out ''`` and read ``iq_tails``
and ``record_iq_gather``."""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, HERE)

FS, SAMPLES, NPERSEG, WINDOW = 300000, 300000, 256, "hamming"
COPY_RATE_TBS = 6.29  # the chip's measured float4 copy rate (read + write bytes)


def make_input(streams, kind):
    from oracle import analyze_oracle as oracle
    from pyradiotracking_amd import synth

    win = oracle.window_coefficients(WINDOW, NPERSEG)
    if kind == "u8":
        iq = synth.make_batch_device(streams, SAMPLES, FS, win, seed=1, noise_sigma=0.012, peak_dbw=(-62.0, -48.0))
        return synth.quantize_u8_device(iq)
    return synth.make_batch_device(streams, SAMPLES, FS, win, seed=1)


def analyzer(streams, kind, margin):
    from pyradiotracking_amd.analyze import BatchSignalAnalyzer

    kw = dict(sample_rate=FS, fft_nperseg=NPERSEG, fft_window=WINDOW, sdr_callback_length=SAMPLES)
    if kind == "u8":
        kw["signal_threshold_dbw"] = -80.0
    if margin is not None:
        kw.update(record_iq=True, record_iq_margin=margin)
    return BatchSignalAnalyzer([str(i) for i in range(streams)], **kw)


def timed_calls(b, iq, kind, steps, settle=3):
    """seconds per call with two calls in flight, records per call"""
    import torch

    enq = b.enqueue_bytes if kind == "u8" else b.enqueue
    enq(iq)
    for _ in range(settle):
        enq(iq)
        b.fetch_records()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    for _ in range(steps):
        enq(iq)
        n += len(b.fetch_records())
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    b.fetch_records()
    return dt, n / steps


def timed_fetch(b, iq, steps, settle=2):
    """seconds of a serial fetch_records (the scan has ended: the stream is drained first), records and snippet bytes per call"""
    import torch

    t, n, nbytes = 0.0, 0, 0
    for i in range(settle + steps):
        b.enqueue(iq)
        torch.cuda.synchronize()
        time.sleep(0.05)  # (the call's kernels have ended: what is timed is the fetch alone)
        t0 = time.perf_counter()
        rec = b.fetch_records()
        dt = time.perf_counter() - t0
        if i >= settle:
            t += dt
            n += len(rec)
            if b.record_iq:
                nbytes += int(b.native.fetch_record_iq()[2].size)
    return t / steps, n / steps, nbytes / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--inputs", nargs="+", default=["u8", "c64"])
    ap.add_argument("--gather-streams", type=int, default=96)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "record_iq_bench.jsonl"))
    a = ap.parse_args()
    import torch

    from pyradiotracking_amd import _native

    if _native.device_count() < 1:
        raise SystemExit("bench_record_iq needs a GPU: nothing is measured without one")

    def emit(line):
        print(json.dumps(line), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")

    K = int(40e-3 * FS / NPERSEG) + 2  # tail columns at the reference's defaults (rt_core.h: tail_cols)
    for kind in a.inputs:
        iq = make_input(a.streams, kind)
        torch.cuda.synchronize()
        handles = {"with": analyzer(a.streams, kind, 0), "without": analyzer(a.streams, kind, None)}
        s = {v: [] for v in handles}
        rec = {}
        for _ in range(a.rounds):
            for v, b in handles.items():
                dt, r = timed_calls(b, iq, kind, a.steps)
                s[v].append(dt)
                rec[v] = r
        for b in handles.values():
            b.close()
        msamples = a.streams * SAMPLES / 1e6
        emit({"metric": "record_iq_cost", "input": kind, "streams": a.streams, "samples_per_buffer": SAMPLES, "sample_rate": FS, "nperseg": NPERSEG,
              "margin": 0, "rounds": a.rounds, "steps": a.steps, "s_per_call": {v: [round(x, 6) for x in s[v]] for v in s},
              "msamples_per_s_with_slowest": round(msamples / max(s["with"]), 1), "msamples_per_s_without_fastest": round(msamples / min(s["without"]), 1),
              "excess_pct_slowest_with_over_fastest_without": round(100.0 * (max(s["with"]) / min(s["without"]) - 1.0), 2),
              "excess_pct_best_over_best": round(100.0 * (min(s["with"]) / min(s["without"]) - 1.0), 2),
              "derived_tail_copy_share_pct": round(100.0 * 2 * K * NPERSEG / SAMPLES, 2), "records_per_call": rec})
        del iq
        torch.cuda.empty_cache()
    if a.gather_streams > 0:
        iq = make_input(a.gather_streams, "c64")
        torch.cuda.synchronize()
        handles = {"with": analyzer(a.gather_streams, "c64", 1024), "without": analyzer(a.gather_streams, "c64", None)}
        s = {v: [] for v in handles}
        rec = nbytes = 0
        for _ in range(a.rounds):
            for v, b in handles.items():
                dt, r, nb = timed_fetch(b, iq, max(2, a.steps // 10))
                s[v].append(dt)
                if v == "with":
                    rec, nbytes = r, nb
        for b in handles.values():
            b.close()
        extra = max(s["with"]) - min(s["without"])
        emit({"metric": "record_iq_gather", "streams": a.gather_streams, "margin": 1024, "records_per_call": rec, "snippet_bytes_per_call": nbytes,
              "s_fetch": {v: [round(x, 6) for x in s[v]] for v in s}, "s_gather_slowest_with_less_fastest_without": round(extra, 6),
              "gather_tb_per_s_read_plus_write": round(2 * nbytes / extra / 1e12, 3) if extra > 0 else None, "chip_copy_tb_per_s": COPY_RATE_TBS})


if __name__ == "__main__":
    main()
