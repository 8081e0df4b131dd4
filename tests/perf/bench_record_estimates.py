"""What ``fetch_record_estimates(k)`` costs (``rt_fetch_record_estimates``) beside what gives the same rows without it --
``fetch_record_fine(k)`` plus ``fetch_record_edges(k)``, the frames copied to the host and reduced there -- and beside
``fetch_record_stft(k)`` alone, on the same delivered calls.  Not part of pytest, and apart from bench.py, whose runs never call any
of them.  The record-IQ workload of README: the reference's defaults (300 kS/s, nperseg 256) at ``--streams`` streams x 300 kS
with clean tag pulses, margin 0, from the uint8 wire format and from complex64 in device memory.

One process, one handle.  After every fetch of a call's records the entries are timed one after the other, the order rotating from
call to call (``--rounds`` calls after one that allocates).  In front of every timed entry an untimed ``fetch_record_stft`` at a hop
that is in no entry (``--spoil``, default 2) makes the hop pool hold other frames, so every ``estimates_k`` and ``stft_k`` with
k > 1 pays for its frames' kernel as a first call does.  (k = 1 through Python is ``rt_fetch_record_stft``, whose values stay
cached per delivered call: ``stft_1`` and ``host_1`` after one another copy without the kernel, as they do for a caller.)

``record_edges`` is a Python loop over the records; beyond ``--edge-sample`` records (default 2 000) it is timed on the first
that many and scaled by the record count -- the line says so (``edges_sampled``).  Both the measured seconds and the scaled ones
are in the line.

    python tests/perf/bench_record_estimates.py [--streams 4096] [--rounds 5] [--inputs u8 c64] [--ks 1 4] [--out FILE]

Prints (and with --out appends, default profiles/record_estimates_bench.jsonl) one JSON line per input: every timing of every entry,
medians and (min, max).  For the kernel's own time run the script under ``rocprofv3 --kernel-trace --stats -- python
tests/perf/bench_record_estimates.py --rounds 2 --out ''`` (no counters in that run) and read ``record_estimates`` beside
``record_stft_hop``."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--inputs", nargs="+", default=["u8", "c64"])
    ap.add_argument("--ks", nargs="+", type=int, default=[1, 4])
    ap.add_argument("--spoil", type=int, default=2)
    ap.add_argument("--edge-sample", type=int, default=2000)
    ap.add_argument("--label", default="product")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "record_estimates_bench.jsonl"))
    a = ap.parse_args()
    import torch

    from bench_record_iq import FS, NPERSEG, SAMPLES, analyzer, make_input
    from pyradiotracking_amd import _native
    from pyradiotracking_amd.analyze import record_edges, record_fine

    if _native.device_count() < 1:
        raise SystemExit("bench_record_estimates needs a GPU: nothing is measured without one")
    assert a.spoil not in a.ks
    for kind in a.inputs:
        iq = make_input(a.streams, kind)
        torch.cuda.synchronize()
        b = analyzer(a.streams, kind, 0)
        enq = b.enqueue_bytes if kind == "u8" else b.enqueue
        entries = [f"{what}_{k}" for k in a.ks for what in ("estimates", "stft", "host")]
        s = {e: [] for e in entries}
        parts = {f"host_{k}": dict(fetch=[], fine=[], edges=[], edges_measured=[]) for k in a.ks}
        n_rec = sampled = 0
        frames = {}
        for i in range(a.rounds + 1):
            enq(iq)
            rec = b.fetch_records()
            torch.cuda.synchronize()
            n_rec = len(rec)
            order = entries[i % len(entries):] + entries[:i % len(entries)]
            for what in order:
                kind_of, k = what.rsplit("_", 1)
                k = int(k)
                got = None
                b.native.fetch_record_stft(a.spoil)  # (untimed: the hop pool holds another hop's frames now)
                t0 = time.perf_counter()
                if kind_of == "estimates":
                    got = b.fetch_record_estimates(hop_div=k)
                    dt = time.perf_counter() - t0
                elif kind_of == "stft":
                    got = b.fetch_record_stft(hop_div=k)
                    dt = time.perf_counter() - t0
                    frames[k] = int(got[2].size)
                else:  # fetch_record_fine(k) + fetch_record_edges(k), in their parts: each fetches the frames for itself
                    off, first, values = b.fetch_record_stft(hop_div=k)
                    t1 = time.perf_counter()
                    record_fine(off, first, values, rec["start"], rec["end"], b.sample_rate, b.fft_nperseg, k, rec["fi"])
                    t2 = time.perf_counter()
                    off, first, values = b.fetch_record_stft(hop_div=k)
                    t3 = time.perf_counter()
                    m = min(n_rec, a.edge_sample)
                    sampled = m if m < n_rec else 0
                    record_edges(off[:m + 1], first[:m], values[:off[m]], rec["start"][:m], rec["end"][:m], b.fft_nperseg, k)
                    t4 = time.perf_counter()
                    edges = (t4 - t3) * (n_rec / m if m else 1.0)
                    dt = (t3 - t0) + edges
                    if i:
                        p = parts[what]
                        p["fetch"].append((t1 - t0) + (t3 - t2))
                        p["fine"].append(t2 - t1)
                        p["edges"].append(edges)
                        p["edges_measured"].append(t4 - t3)
                if i:  # (the first call allocates the pools and the tables)
                    s[what].append(dt)
            got = None
        b.close()

        def stat(v):
            return dict(median=round(statistics.median(v), 6), min=round(min(v), 6), max=round(max(v), 6))

        line = {"metric": "record_estimates_cost", "label": a.label, "input": kind, "streams": a.streams, "samples_per_buffer": SAMPLES, "sample_rate": FS,
                "nperseg": NPERSEG, "margin": 0, "rounds": a.rounds, "records_per_call": n_rec, "frames": frames, "row_bytes": 72 * n_rec,
                "edges_sampled": sampled, "s": {e: [round(x, 6) for x in v] for e, v in s.items()}, "stats": {e: stat(v) for e, v in s.items()},
                "host_parts": {e: {name: stat(v) for name, v in p.items()} for e, p in parts.items()}}
        print(json.dumps(line), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")
        del iq
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
