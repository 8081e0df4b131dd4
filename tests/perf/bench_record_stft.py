"""What ``fetch_record_stft`` costs against ``fetch_record_iq`` on the same calls (``rt_fetch_record_stft``) -- not part of pytest, and
apart from bench.py, whose runs never call either entry.  The record-IQ workload of README: the reference's defaults (300 kS/s,
nperseg 256) at ``--streams`` streams x 300 kS with clean tag pulses, margin 0, from the uint8 wire format and from complex64 in
device memory.  One process, one handle; after every fetch of a call's records the two entries are timed in alternation
(``--rounds`` calls): ``fetch_record_iq`` is what a user has today (the snippets to the host), ``fetch_record_stft`` the kernel over
the snippet pool plus the copy of one complex value a segment.  Reported: seconds of each, the slowest new repeat against the
fastest old one, bytes delivered by each, and the pool bytes over the new entry's time as a lower bound of the kernel's read rate.

    python tests/perf/bench_record_stft.py [--streams 4096] [--rounds 5] [--inputs u8 c64] [--out FILE]

Prints (and with --out appends, default profiles/record_stft_bench.jsonl) one JSON line per input.  For the kernel's own time and
read rate run it under ``rocprofv3 --kernel-trace --stats -- python tests/perf/bench_record_stft.py --rounds 2 --out ''`` and read
``record_stft`` beside ``record_iq_gather``: pool bytes / kernel time against 2 x pool bytes / gather time."""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_record_iq import FS, NPERSEG, SAMPLES, analyzer, make_input  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--inputs", nargs="+", default=["u8", "c64"])
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "record_stft_bench.jsonl"))
    a = ap.parse_args()
    import torch

    from pyradiotracking_amd import _native

    if _native.device_count() < 1:
        raise SystemExit("bench_record_stft needs a GPU: nothing is measured without one")
    for kind in a.inputs:
        iq = make_input(a.streams, kind)
        torch.cuda.synchronize()
        b = analyzer(a.streams, kind, 0)
        enq = b.enqueue_bytes if kind == "u8" else b.enqueue
        s = {"record_iq": [], "record_stft": [], "record_stft_again": []}
        n_rec = n_cells = n_bytes = 0
        for i in range(a.rounds + 1):
            enq(iq)
            rec = b.fetch_records()
            torch.cuda.synchronize()
            order = ("record_iq", "record_stft") if i % 2 else ("record_stft", "record_iq")
            t = {}
            for what in order:
                got = None  # (the previous result is freed here, outside the timed region: the snippets are gigabytes)
                t0 = time.perf_counter()
                got = b.native.fetch_record_iq() if what == "record_iq" else b.native.fetch_record_stft()
                t[what] = time.perf_counter() - t0
                if what == "record_iq":
                    n_bytes = int(got[2].size)
                else:
                    n_cells = int(got[2].size)
            got = None
            t0 = time.perf_counter()
            b.native.fetch_record_stft()  # (the values stand: the copy alone)
            t["record_stft_again"] = time.perf_counter() - t0
            n_rec = len(rec)
            if i:  # (the first call allocates the pools and the table)
                for k, v in t.items():
                    s[k].append(v)
        b.close()
        line = {"metric": "record_stft_cost", "input": kind, "streams": a.streams, "samples_per_buffer": SAMPLES, "sample_rate": FS, "nperseg": NPERSEG,
                "margin": 0, "rounds": a.rounds, "records_per_call": n_rec, "snippet_bytes": n_bytes, "value_bytes": n_cells * 8,
                "s": {k: [round(x, 6) for x in v] for k, v in s.items()},
                "slowest_stft_over_fastest_iq": round(max(s["record_stft"]) / min(s["record_iq"]), 4),
                "pool_gb_per_s_over_whole_entry_slowest": round(n_bytes / max(s["record_stft"]) / 1e9, 1)}
        print(json.dumps(line), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")
        del iq
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
