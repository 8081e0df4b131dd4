"""What ``fetch_record_stft(hop_div=k)`` costs (``rt_fetch_record_stft_hop``) beside ``fetch_record_stft()`` and ``fetch_record_iq()``
on the same delivered calls -- not part of pytest, and apart from bench.py, whose runs never call any of them.  The record-IQ
workload of README: the reference's defaults (300 kS/s, nperseg 256) at ``--streams`` streams x 300 kS with clean tag pulses,
margin 0, from the uint8 wire format and from complex64 in device memory.  One process, one handle; after every fetch of a call's
records the entries are timed one after the other, the order rotating from call to call (``--rounds`` calls after one that
allocates): every hop is another k than the one before it, so each timing is the kernel plus the copy of its frames.

    python tests/perf/bench_record_stft_hop.py [--streams 4096] [--rounds 5] [--inputs u8 c64] [--ks 1 2 4 8] [--no-iq] [--lib FILE] [--out FILE]

Prints (and with --out appends, default profiles/record_stft_hop_bench.jsonl) one JSON line per input: seconds of each entry, the
frames of each k, microseconds per thousand frames beside ``record_stft``'s per thousand segments.

The lane-group A/B: ``--build-g64`` compiles the library once more with ``-DRT_STFT_HOP_FORCE_G64`` (every frame on a whole wave,
as ``record_stft`` runs) to ``librt_analyze_hop_g64.so`` beside the product, and ``--lib`` loads that file instead of the product;
run ``--inputs u8 --ks 4 --no-iq`` in alternating processes, with and without ``--lib``.  For the kernel's own time run the script
under ``rocprofv3 --kernel-trace --stats -- python tests/perf/bench_record_stft_hop.py --rounds 2 --out ''`` (no counters in that
run) and read ``record_stft_hop`` beside ``record_stft``."""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

G64_LIB = os.path.join(HERE, "pyradiotracking_amd", "librt_analyze_hop_g64.so")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--inputs", nargs="+", default=["u8", "c64"])
    ap.add_argument("--ks", nargs="+", type=int, default=[1, 2, 4, 8])
    ap.add_argument("--no-iq", action="store_true", help="leave fetch_record_iq out (the A/B: gigabytes a call that tell nothing there)")
    ap.add_argument("--lib", default=None, help="load this build of the library instead of the product")
    ap.add_argument("--build-g64", action="store_true", help="compile the G = 64 variant and exit")
    ap.add_argument("--label", default="product")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "record_stft_hop_bench.jsonl"))
    a = ap.parse_args()
    if a.build_g64:
        from pyradiotracking_amd import build

        subprocess.run(build._library_cmd(G64_LIB, ("-DRT_STFT_HOP_FORCE_G64",)), check=True)
        print("built", G64_LIB)
        return
    if a.lib:
        os.environ["RT_ANALYZE_LIB"] = a.lib  # (_native's own override for A/B builds of the kernels, read at the first load)
    from pyradiotracking_amd import _native

    import torch

    from bench_record_iq import FS, NPERSEG, SAMPLES, analyzer, make_input

    if _native.device_count() < 1:
        raise SystemExit("bench_record_stft_hop needs a GPU: nothing is measured without one")
    for kind in a.inputs:
        iq = make_input(a.streams, kind)
        torch.cuda.synchronize()
        b = analyzer(a.streams, kind, 0)
        enq = b.enqueue_bytes if kind == "u8" else b.enqueue
        entries = ["record_stft"] + [f"hop_{k}" for k in a.ks] + ([] if a.no_iq else ["record_iq"])
        s = {e: [] for e in entries}
        count = {}
        n_rec = n_bytes = 0
        for i in range(a.rounds + 1):
            enq(iq)
            rec = b.fetch_records()
            torch.cuda.synchronize()
            order = entries[i % len(entries):] + entries[:i % len(entries)]
            for what in order:
                got = None  # (the previous result is freed here, outside the timed region: the snippets are gigabytes)
                t0 = time.perf_counter()
                if what == "record_iq":
                    got = b.native.fetch_record_iq()
                elif what == "record_stft":
                    got = b.native.fetch_record_stft()
                else:
                    got = b.native.fetch_record_stft(int(what[4:]))
                dt = time.perf_counter() - t0
                if what == "record_iq":
                    n_bytes = int(got[2].size)
                else:
                    count[what] = int(got[2].size)
                if i:  # (the first call allocates the pools and the table)
                    s[what].append(dt)
            got = None
            n_rec = len(rec)
        b.close()
        per_k = {e: round(1e9 * min(s[e]) / max(count[e], 1), 3) for e in entries if e != "record_iq"}
        line = {"metric": "record_stft_hop_cost", "label": a.label, "input": kind, "streams": a.streams, "samples_per_buffer": SAMPLES, "sample_rate": FS,
                "nperseg": NPERSEG, "margin": 0, "rounds": a.rounds, "records_per_call": n_rec, "snippet_bytes": n_bytes, "values": count,
                "s": {k: [round(x, 6) for x in v] for k, v in s.items()}, "fastest_us_per_1000_values": per_k}
        print(json.dumps(line), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")
        del iq
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
