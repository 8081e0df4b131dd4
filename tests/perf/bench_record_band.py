"""What ``fetch_record_band(k, w)`` costs (``rt_fetch_record_band``) beside ``fetch_record_stft(hop_div=k)`` -- the w = 0 cost -- and
beside ``fetch_record_iq()``, the route that exists without it (the snippets to the host, an FFT there), on the same delivered
calls.  Not part of pytest, and apart from bench.py, whose runs never call any of them.  The record-IQ workload of README: the
reference's defaults (300 kS/s, nperseg 256) at ``--streams`` streams x 300 kS with clean tag pulses, margin 0, from the uint8 wire
format and from complex64 in device memory.

One process, one handle per input.  After every fetch of a call's records the entries are timed one after the other, the order
rotating from call to call (``--rounds`` calls after one that allocates).  In front of every timed entry an untimed
``fetch_record_band`` at a pair that is in no entry and an untimed ``fetch_record_stft`` at a hop that is in no entry make the two
pools hold other values, so every timed ``band_k_w`` and ``stft_k`` with k > 1 pays for its kernel as a first call does.  (k = 1
through ``fetch_record_stft`` is ``rt_fetch_record_stft``, whose values stay cached per delivered call.)

    python tests/perf/bench_record_band.py [--streams 4096] [--rounds 5] [--inputs u8 c64] [--out FILE]

The table A/B: ``--build-lds`` compiles the library once more with ``-DRT_BAND_LDS_TABLE`` (every workgroup of ``record_band`` copies
the twiddle table to LDS and gathers from there) to ``librt_analyze_band_lds.so`` beside the product, and ``--lib`` loads that file
instead of the product; ``--label`` names the variant in the line.

Prints (and with --out appends, default profiles/record_band_bench.jsonl) one JSON line per input: milliseconds (median, min, max),
frames and bytes delivered per entry.  For the kernels' own time run the script under ``rocprofv3 --kernel-trace --stats -- python
tests/perf/bench_record_band.py --rounds 2 --out ''`` (no counters in that run) and read ``record_band`` beside
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

LDS_LIB = os.path.join(HERE, "pyradiotracking_amd", "librt_analyze_band_lds.so")
PAIRS = ((1, 0), (1, 2), (1, 8), (4, 2))
SPOIL_PAIR, SPOIL_HOP = (2, 1), 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--inputs", nargs="+", default=["u8", "c64"])
    ap.add_argument("--label", default="product")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "record_band_bench.jsonl"))
    ap.add_argument("--build-lds", action="store_true", help="compile the LDS-table variant and exit")
    ap.add_argument("--lib", default=None, help="load this library instead of the product")
    a = ap.parse_args()
    if a.build_lds:
        import subprocess

        from pyradiotracking_amd import build

        subprocess.run(build._library_cmd(LDS_LIB, ("-DRT_BAND_LDS_TABLE",)), check=True)
        print("built", LDS_LIB)
        return
    if a.lib:
        os.environ["RT_ANALYZE_LIB"] = a.lib  # (_native's own override for A/B builds of the kernels, read at the first load)
    import torch

    from bench_record_iq import FS, NPERSEG, SAMPLES, analyzer, make_input
    from pyradiotracking_amd import _native

    if _native.device_count() < 1:
        raise SystemExit("bench_record_band needs a GPU: nothing is measured without one")
    for kind in a.inputs:
        iq = make_input(a.streams, kind)
        torch.cuda.synchronize()
        b = analyzer(a.streams, kind, 0)
        enq = b.enqueue_bytes if kind == "u8" else b.enqueue
        entries = [f"band_{k}_{w}" for k, w in PAIRS] + [f"stft_{k}" for k in sorted({k for k, _ in PAIRS})] + ["iq"]
        s = {e: [] for e in entries}
        frames, nbytes = {}, {}
        n_rec = 0
        for i in range(a.rounds + 1):
            enq(iq)
            rec = b.fetch_records()
            torch.cuda.synchronize()
            n_rec = len(rec)
            order = entries[i % len(entries):] + entries[:i % len(entries)]
            for what in order:
                got = None
                b.native.fetch_record_band(*SPOIL_PAIR)      # (untimed: the band pool holds another pair's values now)
                b.native.fetch_record_stft(SPOIL_HOP)        # (... and the hop pool another hop's frames)
                t0 = time.perf_counter()
                if what.startswith("band_"):
                    k, w = (int(v) for v in what.split("_")[1:])
                    got = b.fetch_record_band(k, w)
                    dt = time.perf_counter() - t0
                    frames[what], nbytes[what] = int(got[2].shape[0]), int(got[2].nbytes)
                elif what.startswith("stft_"):
                    got = b.fetch_record_stft(hop_div=int(what.split("_")[1]))
                    dt = time.perf_counter() - t0
                    frames[what], nbytes[what] = int(got[2].size), int(got[2].nbytes)
                else:
                    got = b.fetch_record_iq()
                    dt = time.perf_counter() - t0
                    frames[what], nbytes[what] = int(got[0][-1]) // NPERSEG, int(got[2].nbytes)
                if i:  # (the first call allocates the pools and the tables)
                    s[what].append(dt * 1e3)
            got = None
        b.close()

        def stat(v):
            return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))

        line = {"metric": "record_band_cost", "label": a.label, "input": kind, "streams": a.streams, "samples_per_buffer": SAMPLES, "sample_rate": FS,
                "nperseg": NPERSEG, "margin": 0, "rounds": a.rounds, "records_per_call": n_rec, "frames": frames, "bytes": nbytes,
                "ms": {e: stat(v) for e, v in s.items()}, "all_ms": {e: [round(x, 4) for x in v] for e, v in s.items()}}
        print(json.dumps(line), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")
        del iq
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
