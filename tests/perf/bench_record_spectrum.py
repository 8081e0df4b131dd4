"""What ``fetch_record_spectrum(k, w)`` costs (``rt_fetch_record_spectrum``) beside the pair it replaces -- ``fetch_record_band(k, w)``
followed by ``record_band_rows`` on the host -- on the same delivered calls.  Not part of pytest, and apart from bench.py, whose runs
never call any of them.  The record-IQ workload of README: the reference's defaults (300 kS/s, nperseg 256) at ``--streams`` streams
x 300 kS with clean tag pulses, margin 0, from the uint8 wire format and from complex64 in device memory.

One process, one handle per input.  After every fetch of a call's records the entries are timed one after the other, the order
rotating from call to call (``--rounds`` calls after one that allocates):

    spectrum_k_w   the new entry as a first call pays for it: band kernel, reduction kernel, rows, means and peaks to the host.  An
                   untimed ``fetch_record_spectrum`` at a pair that is in no entry makes both pools hold other values first.
    reduce_k_w     the new entry with the band pool already holding (k, w): the reduction kernel and the copies alone
    band_k_w       ``fetch_record_band(k, w)`` as a first call pays for it: band kernel, every frame to the host

``record_band_rows`` on what ``band_k_w`` returned is timed apart, once per pair, on the first ``--host-records`` records of the
call and scaled to all of them (it walks the records in Python; ``host_rows_ms_scaled``).

    python tests/perf/bench_record_spectrum.py [--streams 4096] [--rounds 5] [--inputs u8 c64] [--out FILE]

Prints (and with --out appends, default profiles/record_spectrum_bench.jsonl) one JSON line per input: milliseconds (median, min,
max) and bytes delivered per entry.  For the kernels' own time run the script under ``rocprofv3 --kernel-trace --stats -- python
tests/perf/bench_record_spectrum.py --rounds 2 --host-records 0 --out ''`` (no counters in that run) and read ``record_spectrum``
beside ``record_band``."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

PAIRS = ((1, 2), (1, 8), (4, 2))
SPOIL_PAIR = (2, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--inputs", nargs="+", default=["u8", "c64"])
    ap.add_argument("--host-records", type=int, default=4000, help="records record_band_rows is timed on (0: not timed)")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "record_spectrum_bench.jsonl"))
    a = ap.parse_args()
    import numpy as np
    import torch

    from bench_record_iq import FS, NPERSEG, SAMPLES, analyzer, make_input
    from pyradiotracking_amd import _native
    from pyradiotracking_amd.analyze import record_band_rows

    if _native.device_count() < 1:
        raise SystemExit("bench_record_spectrum needs a GPU: nothing is measured without one")
    for kind in a.inputs:
        iq = make_input(a.streams, kind)
        torch.cuda.synchronize()
        b = analyzer(a.streams, kind, 0)
        enq = b.enqueue_bytes if kind == "u8" else b.enqueue
        entries = [f"{what}_{k}_{w}" for k, w in PAIRS for what in ("spectrum", "reduce", "band")]
        s = {e: [] for e in entries}
        nbytes, frames, host_ms = {}, {}, {}
        n_rec = 0
        for i in range(a.rounds + 1):
            enq(iq)
            rec = b.fetch_records()
            torch.cuda.synchronize()
            n_rec = len(rec)
            order = entries[i % len(entries):] + entries[:i % len(entries)]
            for what in order:
                name, k, w = what.split("_")
                k, w = int(k), int(w)
                b.native.fetch_record_spectrum(*SPOIL_PAIR)  # (untimed: the band pool and the row pool hold another pair's values now)
                got = None
                if name == "reduce":
                    b.native.fetch_record_band(k, w)         # (untimed: the band pool holds the pair, the row pool does not)
                t0 = time.perf_counter()
                if name == "band":
                    got = b.fetch_record_band(k, w)
                    dt = time.perf_counter() - t0
                    frames[what], nbytes[what] = int(got[2].shape[0]), int(got[2].nbytes)
                    if i == 1 and a.host_records:  # the host half of the pair, once: on the first records, scaled
                        m = min(a.host_records, n_rec)
                        off = got[0][:m + 1]
                        t1 = time.perf_counter()
                        record_band_rows(off, got[1][:m], got[2][:off[-1]], rec["start"][:m], rec["end"][:m], NPERSEG, k)
                        host_ms[f"{k}_{w}"] = round((time.perf_counter() - t1) * 1e3 * n_rec / max(m, 1), 1)
                else:
                    got = b.fetch_record_spectrum(k, w)
                    dt = time.perf_counter() - t0
                    nbytes[what] = int(sum(np.asarray(x).nbytes for x in got))
                if i:  # (the first call allocates the pools and the tables)
                    s[what].append(dt * 1e3)
            got = None
        b.close()

        def stat(v):
            return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))

        line = {"metric": "record_spectrum_cost", "input": kind, "streams": a.streams, "samples_per_buffer": SAMPLES, "sample_rate": FS, "nperseg": NPERSEG,
                "margin": 0, "rounds": a.rounds, "records_per_call": n_rec, "frames": frames, "bytes": nbytes, "ms": {e: stat(v) for e, v in s.items()},
                "host_rows_ms_scaled": host_ms, "host_rows_records_timed": min(a.host_records, n_rec),
                "all_ms": {e: [round(x, 4) for x in v] for e, v in s.items()}}
        print(json.dumps(line), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")
        del iq
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
