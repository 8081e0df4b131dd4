"""Throughput of the float64 path (precision="float64", rt_create_f64) from device complex128 tensors -- not part of pytest,
and apart from bench.py, which measures the float32 headline.

    python tests/perf/bench_float64.py [--streams 256] [--samples 2048000] [--nperseg 256 4096] [--steps 5] [--warmup 2]

Prints one JSON line per nperseg: MS/s, the bytes per sample the kernels move at least (16 B complex128 read, 8 B map write,
8 B map read by the row scan) and the share of the HBM roofline (6.3 TB/s) that is."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch  # noqa: E402

from pyradiotracking_amd.analyze import BatchSignalAnalyzer  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
BYTES_PER_SAMPLE = 16 + 8 + 8


def run(streams, samples, nperseg, steps, warmup):
    g = torch.Generator(device="cuda").manual_seed(nperseg)
    iq = torch.randn((streams, samples), dtype=torch.complex128, device="cuda", generator=g) * 1e-6  # noise far under -90 dBW
    b = BatchSignalAnalyzer([str(i) for i in range(streams)], precision="float64", sample_rate=2048000, fft_nperseg=nperseg,
                            sdr_callback_length=samples)
    for _ in range(warmup):
        b.enqueue(iq)
        b.fetch_records()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    b.enqueue(iq)
    n_rec = 0
    for k in range(steps):
        if k + 1 < steps:
            b.enqueue(iq)  # two calls in flight
        n_rec += len(b.fetch_records())
    dt = time.perf_counter() - t0
    b.close()
    ms = streams * samples * steps / dt / 1e6
    return {"metric": "float64_path_msamples_per_s", "nperseg": nperseg, "streams": streams, "samples": samples, "steps": steps,
            "msamples_per_s": round(ms, 1), "ms_per_call": round(dt / steps * 1e3, 3), "bytes_per_sample_min": BYTES_PER_SAMPLE,
            "hbm_roofline_fraction": round(ms * 1e6 * BYTES_PER_SAMPLE / HBM_BYTES_PER_S, 3), "records": n_rec}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--samples", type=int, default=2048000)
    ap.add_argument("--nperseg", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    for n in a.nperseg:
        print(json.dumps(run(a.streams, a.samples, n, a.steps, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
