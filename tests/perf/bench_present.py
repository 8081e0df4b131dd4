"""Cost of the presence mask (``rt_set_present``) -- not part of pytest, and apart from bench.py, whose runs never call the entry.
Config-2 geometry (2.048 MS/s, one second per buffer, nperseg 256) and the reference's defaults (300 kS/s, one second, nperseg
256), 4 096 streams each, bench.py's pipelined loop (two calls in flight), every variant timed ``--rounds`` times in alternation on
one box so that all see the same clocks; the spread of the rounds of one variant is the noise the comparisons are held against.

Case 1, the feature unused or idle: ``never`` (the entry is never called) against ``full`` (a mask with every stream present, set
through the native entry, so that the handle runs its per-stream path).  With ``--parent-tree DIR`` (a checkout of the parent
commit with its library built) ``never`` is also timed on that tree's package in a child process per round -- A / B pairs with
this tree's -- and the line reports both.

Case 2, time follows the present streams: ``half`` and ``seven_eighths`` of the streams present (every second / all but every
eighth; the absent rows are never read) against ``full`` on the same handle and against ``small_*``, a handle created with only
that many streams.

    python tests/perf/bench_present.py [--workloads config2 defaults] [--rounds 3] [--streams 4096] [--parent-tree DIR] [--out FILE]

Prints (and with --out appends, default profiles/present_bench.jsonl) one JSON line per case and workload."""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REPO = os.environ.get("RT_PRESENT_BENCH_TREE") or HERE  # (a child process of --parent-tree imports the package of that tree)
sys.path.insert(0, REPO)

WORKLOADS = {
    "config2": dict(sample_rate=2048000, samples=2048000, nperseg=256, window="hamming", steps=40, what="BASELINE config 2 geometry"),
    "defaults": dict(sample_rate=300000, samples=300000, nperseg=256, window="hamming", steps=40, what="the reference's defaults"),
}
VARIANTS = ("never", "full", "half", "seven_eighths", "small_half", "small_seven_eighths")


def mask_of(variant, n):
    import numpy as np

    if variant == "half":
        return np.arange(n) % 2 == 0
    if variant == "seven_eighths":
        return np.arange(n) % 8 != 7
    return np.ones(n, bool)


def timed(w, iq, variant, streams, settle=4):
    """(ms per step, records per step) of one variant on the input ``iq`` ([streams, samples] on the device)."""
    import torch

    from pyradiotracking_amd.analyze import BatchSignalAnalyzer, default_lanes

    n = streams
    if variant.startswith("small_"):
        n = int(mask_of(variant[len("small_"):], streams).sum())
    b = BatchSignalAnalyzer([str(i) for i in range(n)], sample_rate=w["sample_rate"], fft_nperseg=w["nperseg"], fft_window=w["window"],
                            sdr_callback_length=w["samples"], lanes=default_lanes(w["nperseg"], n))
    x = iq[:n]
    if variant in ("full", "half", "seven_eighths"):
        b.native.set_present(mask_of(variant, n))
    steps = w["steps"]

    def loop(k_steps):
        b.enqueue(x)
        n_rec = 0
        for k in range(k_steps):
            if k + 1 < k_steps:
                b.enqueue(x)  # two calls in flight
            n_rec += len(b.fetch_records())
        return n_rec

    loop(settle)  # (warm-up: code objects, AUTO's level, clocks)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n_rec = loop(steps)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    b.close()
    return dt / steps * 1e3, n_rec / steps


def make_input(w, streams):
    from oracle import analyze_oracle as oracle
    from pyradiotracking_amd import synth

    win = oracle.window_coefficients(w["window"], w["nperseg"])
    return synth.make_batch_device(streams, w["samples"], w["sample_rate"], win, seed=1)


def child(a):
    """One timing of ``never`` in a fresh process (the tree is chosen by RT_PRESENT_BENCH_TREE before the package is imported)."""
    w = WORKLOADS[a.workloads[0]]
    iq = make_input(w, a.streams)
    ms = [timed(w, iq, "never", a.streams)[0] for _ in range(a.rounds)]
    print(json.dumps({"ms": ms}))


def ab_parent(a, name):
    """A / B pairs of ``never``: this tree's library and the parent's, a child process each, alternating."""
    out = {"ours": [], "parent": []}
    for _ in range(a.rounds):
        for which, tree in (("ours", None), ("parent", a.parent_tree)):
            env = dict(os.environ)
            env.pop("RT_PRESENT_BENCH_TREE", None)
            if tree:
                env["RT_PRESENT_BENCH_TREE"] = os.path.abspath(tree)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--workloads", name, "--rounds", "2", "--streams", str(a.streams)],
                               env=env, capture_output=True, text=True, check=True)
            out[which].append(min(json.loads(r.stdout.strip().splitlines()[-1])["ms"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=list(WORKLOADS))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "present_bench.jsonl"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    import torch

    def emit(line):
        print(json.dumps(line), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")

    for name in a.workloads:
        w = WORKLOADS[name]
        if a.parent_tree:
            ab = ab_parent(a, name)
            emit({"metric": "present_unused_vs_parent", "workload": name, "what": w["what"], "streams": a.streams, "rounds": a.rounds,
                  "ms_per_step_ours": [round(v, 4) for v in ab["ours"]], "ms_per_step_parent": [round(v, 4) for v in ab["parent"]],
                  "best_ours_over_best_parent": round(min(ab["ours"]) / min(ab["parent"]), 4),
                  "spread_ours_pct": round(100.0 * (max(ab["ours"]) / min(ab["ours"]) - 1.0), 2),
                  "spread_parent_pct": round(100.0 * (max(ab["parent"]) / min(ab["parent"]) - 1.0), 2)})
        iq = make_input(w, a.streams)
        ms = {v: [] for v in VARIANTS}
        rec = {}
        for _ in range(a.rounds):
            for v in VARIANTS:
                t, r = timed(w, iq, v, a.streams)
                ms[v].append(t)
                rec[v] = r
        best = {v: min(ms[v]) for v in VARIANTS}
        spread = {v: round(100.0 * (max(ms[v]) / min(ms[v]) - 1.0), 2) for v in VARIANTS}
        emit({"metric": "present_idle_cost", "workload": name, "what": w["what"], "streams": a.streams, "samples": w["samples"], "steps": w["steps"],
              "rounds": a.rounds, "ms_per_step_never": round(best["never"], 4), "ms_per_step_full_mask": round(best["full"], 4),
              "full_over_never": round(best["full"] / best["never"], 4), "spread_pct": {v: spread[v] for v in ("never", "full")},
              "records_per_step": {v: rec[v] for v in ("never", "full")}})
        for part in ("half", "seven_eighths"):
            emit({"metric": "present_partial", "workload": name, "part": part, "present_streams": int(mask_of(part, a.streams).sum()), "streams": a.streams,
                  "rounds": a.rounds, "ms_per_step_masked": round(best[part], 4), "ms_per_step_all_present": round(best["full"], 4),
                  "ms_per_step_small_handle": round(best["small_" + part], 4), "masked_over_all_present": round(best[part] / best["full"], 4),
                  "masked_over_small_handle": round(best[part] / best["small_" + part], 4),
                  "spread_pct": {v: spread[v] for v in (part, "full", "small_" + part)}, "records_per_step": {v: rec[v] for v in (part, "small_" + part)}})
        del iq
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
