"""CPU side of the covering table (tests/combo_cases.py): without it tests/test_gpu_combos.py could pass on a table that covers
less than it says, on an oracle that finds nothing, or on decisions float32 cannot make.

* coverage: every pair of values of two axes, and every (size, format, sparse | dense) triple, that the constraints allow occurs in
  ``CASES`` -- recomputed here by brute force over all combinations, with the constraints restated, not from the generator;
* the oracle runs every case (no ``times[d + 1]`` IndexError of the reference), finds records in most calls, negative starts at a
  third of the boundaries, records across a gap under the presence table, different records under different settings;
* every decision is decidable: no cell of any oracle map within 2e-4 (relative) of a threshold on the float32 paths -- the margin
  tests/perf/soak_parity.py and DESIGN section 2 call undecidable in float32 --, within ``f64_sparse_cases.REL`` on the float64 ones;
* the contract oracle differs from every wrong model that applies to a case, and schedule P sees both mutations of the look-back
  tail from its fourth call on."""
import itertools

import pytest

from tests import combo_cases as cc
from tests import f64_sparse_cases as f64s
from tests import float64_cases as fc
from tests import present_cases as pc
from tests import sequence_cases as sq
from tests import test_gpu_combos as tgc

SCHED = sq.SCHEDULES[cc.SCHEDULE]
# the cases by what their oracle depends on, so that the maps of one (size, format) are made once (combo_cases.maps keeps two)
EVERY = cc.CASES + [cc.case_of(t) for t in tgc.REGRESSIONS]  # (the reduced cases of earlier findings run on the GPU as well)
KEYS = sorted({cc.oracle_key(c) for c in EVERY}, key=str)
CASE_OF = {k: next(c for c in EVERY if cc.oracle_key(c) == k) for k in KEYS}


def _ids(keys):
    return [f"{n}-{f}-{'gaps' if g else 'all'}-{s}" for n, f, g, s in keys]


# ---- coverage --------------------------------------------------------------------------------------------------------------------
def _allowed(c):
    """The refusals of rt_create / rt_create_f64, restated from the issue's list (combo_cases.valid is not used here)."""
    if c.size in (16, 300) and c.mode in ("sparse", "runfilter"):
        return False
    if c.size == 8192 and c.mode == "runfilter":
        return False
    if c.path in ("f64", "f64s"):
        if c.lanes > 1 or c.mode in ("sparse", "runfilter") or c.form == "group":
            return False
    if c.path == "f64s":
        if c.size in (16, 300, 8192) or c.side == "cells" or c.mode == "dense":
            return False
    if c.form == "group" and (c.size > 256 or c.size in (16, 300)):
        return False
    return True


def _goals(c):
    v = list(c._asdict().items())
    out = {(a, x, b, y) for (a, x), (b, y) in itertools.combinations(v, 2)}
    if c.path == "f32" and c.size in (64, 256, 512, 1024, 4096, 8192) and c.mode in ("sparse", "dense"):  # (the float32 scans')
        out.add(("triple", c.size, c.fmt, c.mode))
    return out


def test_every_allowed_pair_and_triple_occurs():
    allowed = set()
    for values in itertools.product(*cc.AXES.values()):
        c = cc.Case(*values)
        if _allowed(c):
            allowed |= _goals(c)
    have = set().union(*(_goals(c) for c in cc.CASES))
    missing = sorted(allowed - have, key=str)
    assert not missing, missing[:20]
    assert len([g for g in allowed if g[0] == "triple"]) == 48 and len(allowed) > 600, len(allowed)
    # the mirror: what a path allows occurs ON that path -- every size and every mode of it, and the float32 scans' dense and sparse
    # instantiations are launched by float32 handles
    for a, b in (("size", "path"), ("mode", "path"), ("fmt", "path")):
        want = {(getattr(c, a), c.path) for c in (cc.Case(*v) for v in itertools.product(*cc.AXES.values())) if _allowed(c)}
        assert want == {(getattr(c, a), c.path) for c in cc.CASES}, (a, b)
    f32 = {(c.size, c.fmt, c.mode) for c in cc.CASES if c.path == "f32"}
    assert all((n, f, m) in f32 for n in (64, 256, 512, 1024, 4096, 8192) for f in cc.AXES["fmt"] for m in ("sparse", "dense"))


def test_the_table_is_small_valid_and_readable():
    assert 40 <= len(cc.CASES) <= cc.MAX_CASES == 80
    assert all(_allowed(c) and cc.valid(c) for c in cc.CASES)
    ids = [cc.case_id(c) for c in cc.CASES]
    assert len(set(ids)) == len(ids)
    assert cc.case_id(cc.Case(256, "f32", "i8", "sparse", 3, True, "gaps", "perstream", "cells", 4, "default")) == \
        "256-f32-i8-sparse-l3-pipe-gaps-perstream-cells-c4-default"
    assert list(cc._generate()) == list(cc.CASES)  # deterministic


def test_schedule_p_keeps_its_properties():
    T, K = SCHED.T, sq.tail_cols(256)
    assert K == 42 and len(T) >= 8 and T.count(0) == 1 and max(T) <= 64
    assert any(0 < t < K / 4 for t in T) and 33 in T and sum(1 for t in T if 0 < t < K) >= 3
    t = pc.table("P")
    assert t.shape == (len(T), 5) and not t[pc.P_ALL_ABSENT_CALL].any() and t[:, 0].sum() == len(T) - 1
    assert sorted(b - a - 1 for a, b in pc.gaps(t, 2)) == [2, 3]
    # one of the two events falls on a call its stream sits out, the other on one it takes part in
    (_, k_snr, s_snr, _), (_, k_reset, s_reset) = cc.EVENTS
    assert not t[k_snr, s_snr] and t[k_reset, s_reset] and max(s_snr, s_reset) < sq.n_streams(8192)


# ---- the oracle is runnable and non-trivial --------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS, ids=_ids(KEYS))
def test_the_oracle_runs_finds_records_and_every_decision_is_decidable(key):
    size, fmt, gaps, settings = key
    c = CASE_OF[key]
    want = cc.oracle_run(c)  # (an IndexError here: adjust the presence table or the schedule, not the oracle)
    S = sq.n_streams(size)
    present = cc.presence_of(gaps, size)
    assert len(want) == len(SCHED.T) and all((want[k][s] is None) == (not present[k, s]) for k in range(len(want)) for s in range(S))
    calls_with = sum(1 for row in want if any(w is not None and w.records for w in row))
    assert calls_with > len(SCHED.T) // 2, calls_with
    # boundaries: a present (call, stream) pair with a previous map of at least one column
    last, n_bound, n_neg, n_gap = [None] * S, 0, 0, 0
    for k, row in enumerate(want):
        for s, w in enumerate(row):
            if w is None:
                continue
            if last[s] is not None and SCHED.T[last[s]] > 0 and SCHED.T[k] > 0:
                n_bound += 1
                neg = any(r.start < 0 for r in w.records)
                n_neg += neg
                n_gap += neg and k - last[s] > 1
            last[s] = k
    assert 3 * n_neg >= n_bound > 0, (n_neg, n_bound)
    if gaps:
        assert n_gap >= 1, "no record across a gap"
    if settings != "uniform":
        sets = [tuple(tuple(sq.key(want[k][s].records)) if want[k][s] is not None else None for k in range(len(want))) for s in range(S)]
        assert any(len({sets[a], sets[b], sets[d]}) == 3 for a, b, d in itertools.combinations(range(S), 3)), "settings do not separate three streams"
    # every map a stream analyses, against that stream's own thresholds (the event's new SNR threshold included): margin_ok on the
    # rows that hold a cell not clearly under the absolute threshold.  The other rows are clear of it by that, and their cells'
    # SNR figures decide nothing (analyze.py:370 fails first) -- among the 2 M noise cells of a case some hundred lie within 2e-4 of
    # 3 dB over their row's mean by chance, whatever the settings.  The look-back cells get the same check against the row means
    # they are compared with.
    rel = 2e-4 if fmt not in sq.F64_FORMATS else f64s.REL
    every = cc.maps(size, fmt)
    before = [None] * S  # each stream's previous present map (a reset only takes look-backs away)
    for s in range(S):
        p = sq.params_of(cc.stream_kwargs(size, fmt, settings, s))
        changed = [(ev[1], sq.params_of(dict(snr_threshold_db=ev[3])).snr_threshold) for ev in cc.events_of(settings) if ev[0] == "snr" and ev[2] == s]
        for k in range(len(SCHED.T)):
            if SCHED.T[k] and present[k, s]:
                spec = every[k][s][2]
                rows = ~(spec < p.signal_threshold * (1.0 - rel)).all(axis=1)
                for snr in [v for k0, v in changed if k >= k0][-1:] or [p.snr_threshold]:
                    assert fc.margin_ok(spec[rows], p.signal_threshold, snr, rel=rel), (key, k, s, "a cell within", rel, "of a threshold")
                    # the walk's look-back compares the cells of the stream's PREVIOUS map with THIS map's row means (analyze.py:
                    # 382-398): the same margin for them, on the rows either map holds a cell near the threshold in
                    # (the trailing cells a walk can reach: one deeper than the stream's maximum duration fails the duration gate
                    # whatever cell it stops on)
                    if before[s] is not None and before[s].shape[1]:
                        tail = before[s][:, -(int(p.signal_max_duration / sq.hop_s(size)) + 2):]
                        both = rows | ~(tail < p.signal_threshold * (1.0 - rel)).all(axis=1)
                        ratio = tail[both].astype("f8") / spec[both].astype("f8").mean(axis=1, keepdims=True) / snr
                        near = (abs(ratio - 1.0) < rel) & ~(tail[both] < p.signal_threshold * (1.0 - rel))  # (a cell clearly under the absolute threshold is cold whatever its ratio)
                        assert not near.any(), (key, k, s, "a look-back cell within", rel, "of the SNR threshold")
                before[s] = spec


# ---- discriminating power --------------------------------------------------------------------------------------------------------
def _differs(c, model):
    want, wrong = cc.oracle_run(c), cc.oracle_run(c, model)
    return [(k, s) for k in range(len(want)) for s in range(len(want[k]))
            if want[k][s] is not None and sq.key(want[k][s].records) != sq.key(wrong[k][s].records)]


@pytest.mark.parametrize("key", KEYS, ids=_ids(KEYS))
def test_every_wrong_model_that_applies_differs_from_the_contract(key):
    size, fmt, gaps, settings = key
    c = CASE_OF[key]
    if gaps:
        for model in ("zeros_reset", "lockstep"):
            assert _differs(c, model), model
    if settings != "uniform":
        assert _differs(c, "envelope"), "envelope"
    if settings == "events":
        d = _differs(c, "no_restart")
        assert d and {s for _, s in d} == {cc.EVENTS[0][2]}, d


@pytest.mark.parametrize("size", [n for n in cc.AXES["size"] if n in cc.TRIPLE_SIZES])
def test_schedule_p_sees_both_mutations_of_the_tail_from_the_fourth_call_on(size):
    """Stream 0, chunks of 4, 16 and 32: the correct rule equals the oracle (``sequence_cases.oracle_run``, whose settings the tail
    model takes), ``drop_stop`` and ``offset`` differ from it within the schedule's calls and not within its first three."""
    c = cc.Case(size, "f32", "cx", "sparse", 1, False, "all", "uniform", "none", 0, "default")
    plain = sq.oracle_run(cc.SCHEDULE, size)
    want = [sq.key(row[0].records) for row in plain]
    for L in (4, 16, 32):
        assert sq.tail_model_records(cc.SCHEDULE, size, 0, L, "correct") == want, L
        for rule in ("drop_stop", "offset"):
            got = sq.tail_model_records(cc.SCHEDULE, size, 0, L, rule)
            bad = [k for k in range(len(want)) if got[k] != want[k]]
            assert bad and min(bad) >= 3, (L, rule, bad)
            assert sq.tail_model_records(cc.SCHEDULE, size, 0, L, rule, n_calls=3) == want[:3], (L, rule)
    if size == 256:  # through oracle_run, every stream
        for rule in ("drop_stop", "offset"):
            wrong = cc.oracle_run(c, rule)
            # (None: a misplaced column sends that stream's walk past a short call's time axis and the reference raises)
            ran = [s for s in range(sq.n_streams(size)) if wrong[0][s] is not None]
            assert 0 in ran, (rule, ran)
            assert all(any(wrong[k][s] != sq.key(plain[k][s].records) for k in range(len(want))) for s in ran), rule
