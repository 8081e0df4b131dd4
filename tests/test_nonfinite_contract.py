"""The NaN / Inf cases of tests/nonfinite_cases.py on the CPU: the oracle equals what the reference made of them
(tests/golden/nonfinite_cases.npz, written by tests/golden/make_golden_nonfinite.py), and every case is shown to do what it claims --
otherwise tests/test_gpu_nonfinite.py could pass vacuously."""
import datetime

import numpy as np
import pytest

from oracle import analyze_oracle as oracle
from tests import golden_util as gu
from tests import nonfinite_cases as nf
from tests import sequence_cases as sq

GOLDEN = nf.golden_cases()


def _fixture():
    return gu._npz("nonfinite_cases.npz")


def test_the_fixture_holds_exactly_the_golden_cases():
    z = _fixture()
    assert [str(n) for n in z["names"]] == [nf.case_id(c) for c in GOLDEN]
    assert len(GOLDEN) >= 60 and {c.kind for c in GOLDEN} == set(nf.KINDS) and {c.fmt for c in GOLDEN} == {"c64", "c128"}


@pytest.mark.parametrize("case", GOLDEN, ids=nf.case_id)
def test_oracle_equals_the_reference(case):
    """Tables (NaN equal to NaN), shadow verdicts and the spectrograms' digests of the poisoned stream's three buffers."""
    z = _fixture()
    pre = nf.case_id(case)
    bufs = [b[nf.POISONED] for b in nf.buffers(case)]
    rows = z[pre]
    sha = [str(v) for v in z["sha256"][[str(n) for n in z["names"]].index(pre)]]
    assert gu.iq_sha256(bufs) == sha[0], "regenerated IQ differs from the bytes the reference saw"
    oa = oracle.OracleAnalyzer(device="0", **nf.settings(case.nperseg, case.hops))
    with np.errstate(all="ignore"):
        for k, buf in enumerate(bufs):
            ts = gu.TS0 + datetime.timedelta(seconds=k * len(buf) / nf.FS)
            every, kept = oa.process(buf, ts)
            tab = gu.signals_table(every, ts.replace(tzinfo=datetime.timezone.utc))
            mine = rows[rows[:, 0] == k]
            assert np.array_equal(tab, mine[:, 1:9], equal_nan=True), f"buffer {k}"
            kept_ids = {id(s) for s in kept}
            assert [id(s) in kept_ids for s in every] == [bool(v) for v in mine[:, 9]], f"buffer {k}"
            assert nf.spec_digest(oa.spec_last) == sha[1 + k], f"buffer {k}"
            # every kind gives an all-NaN column (the digest holds the NaN mask: the reference's map has it too) and no other NaN cell
            nan = np.isnan(oa.spec_last)
            p = nf.segment_of(case.pos)
            want = np.zeros_like(nan)
            if k == 0 and p is not None:
                want[:, p] = True
            assert np.array_equal(nan, want), f"buffer {k}: NaN cells {np.argwhere(nan != want)[:5]}"


def _cases_run_on_the_gpu():
    from tests import test_gpu_nonfinite as gn

    return gn.oracle_cases()


def _finite_overlapping(call, spec_prev, p):
    """(shadowed, not shadowed) counts among the records without a NaN cell that overlap the column in time: [start, end] holds
    p - 1 or p + 1 (a record's ``end`` is the cold cell it stops on, its ``start`` the cold cell before it)."""
    n = [0, 0]
    for r, sh in zip(call.records, call.shadowed):
        if not nf.has_nan_cells(r, call.spec, spec_prev) and r.start <= p + 1 and r.end >= p - 1:
            n[0 if sh else 1] += 1
    return n


def test_every_case_does_what_it_claims():
    """On the oracle, for every case the GPU tests run up to nperseg 4096 -- the size whose 1-hop cases hold thousands of NaN records
    for the tiled shadow ranking and the record growth -- (8192 and 16384 repeat the layout with more quiet bins):
    * stream 2's call 0 has the NaN column and a NaN row mean in every bin; no other stream or call has a NaN;
    * at least one record with NaN statistics per case (none at all for the ragged-tail position, which equals the clean batch);
    * positions 0, 7, 8: at least one finite record shadowed and one not shadowed among those that overlap the column in time;
      with the 1-hop setting exactly one NaN record in every bin that holds no tone, the two-cell one;
    * position T - 1: the column's plateaus lap into the next buffer (analyze.py:415), so call 0 reports no NaN record, and
      call 1 holds records with a negative start that walked through the NaN tail column, shadowed and unshadowed finite records
      beside them.  (For the other positions call 1 cannot reach the column: the maximum duration is 40 hops.)"""
    cases = [c for c in _cases_run_on_the_gpu() if c.nperseg <= 4096]
    assert len(cases) > 80 and any(c.layout == "long" for c in cases) and any(c.nperseg == 4096 and c.hops == 1.0 for c in cases)
    for case in cases:
        what = nf.case_id(case)
        p = nf.segment_of(case.pos)
        with np.errstate(all="ignore"):
            run = nf.oracle_case(case)
        for s, calls in enumerate(run):
            for k, c in enumerate(calls):
                nan = np.isnan(c.spec)
                if s == nf.POISONED and k == 0 and p is not None:
                    assert nan[:, p].all() and nan.sum() == case.nperseg, what
                else:
                    assert not nan.any(), (what, s, k)
        calls = run[nf.POISONED]
        prev = [None, calls[0].spec, calls[1].spec]
        n_nan = [sum(nf.has_nan_cells(r, c.spec, prev[k]) for r in c.records) for k, c in enumerate(calls)]
        for k, c in enumerate(calls):  # a record's statistics are NaN exactly when one of its cells is
            for r in c.records:
                assert np.isnan(r.max_dbw) == np.isnan(r.avg_dbw) == np.isnan(r.std_db) == nf.has_nan_cells(r, c.spec, prev[k]), (what, k, r)
                assert np.isnan(r.noise_dbw) == (k == 0 and p is not None), (what, k, r)
        if p is None:
            clean = nf.oracle_clean(case.nperseg, nf.layout_segment(case.pos), case.hops, case.fmt, case.layout)[nf.POISONED]
            assert n_nan == [0, 0, 0] and all(sq.key(a.records) == sq.key(b.records) for a, b in zip(calls, clean)), what
            continue
        assert sum(n_nan) >= 1 and n_nan[2] == 0, (what, n_nan)
        if p == nf.T - 1:
            assert n_nan[0] == 0 and n_nan[1] >= 2, (what, n_nan)
            walked = [r for r in calls[1].records if r.start < 0 and nf.has_nan_cells(r, calls[1].spec, calls[0].spec)]
            assert len(walked) >= 2 and all(r.start < -1 for r in walked), what
        else:
            assert n_nan[0] >= 3 and n_nan[1] == 0, (what, n_nan)
            assert any(r.start < 0 for r in calls[1].records), what
        shadowed, free = _finite_overlapping(calls[0], None, p)
        assert shadowed >= 1 and free >= 1, (what, shadowed, free)
        if case.hops == 1.0 and p != nf.T - 1:
            quiet = nf.quiet_bins(case)
            assert len(quiet) >= (1 if case.nperseg == 16 else case.nperseg // 3), (what, len(quiet))
            want = (max(p - 1, 0), p + 1)
            for fi in quiet:
                got = [(r.start, r.end) for r in calls[0].records if r.fi == fi]
                assert got == [want], (what, fi, got)


def test_the_fast_shadow_verdicts_equal_the_oracles_loop():
    """``nonfinite_cases.shadow_flags`` against ``oracle.shadow_index`` over the unfiltered list, NaN records included."""
    n = 0
    for case in (nf.Case(256, "nan", "seg7", "first", 1.0), nf.Case(32, "+inf_re", "last", "first", 1.0), nf.Case(300, "-inf_im", "seg8", "last", 4.0, "c128")):
        with np.errstate(all="ignore"):
            for calls in nf.oracle_case(case):
                for c in calls:
                    assert c.shadowed == sq.shadow_flags(c.records, c.freqs)
                    n += sum(c.shadowed)
    assert n > 20


@pytest.mark.parametrize("case", [nf.Case(256, "nan", "seg7", "first", 1.0), nf.Case(256, "+inf_re", "seg8", "last", 4.0),
                                  nf.Case(32, "nan_im", "last", "first", 1.0), nf.Case(300, "-inf_im", "last", "last", 4.0),
                                  nf.Case(256, "nan", "seg0", "last", 4.0)], ids=nf.case_id)
def test_an_extraction_with_greater_equal_tests_is_seen(case):
    """``cell >= thr`` instead of ``not cell < thr`` (a kernel that lost one ``!(p < t)``): the records of the poisoned call -- and, for
    the last segment, of the call that reaches back into it -- differ from the reference's."""
    xs = [b[nf.POISONED] for b in nf.buffers(case)]
    with np.errstate(all="ignore"):
        want = nf.oracle_stream(xs, case.nperseg, case.hops)
        got = nf.oracle_stream(xs, case.nperseg, case.hops, compare=">=")
    k = 1 if case.pos == "last" else 0
    assert sq.key(got[k].records) != sq.key(want[k].records)
    assert sq.key(got[2].records) == sq.key(want[2].records)


def test_the_planted_maps_hold_what_they_claim():
    for dt in (np.float32, np.float64):
        cur, last = nf.planted_maps(dt)
        assert np.isnan(cur).sum() == 2 and np.isnan(last).sum() == 1
        with np.errstate(all="ignore"):
            run = nf.planted_oracle(cur, last)
        k0 = {(r.fi, r.start, r.end): r for r in run[0].records}
        assert set(k0) == {(3, 9, 18), (7, 24, 26), (11, 9, 16)}, sorted(k0)
        assert np.isnan(k0[(3, 9, 18)].max_dbw) and np.isnan(k0[(7, 24, 26)].max_dbw) and np.isfinite(k0[(11, 9, 16)].max_dbw)
        assert np.isnan(k0[(3, 9, 18)].noise_dbw) and np.isfinite(k0[(11, 9, 16)].noise_dbw)  # one cell, not a column: only that bin's mean
        k1 = {(r.fi, r.start, r.end): r for r in run[1].records}
        assert set(k1) == {(5, -4, 4), (9, 19, 27)}, sorted(k1)
        assert np.isnan(k1[(5, -4, 4)].max_dbw) and np.isfinite(k1[(5, -4, 4)].noise_dbw) and np.isfinite(k1[(9, 19, 27)].std_db)
