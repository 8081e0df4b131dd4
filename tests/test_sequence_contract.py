"""The schedules of tests/sequence_cases.py on the CPU: the oracle runs every one of them, they reach back at every boundary and
differently at boundaries three apart, and -- the reason this file exists -- a model of the sparse look-back tail shows that they
see a tail writer that is subtly wrong, while the three equal calls of the older tests do not."""
import numpy as np
import pytest

from oracle import analyze_oracle as oracle
from tests import sequence_cases as sq
from tests import test_gpu_sequences as gs

CHUNK_LENGTHS = (4, 8, 32, 37, 71)


def test_oracle_runs_every_schedule_of_the_gpu_cases():
    """Every call of every parametrisation: no IndexError (the pinned ``times[-start]`` deviation must not arise), no call left out."""
    keys = gs.oracle_keys()
    assert len(keys) >= 25
    for name, nperseg, fmt, events, min_hops in keys:
        run = sq.oracle_run(name, nperseg, fmt, events, min_hops)
        sched = sq.SCHEDULES[name]
        assert len(run) == len(sched.T) and all(len(row) == sq.n_streams(nperseg) for row in run)
        assert sum(len(c.records) for row in run for c in row) > len(sched.T), (name, nperseg, fmt)


def _gate_cannot_open(sched, j, s, nperseg):
    """Every tone that reaches back over boundary j lights more than 1 / snr of its row in buffer j (short buffers): cell / row mean
    stays under the SNR threshold whatever the tone's level, so the reference finds nothing there."""
    snr = oracle.db_to_linear(sq.SNR_DB)
    T = sched.T[j]
    for i in range(len(sq.tone_bins(nperseg, s))):
        d, e = sq.reach(sched, j, s, i)
        if d and e:
            hot = np.zeros(T, bool)
            hot[:e] = True
            d_next, _ = sq.reach(sched, j + 1, s, i)
            if d_next:
                hot[T - d_next:] = True
            if hot.sum() * snr < T:
                return False
    return True


@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("nperseg", [256, 32, 4096])
def test_negative_starts_at_every_boundary(name, nperseg):
    """At every boundary whose two buffers have at least 3 segments every stream has a record with start < 0 -- unless the buffer is
    so short (schedule A's 9 segments) that every reaching tone fills over half its row and the 3 dB SNR gate cannot open."""
    sched = sq.SCHEDULES[name]
    run = sq.oracle_run(name, nperseg)
    excused = []
    for j in range(1, len(sched.T)):
        if sched.T[j - 1] < 3 or sched.T[j] < 3:
            continue
        for s in range(sq.n_streams(nperseg)):
            if any(r.start < 0 for r in run[j][s].records):
                continue
            assert _gate_cannot_open(sched, j, s, nperseg) and sched.T[j] < 16, (name, nperseg, j, s)
            excused.append((j, s))
    assert len(excused) <= 2, excused


@pytest.mark.parametrize("name", ["A", "B"])
def test_boundaries_three_apart_reach_back_differently(name):
    """Boundaries j and j - 3 share a tail buffer: for every j >= 4 and stream at least two tones have d(j) != d(j - 3), and over the
    schedule both signs occur for every stream -- a stale column of three calls ago is deeper here and shallower there."""
    sched = sq.SCHEDULES[name]
    for s in range(5):
        signs = set()
        for j in range(4, len(sched.T)):
            diff = [sq.reach(sched, j, s, i)[0] - sq.reach(sched, j - 3, s, i)[0] for i in range(6)]
            if min(sched.T[j - 1], sched.T[j], sched.T[j - 3], sched.T[j - 4]) >= 3:
                assert sum(1 for v in diff if v) >= 2, (name, s, j, diff)
            signs |= {int(np.sign(v)) for v in diff if v}
        assert signs == {-1, 1}, (name, s, signs)


def test_schedule_a_crosses_one_and_two_chunk_boundaries():
    """Negative starts of schedule A cross one chunk boundary of the previous call for every chunk length, and two of them for
    L = 4, 8 and 16.  With L = 32 a walk of at most 34 cells (D's deepest 33 and the cell it stops on) crosses two boundaries only
    from a previous call of exactly 65 segments (segment 64 down to 31), which the schedule does not hold: one crossing there."""
    run = sq.oracle_run("A", 256)
    sched = sq.SCHEDULES["A"]
    for L in (4, 8, 16, 32):
        crossed = set()
        for j in range(1, len(sched.T)):
            T_prev = sched.T[j - 1]
            for row in run[j]:
                for r in row.records:
                    if r.start < 0:
                        crossed.add((T_prev - 1) // L - (T_prev + r.start) // L)
        assert 1 in crossed and max(crossed) >= (2 if L < 32 else 1), (L, crossed)


def test_the_tone_after_the_empty_call_decides_differently_than_after_a_reset():
    """Schedule A, the call behind the empty one: the tone whose first hot segment is segment 1.  With an empty previous map the
    reference's walk may not go under ``lo_limit = 1 - 0`` and the record starts ON segment 1; after a reset it starts at 0."""
    sched = sq.SCHEDULES["A"]
    k = sq.empty_call(sched) + 1
    nperseg = 256
    x = sq.buffer(sched, nperseg, k)[0]
    _, times, spec = oracle.stft_power(x, sq.FS, sq.WINDOW, nperseg)
    params = sq.params_of(sq.settings(nperseg))
    b0, b1 = sq.extra_bins(nperseg, 0)
    after_empty = {r.fi: (r.start, r.end) for r in sq.extract(times, spec, spec[:, :0], params)}
    after_reset = {r.fi: (r.start, r.end) for r in sq.extract(times, spec, None, params)}
    assert after_empty[b1] == (1, 5) and after_reset[b1] == (0, 5)
    assert after_empty[b0] == after_reset[b0] == (0, 4)
    assert (b1, 1, 5) in sq.key(sq.oracle_run("A", nperseg)[k][0].records)


@pytest.mark.parametrize("nperseg", [8, 16, 32])
def test_under_64_bins_one_of_the_tones_takes_the_place_of_the_segment_1_tone(nperseg):
    sched = sq.SCHEDULES["A"]
    k = sq.empty_call(sched) + 1
    x = sq.buffer(sched, nperseg, k)[0]
    _, times, spec = oracle.stft_power(x, sq.FS, sq.WINDOW, nperseg)
    params = sq.params_of(sq.settings(nperseg))
    b = sq.tone_bins(nperseg, 0)[sq.shifted_tone(sched, k, 0, nperseg)]
    after_empty = {r.fi: (r.start, r.end) for r in sq.extract(times, spec, spec[:, :0], params)}
    after_reset = {r.fi: (r.start, r.end) for r in sq.extract(times, spec, None, params)}
    assert after_empty[b] == (1, 5) and after_reset[b] == (0, 5)


# ---- sharpness ---------------------------------------------------------------------------------------------------------------------
def _differing_calls(name, L, rule, n_calls=None, s=0):
    want = [sq.key(row[s].records) for row in sq.oracle_run(name, 256)]
    got = sq.tail_model_records(name, 256, s, L, rule, n_calls)
    return [k for k, g in enumerate(got) if g != want[k]]


@pytest.mark.parametrize("L", CHUNK_LENGTHS)
def test_the_tail_model_with_the_correct_rule_equals_the_oracle(L):
    assert _differing_calls("A", L, "correct") == [] and _differing_calls("B", L, "correct") == []


@pytest.mark.parametrize("L", CHUNK_LENGTHS)
def test_the_schedules_see_a_tail_that_drops_the_stopping_cell(L):
    a, b = _differing_calls("A", L, "drop_stop"), _differing_calls("B", L, "drop_stop")
    assert a and min(a) == 4, a   # the first call that reads a tail buffer written twice
    assert b == list(range(4, 10)), b  # equal lengths: every call from 4 on


@pytest.mark.parametrize("L", CHUNK_LENGTHS)
def test_schedule_a_sees_a_column_offset_that_ignores_short_calls(L):
    assert _differing_calls("A", L, "offset"), "varying lengths must show it"
    assert _differing_calls("B", L, "offset") == []  # (equal lengths cannot: T >= K throughout)


@pytest.mark.parametrize("rule", ["drop_stop", "offset"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_three_calls_are_blind_to_both_mutations(name, rule):
    """The shape of the older look-back tests: within three calls no tail is written twice, and what a wrong writer leaves out is
    still zero -- cold, like the cell that should be there."""
    for L in CHUNK_LENGTHS:
        assert _differing_calls(name, L, rule, n_calls=3) == []


# ---- schedule C ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nperseg", sorted(sq.C_SEEDS))
def test_schedule_c_seeds_decide_the_same_in_float32_and_float64(nperseg):
    """Under a noise floor thousands of cells lie near a threshold.  For the committed seeds the float32 oracle and its float64
    restatement find the same records on every call and stream, so a kernel whose round-off differs from SciPy's within the model
    still has to find exactly these.  (The seeds were searched here; no case is excluded at run time.)"""
    sched = sq.SCHEDULES["C"]
    S = sq.n_streams(nperseg)
    params = sq.params_of(sq.settings(nperseg, min_hops=sq.C_MIN_HOPS))
    want = sq.oracle_run("C", nperseg, "c64", (), sq.C_MIN_HOPS)
    last = [None] * S
    n_noisy = 0
    for k in range(len(sched.T)):
        # a call takes part if it or a neighbour carries noise (its own cells, its look-back, or the map it leaves behind); in the
        # quiet calls between, no cell but the tones' comes within 60 dB of a threshold
        if all(sq.call_sigma(sched, kk, s, 0.0) == sq.ssc.SIGMA_QUIET for s in range(S) for kk in (k - 1, k, k + 1) if 0 <= kk < len(sched.T)):
            last = [None] * S
            continue
        x = sq.buffer(sched, nperseg, k)
        for s in range(S):
            got, spec = sq.records_f64(x[s], nperseg, last[s], params)
            if last[s] is not None or k == 0:
                assert sq.key(got) == sq.key(want[k][s].records), (nperseg, k, s)
                n_noisy += len(got)
            last[s] = spec
    assert n_noisy > 50, n_noisy


def test_schedule_c_moves_through_the_noise_regimes():
    sched = sq.SCHEDULES["C"]
    sig = [sq.call_sigma(sched, k, 0, 0.0) for k in range(len(sched.T))]
    assert sig[:6] == [sq.ssc.SIGMA_QUIET] * 2 + [sq.SIGMA_FLOOR, sq.SIGMA_HIGH, sq.SIGMA_HIGH, sq.SIGMA_FLOOR] and set(sig[6:]) == {sq.ssc.SIGMA_QUIET}
    alone = [k for k in range(len(sched.T)) if sq.call_sigma(sched, k, 1, 0.0) != sig[k]]
    assert alone == [9, 10] and all(sq.call_sigma(sched, k, s, 0.0) == sig[k] for k in alone for s in (0, 2, 3, 4))
    run = sq.oracle_run("C", 256, "c64", (), sq.C_MIN_HOPS)
    for j in range(1, len(sched.T)):  # pulses cross every boundary
        assert all(any(r.start < 0 for r in run[j][s].records) for s in range(5)), j
