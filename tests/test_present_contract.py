"""CPU side of the presence tests (``rt_set_present``): without it tests/test_gpu_present.py could pass on nothing.

* the gapped oracle of tests/present_cases.py raises nothing on any pattern the GPU cases run -- in particular not the reference's
  ``times[d + 1]`` IndexError (the presence tables are made so; the oracle is never bent);
* every pattern holds reach-back records across a gap of one, of two and of three or more absent calls, per nperseg the GPU runs;
* the gapped oracle differs from both wrong models of an absent stream ("zeros + reset", "the batch's previous call");
* the host-only bookkeeping (rt_core.h: PresenceBook, through _rt_hostcheck.so) equals a plain NumPy model over the patterns and
  over a randomised 200-call schedule with resets, rollbacks and mask changes, and keeps every stream's look-back columns within
  reach of the rotation of three tail buffers;
* the entry point's refusals that need no device, the binding, and ``BatchRunner(skip_absent=True)`` on a fake analyzer."""
import ctypes as C

import numpy as np
import pytest

from pyradiotracking_amd import _native, build
from tests import present_cases as pc
from tests import sequence_cases as sq
from tests import test_gpu_present as tgp

KEYS = tgp.oracle_keys()


@pytest.mark.parametrize("name,nperseg,fmt,events,min_hops", KEYS, ids=[f"{a}-{n}-{f}{'-events' if e else ''}" for a, n, f, e, _ in KEYS])
def test_gapped_oracle_raises_nothing_and_reaches_back_across_every_gap_length(name, nperseg, fmt, events, min_hops):
    want = pc.oracle_run(name, nperseg, fmt, events, min_hops)  # (an IndexError here: adjust the presence table, not the oracle)
    S = sq.n_streams(nperseg)
    present = pc.table(name, S)
    assert len(want) == present.shape[0]
    assert all((want[k][s] is None) == (not present[k, s]) for k in range(len(want)) for s in range(S))
    if events:
        return
    by_gap = pc.gap_records(name, nperseg, fmt, min_hops)
    n1, n2, n3 = len(by_gap.get(1, [])), len(by_gap.get(2, [])), sum(len(v) for g, v in by_gap.items() if g >= 3)
    assert n1 >= 3 and n2 >= 3 and n3 >= 3, (n1, n2, n3)
    # such a record is ONE plateau of d + e cells: the tail of the stream's last present buffer and the head of this one
    sched = sq.SCHEDULES[name]
    for g, recs in by_gap.items():
        for b, s, r in recs:
            assert r.start < 0 < r.end and r.end - r.start >= 2, (g, b, s, r)


def test_tables_hold_the_patterns():
    t = pc.table("A")
    assert t.shape == (13, 5) and t[:, 0].sum() == 12 and not t[pc.ALL_ABSENT_CALL].any()
    assert [len(g) for g in (pc.gaps(t, s) for s in range(5))] == [1, 4, 3, 1, 4]
    assert sorted(b - a - 1 for a, b in pc.gaps(t, 2)) == [2, 3, 3]
    assert not t[0, 3] and not t[9, 3] and not t[10, 3] and sq.A_T[9] == 0
    assert all(not t[k, 4] for k in range(13) if (k + 1) % 3 == 0)
    c = pc.table("C")
    assert not c[2:6, 1].any() and sorted(b - a - 1 for a, b in pc.gaps(c, 2)) == [1, 2, 3, 4]


WRONG = [(a, n, f, h) for a, n, f, e, h in KEYS if not e]


@pytest.mark.parametrize("name,nperseg,fmt,min_hops", WRONG, ids=[f"{a}-{n}-{f}" for a, n, f, _ in WRONG])
@pytest.mark.parametrize("model", ["zeros_reset", "lockstep"])
def test_wrong_models_of_an_absent_stream_fail(name, nperseg, fmt, min_hops, model):
    """Both models lose (or bend) the reach-back across a gap; neither touches a stream that is always present."""
    want = pc.oracle_run(name, nperseg, fmt, (), min_hops)
    wrong = pc.oracle_run(name, nperseg, fmt, (), min_hops, None, model)
    S = sq.n_streams(nperseg)
    differs = [(k, s) for k in range(len(want)) for s in range(S)
               if want[k][s] is not None and sq.key(want[k][s].records) != sq.key(wrong[k][s].records)]
    assert len(differs) >= 3, differs
    present = pc.table(name, S)
    for k, s in differs:  # ... and only in the first present call behind a gap
        assert k > 0 and not present[k - 1, s], (k, s)


# ---- the host-only bookkeeping ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hc():
    lib = C.CDLL(build.build_hostcheck())
    vp = C.c_void_p
    lib.hc_presence_new.argtypes = [C.c_int, C.c_int]
    lib.hc_presence_new.restype = vp
    lib.hc_presence_free.argtypes = [vp]
    lib.hc_presence_free.restype = None
    lib.hc_presence_set.argtypes = [vp, vp]
    lib.hc_presence_reset_stream.argtypes = [vp, C.c_int]
    lib.hc_presence_reset_stream.restype = None
    lib.hc_presence_reset_all.argtypes = [vp]
    lib.hc_presence_reset_all.restype = None
    lib.hc_presence_call.argtypes = [vp, C.c_int, vp, vp, vp]
    lib.hc_presence_snapshot.argtypes = [vp, C.c_ulonglong, vp, vp, vp]
    lib.hc_presence_rollback.argtypes = [vp]
    lib.hc_presence_rollback.restype = None
    lib.hc_presence_state.argtypes = [vp, vp, vp, vp]
    lib.hc_presence_state.restype = None
    return lib


class Model:
    """The contract in plain NumPy: per stream the segment count of its own last present buffer, its pending reset -- and three
    tail buffers, each holding per stream the number of the call whose columns it holds (-1: none), written by a present stream,
    carried from the buffer read to the buffer written for an absent one."""

    def __init__(self, S, all_=-1):
        self.S = S
        self.present = np.ones(S, bool)
        self.nsl = np.full(S, all_, np.int32)
        self.reset = np.zeros(S, bool)
        self.cur = 0
        self.n_calls = 0
        self.tails = np.full((3, S), -1, np.int64)
        self.last_call = np.full(S, -1, np.int64)  # the call of each stream's own last present buffer
        self.undo = None

    def call(self, T):
        self.undo = (self.nsl.copy(), self.reset.copy(), self.cur, self.tails.copy(), self.last_call.copy())
        rd, wr = self.cur, (self.cur + 1) % 3
        absent = ~self.present
        seen = np.where(absent, self.nsl, np.where(self.reset, -1, self.nsl)).astype(np.int32)
        # what the call reads as "previous buffer" of a present stream is the stream's own last present buffer
        for s in np.flatnonzero(self.present):
            assert self.tails[rd, s] == self.last_call[s], (self.n_calls, s, self.tails[:, s], self.last_call[s])
        self.tails[wr] = np.where(absent, self.tails[rd], self.n_calls)
        self.last_call = np.where(absent, self.last_call, self.n_calls)
        self.reset &= absent
        self.nsl = np.where(absent, self.nsl, T).astype(np.int32)
        self.cur = wr
        self.n_calls += 1
        return absent.astype(np.uint8), seen, (rd, wr), int(self.present.sum())

    def rollback(self):
        took = self.undo[1] & ~self.reset
        self.nsl, _, self.cur, self.tails, self.last_call = self.undo
        self.reset = self.reset | took
        self.n_calls -= 1


def _call(hc, h, S, T):
    absent, nsl, tails = np.zeros(S, np.uint8), np.zeros(S, np.int32), np.zeros(2, np.int32)
    n = hc.hc_presence_call(h, T, absent.ctypes.data, nsl.ctypes.data, tails.ctypes.data)
    return absent, nsl, tuple(int(x) for x in tails), n


def _state(hc, h, S):
    nsl, rp, pr = np.zeros(S, np.int32), np.zeros(S, np.uint8), np.zeros(S, np.uint8)
    hc.hc_presence_state(h, nsl.ctypes.data, rp.ctypes.data, pr.ctypes.data)
    return nsl, rp.astype(bool), pr.astype(bool)


def _same(got, want):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2] and got[3] == want[3], (got, want)


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_bookkeeping_equals_the_model_over_the_patterns(hc, name):
    """Every call's snapshot -- who is absent, each stream's own previous segment count, the tail buffers read and written -- and
    after the last call the book's state; resets issued while their stream is absent (the events of the GPU case) stay pending
    until its next present call.  The model itself asserts that a present stream always finds its own last present buffer in the
    tail buffer its call reads, after any number of absent calls."""
    sched = sq.SCHEDULES[name]
    present = pc.table(name)
    S = present.shape[1]
    h = hc.hc_presence_new(S, -1)
    m = Model(S)
    try:
        for k, T in enumerate(sched.T):
            if name == "A" and k in (5, 7):
                s = {5: 1, 7: 2}[k]
                assert not present[k, s]
                hc.hc_presence_reset_stream(h, s)
                m.reset[s] = True
            mask = np.ascontiguousarray(present[k], np.uint8)
            changed = hc.hc_presence_set(h, mask.ctypes.data)
            assert bool(changed) == bool((m.present != present[k]).any())
            m.present = present[k].copy()
            got, want = _call(hc, h, S, T), m.call(T)
            _same(got, want)
            if name == "A" and k in (5, 7):
                assert _state(hc, h, S)[1][s]  # still pending: the stream sat the call out
            if name == "A" and k in (6, 8):
                s = {6: 1, 8: 2}[k]
                assert got[1][s] == -1 and not _state(hc, h, S)[1][s]  # taken at its next present call: no previous buffer
            # the snapshot of this call and of the one before stay readable (two call slots): what a re-analysis in rt_fetch uses
            a2, n2, t2 = np.zeros(S, np.uint8), np.zeros(S, np.int32), np.zeros(2, np.int32)
            assert hc.hc_presence_snapshot(h, k, a2.ctypes.data, n2.ctypes.data, t2.ctypes.data) == want[3]
            assert np.array_equal(a2, want[0]) and np.array_equal(n2, want[1])
        nsl, rp, pr = _state(hc, h, S)
        assert np.array_equal(nsl, m.nsl) and np.array_equal(rp, m.reset) and np.array_equal(pr, m.present)
    finally:
        hc.hc_presence_free(h)


def test_bookkeeping_equals_the_model_over_200_random_calls(hc):
    """Random masks (NULL = every stream among them), segment counts (0 and short ones included), stream resets, whole resets
    and rollbacks of the newest call, and a handle that had made calls before the entry was first used (``all`` = 57)."""
    rng = np.random.default_rng(20240611)
    S = 11
    h = hc.hc_presence_new(S, 57)
    m = Model(S, 57)
    m.tails[0] = -2  # (the buffer the first call reads holds every stream's latest buffer: call "-2")
    m.last_call[:] = -2
    prev_snapshot = None
    try:
        for k in range(200):
            r = rng.random()
            if r < 0.15:
                hc.hc_presence_set(h, None)
                m.present = np.ones(S, bool)
            elif r < 0.8:
                mask = rng.random(S) < rng.choice([0.1, 0.5, 0.9])
                hc.hc_presence_set(h, np.ascontiguousarray(mask, np.uint8).ctypes.data)
                m.present = mask
            for s in np.flatnonzero(rng.random(S) < 0.05):
                hc.hc_presence_reset_stream(h, int(s))
                m.reset[s] = True
            if rng.random() < 0.02:
                hc.hc_presence_reset_all(h)
                m.nsl[:] = -1
                m.reset[:] = False
                m.tails[:] = -1  # (no stream has a previous buffer: whatever the tails hold is never read)
                m.last_call[:] = -1
            T = int(rng.choice([0, 2, 9, 33, 64, 96, 1171]))
            got, want = _call(hc, h, S, T), m.call(T)
            _same(got, want)
            if rng.random() < 0.1:
                # the newest call is undone (a later lane failed to enqueue): counts, resets and rotation as before it
                hc.hc_presence_rollback(h)
                m.rollback()
                if prev_snapshot is not None and m.n_calls >= 1:
                    a2, n2, t2 = np.zeros(S, np.uint8), np.zeros(S, np.int32), np.zeros(2, np.int32)
                    assert hc.hc_presence_snapshot(h, m.n_calls - 1, a2.ctypes.data, n2.ctypes.data, t2.ctypes.data) >= 0
                    assert np.array_equal(a2, prev_snapshot[0]) and np.array_equal(n2, prev_snapshot[1])
            else:
                prev_snapshot = want
            nsl, rp, pr = _state(hc, h, S)
            assert np.array_equal(nsl, m.nsl) and np.array_equal(rp, m.reset) and np.array_equal(pr, m.present), k
    finally:
        hc.hc_presence_free(h)


# ---- the entry point -------------------------------------------------------------------------------------------------------------
def test_entry_point_refusals_that_need_no_device():
    lib = _native.load_library()
    assert "rt_set_present" in _native.ABI_SYMBOLS
    assert lib.rt_set_present(None, None) == _native.RT_E_INVALID
    mask = np.ones(4, np.uint8)
    assert lib.rt_set_present(None, mask.ctypes.data) == _native.RT_E_INVALID


def test_header_declares_the_entry_and_its_contract():
    import os

    text = open(os.path.join(build.REPO, "include", "rt_analyze.h")).read()
    assert "int rt_set_present(rt_handle *h, const uint8_t *present);" in text
    for phrase in ("no effect from its row", "state as if no call happened", "deferred changes", "whole-call errors stay"):
        assert phrase in text, phrase
    assert "#define RT_ABI_VERSION 6" in text


# ---- BatchRunner(skip_absent=True) on a fake analyzer ------------------------------------------------------------------------------
class _Fake:
    def __init__(self, devices, calibration_db=None, gpu=0, **kw):
        self.devices = list(devices)
        self.masks, self.resets, self.chunks = [], [], []
        self.decoder = self
        self.precision = "float32"

    def set_present(self, mask):
        self.masks.append(list(mask))

    def reset_stream(self, s):
        self.resets.append(s)

    def enqueue(self, chunk):
        self.chunks.append(np.array(chunk))

    def fetch_records(self, allow_truncated=False):
        return np.zeros(0, dtype=_native.RECORD_DTYPE)

    def signals(self, rec, names, starts):
        return []

    def close(self):
        pass


def _fake_runner(**kw):
    from pyradiotracking_amd.runner import BatchRunner

    made = []

    def factory(devices, **k):
        made.append(_Fake(devices, **k))
        return made[-1]

    r = BatchRunner(device=list("abc"), gpus=(0,), sdr_timeout_s=100, analyzer_factory=factory, sample_rate=1000, **kw)
    r.start_analyzers()
    return r, made[0]


def test_runner_skip_absent_sets_the_mask_instead_of_zero_filling_and_resetting():
    r, fake = _fake_runner(skip_absent=True)
    buf = np.ones((3, 1000), np.complex64)
    t0 = 1700000000.0
    r.process(buf, now=t0)
    r.process(buf, present=[True, False, True], now=t0 + 1)
    r.process(buf, present=[True, False, True], now=t0 + 2)
    r.process(buf, now=t0 + 3)
    assert fake.masks == [[True, True, True], [True, False, True], [True, False, True], [True, True, True]]
    assert fake.resets == [] and not any(st.stale for st in r.streams)
    assert all((c == 1).all() for c in fake.chunks)  # the absent row is handed on as it is: the handle does not read it
    # only the present streams' clocks moved: b is two buffers behind a and c
    assert r.streams[0].ts - r.streams[1].ts == __import__("datetime").timedelta(seconds=2)
    # a restarted stream still starts without look-back
    r.restart_stream(r.streams[1])
    assert fake.resets == [1]


def test_runner_default_is_unchanged():
    r, fake = _fake_runner()
    buf = np.ones((3, 1000), np.complex64)
    t0 = 1700000000.0
    r.process(buf, now=t0)
    r.process(buf, present=[True, False, True], now=t0 + 1)
    r.process(buf, now=t0 + 2)
    assert fake.masks == [] and fake.resets == [1]
    assert (fake.chunks[1][1] == 0).all() and (fake.chunks[1][0] == 1).all()
