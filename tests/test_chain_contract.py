"""CPU side of the chain tests (``rt_set_chain``): without it tests/test_gpu_chain.py could pass on nothing.

* the host-only book (rt_core.h: ChainBook on a PresenceBook, through _rt_hostcheck.so) equals the NumPy model of
  tests/chain_cases.py -- "a run is one reference analyzer; its buffers of a call are the present links in index order" -- over the
  presence tables of tests/present_cases.py re-read as runs, links 2, 3 and 4, and over 200 random calls with random masks, resets,
  rollbacks and T; the model asserts that every present stream's source holds the columns of its predecessor buffer, and runs that
  sit out 1 ... 4 calls find their last present stream afterwards (the rotation has three buffers);
* the two wrong models (a run's first link looks into its OWN index of the call before; ``start_min`` from the call's own T behind
  a call of another length) differ from the book on those cases;
* the chain schedules hold, in the oracle's records, reach-backs across link boundaries inside a call, across call boundaries and
  ones that end with segment 0 of a link, so the GPU cases compare such records;
* the entry point's refusals that need no device, the binding, and the Python layer's row packing."""
import ctypes as C
import re

import numpy as np
import pytest

from pyradiotracking_amd import _native, build
from pyradiotracking_amd.analyze import BatchSignalAnalyzer
from tests import chain_cases as cc
from tests import sequence_cases as sq


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
    lib.hc_chain_set.argtypes = [vp, C.c_int]
    lib.hc_chain_set.restype = None
    lib.hc_chain_reset_all.argtypes = [vp]
    lib.hc_chain_reset_all.restype = None
    lib.hc_chain_call.argtypes = [vp, C.c_int] + [vp] * 6
    lib.hc_chain_snapshot.argtypes = [vp, C.c_ulonglong, vp, vp, vp]
    lib.hc_chain_rollback.argtypes = [vp]
    lib.hc_chain_rollback.restype = None
    lib.hc_chain_first_mixed_run.argtypes = [vp, vp]
    return lib


class Book:
    def __init__(self, hc, S, links):
        self.hc, self.S = hc, S
        self.h = hc.hc_presence_new(S, -1)
        hc.hc_chain_set(self.h, links)

    def close(self):
        self.hc.hc_presence_free(self.h)

    def set(self, mask):
        m = np.ascontiguousarray(mask, np.uint8)
        self.hc.hc_presence_set(self.h, m.ctypes.data)

    def call(self, T):
        S = self.S
        absent, took = np.zeros(S, np.uint8), np.zeros(S, np.uint8)
        nsl, buf, idx, tails = np.zeros(S, np.int32), np.zeros(S, np.int32), np.zeros(S, np.int32), np.zeros(2, np.int32)
        self.hc.hc_chain_call(self.h, T, absent.ctypes.data, nsl.ctypes.data, tails.ctypes.data, buf.ctypes.data, idx.ctypes.data, took.ctypes.data)
        return absent, nsl, tuple(int(x) for x in tails), buf, idx, took

    def snapshot(self, k):
        S = self.S
        nsl, buf, idx = (np.zeros(S, np.int32) for _ in range(3))
        assert self.hc.hc_chain_snapshot(self.h, k, nsl.ctypes.data, buf.ctypes.data, idx.ctypes.data) == 0
        return nsl, buf, idx


def _same(got, want, what):
    absent, nsl, tails, buf, idx, took = got
    w_absent, w_nsl, w_tails, w_buf, w_idx, w_took = want
    assert np.array_equal(absent, w_absent), what
    assert tails == w_tails, what
    assert np.array_equal(took, w_took), what
    pres = absent == 0
    assert np.array_equal(buf, w_buf), (what, buf, w_buf)
    assert np.array_equal(idx, w_idx), (what, idx, w_idx)
    assert np.array_equal(nsl[pres], w_nsl[pres]), (what, nsl, w_nsl)


def _differs(got, want):
    absent, nsl, _, buf, idx, _ = got
    _, w_nsl, _, w_buf, w_idx, _ = want
    pres = absent == 0
    return not (np.array_equal(buf, w_buf) and np.array_equal(idx, w_idx) and np.array_equal(nsl[pres], w_nsl[pres]))


def _table_script(name, links):
    """[(mask, T, resets before the call)]: the table's calls; stream 1 reset before call 2, stream links (run 1's first) before call 4"""
    table = cc.run_tables(name, links)
    T = sq.SCHEDULES[name].T
    return [(table[k], T[k], [1] if k == 2 else [links] if k == 4 else []) for k in range(len(T))]


def _random_script(seed, S, links, n=200):
    rng = np.random.default_rng(seed)
    out = []
    away = np.zeros(S // links, int)  # calls a run still sits out
    for k in range(n):
        mask = rng.random(S) < 0.7
        for r in range(S // links):
            if away[r] == 0 and rng.random() < 0.12:
                away[r] = int(rng.integers(1, 5))  # a whole run absent for 1 ... 4 calls
            elif away[r] > 0:
                away[r] -= 1
            if away[r] > 0:
                mask[r * links:(r + 1) * links] = False
        resets = [int(s) for s in np.flatnonzero(rng.random(S) < 0.05)]
        out.append((mask, int(rng.choice([0, 2, 9, 33, 47, 96])), resets))
    return out


SCRIPTS = [(f"{name}-links{links}", name, links) for name in ("A", "P", "B") for links in (2, 3, 4)]


def _drive(hc, script, S, links, wrong=None, rollbacks=False, seed=0):
    """The book and the model side by side; returns the calls on which they differ (the correct model: asserts equality)."""
    book, model = Book(hc, S, links), cc.Model(S, links, wrong)
    rng = np.random.default_rng(seed)
    differing, absent_runs = [], {}
    try:
        for k, (mask, T, resets) in enumerate(script):
            for s in resets:
                hc.hc_presence_reset_stream(book.h, s)
                model.reset[s] = True
            book.set(mask)
            model.present = np.asarray(mask, bool).copy()
            got, want = book.call(T), model.call(T)
            if rollbacks and rng.random() < 0.1:  # the call fails: undone, then made again -- the same answers
                hc.hc_chain_rollback(book.h)
                model.rollback()
                again, want = book.call(T), model.call(T)
                assert all(np.array_equal(a, b) for a, b in zip(got, again)), k
            if wrong is None:
                _same(got, want, f"call {k} T {T}")
                n_calls = k + 1
                snap = book.snapshot(n_calls - 1)  # what a re-analysis inside rt_fetch reads
                assert np.array_equal(snap[1], got[3]) and np.array_equal(snap[2], got[4]) and np.array_equal(snap[0], got[1])
                for r in range(S // links):
                    sl = slice(r * links, (r + 1) * links)
                    if not np.asarray(mask, bool)[sl].any():
                        absent_runs[r] = absent_runs.get(r, 0) + 1
                    else:
                        gap = absent_runs.pop(r, 0)
                        first = r * links + int(np.flatnonzero(np.asarray(mask, bool)[sl])[0])
                        if gap and got[3][first] == cc.READ:
                            differing.append(gap)  # (here: the gap lengths a run came back from with its look-back found)
            elif _differs(got, want):
                differing.append(k)
            if rollbacks and rng.random() < 0.02:  # rt_reset
                hc.hc_chain_reset_all(book.h)
                model.forget()
    finally:
        book.close()
    return differing


@pytest.mark.parametrize("what,name,links", SCRIPTS, ids=[s[0] for s in SCRIPTS])
def test_book_equals_the_model_over_the_presence_tables(hc, what, name, links):
    _drive(hc, _table_script(name, links), 2 * links, links)


@pytest.mark.parametrize("links", [2, 3, 4])
def test_book_equals_the_model_over_random_calls(hc, links):
    S = 3 * links
    gaps = _drive(hc, _random_script(11 + links, S, links), S, links, rollbacks=True, seed=links)
    assert {1, 2, 3, 4} <= set(gaps), sorted(set(gaps))  # every gap length met with the run's look-back found behind it


# (schedule B has one length: there the call's own T is the right one)
WRONG = [(w, n, l, wrong) for w, n, l in SCRIPTS for wrong in ("own_index", "call_T") if not (wrong == "call_T" and n == "B")]


@pytest.mark.parametrize("what,name,links,wrong", WRONG, ids=[f"{s[0]}-{s[3]}" for s in WRONG])
def test_wrong_models_are_rejected(hc, what, name, links, wrong):
    assert len(_drive(hc, _table_script(name, links), 2 * links, links, wrong)) >= 2


def test_wrong_models_are_rejected_by_the_unmasked_gpu_schedules(hc):
    """... and by what the GPU cases run without a mask: every stream present, the per-call lengths of chain_cases.CALLS"""
    for base, links in (("A", 4), ("P", 4), ("A", 3)):
        S = cc.R * links
        script = [(np.ones(S, bool), T, []) for T in cc.CALLS[base][0]]
        _drive(hc, script, S, links)
        assert len(_drive(hc, script, S, links, "own_index")) == len(script) - 1
        assert len(_drive(hc, script, S, links, "call_T")) >= 3


def test_uniform_values_per_run(hc):
    book = Book(hc, 6, 3)
    try:
        v = np.array([1, 1, 1, 2, 2, 2], np.float32)
        assert hc.hc_chain_first_mixed_run(book.h, v.ctypes.data) == -1
        v[4] = 3
        assert hc.hc_chain_first_mixed_run(book.h, v.ctypes.data) == 1
        v[0] = np.nan  # (a NaN equals nothing: mixed)
        assert hc.hc_chain_first_mixed_run(book.h, v.ctypes.data) == 0
    finally:
        book.close()


CHAINS = [("A", 4, 256), ("P", 4, 256), ("A", 3, 256), ("P", 4, 64), ("P", 4, 300), ("P", 4, 1024)]


@pytest.mark.parametrize("base,links,nperseg", CHAINS, ids=[f"{b}{l}-{n}" for b, l, n in CHAINS])
def test_chain_schedules_reach_back_across_link_and_call_boundaries_and_end_at_t0(base, links, nperseg):
    name = cc.schedule(base, links)
    sched = sq.SCHEDULES[name]
    assert len(sched.T) == links * cc.n_calls(base) and len(set(sched.T)) >= 4 and len(sched.T) // links >= 4
    for c in range(cc.n_calls(base)):  # all links of a call have one length
        assert len({(t, g) for t, g in zip(sched.T[c * links:(c + 1) * links], sq.rag(sched, nperseg)[c * links:(c + 1) * links])}) == 1
    kinds = cc.boundary_kinds(name, nperseg, links)
    assert len(kinds["link"]) >= 3 and len(kinds["call"]) >= 3 and len(kinds["t0"]) >= 3, {k: len(v) for k, v in kinds.items()}
    assert any(k % links for k, _, _ in kinds["t0"]) and any(k % links == 0 for k, _, _ in kinds["t0"])
    if base == "A":
        assert 2 in sched.T


def test_entry_point_is_declared_bound_and_refuses_without_a_device():
    assert "rt_set_chain" in _native.ABI_SYMBOLS
    header = open(build.os.path.join(build.REPO, "include", "rt_analyze.h")).read()
    assert re.search(r"int\s+rt_set_chain\(rt_handle \*h, int32_t links\);", header)
    for word in ("pending", "lanes > 1", "float64 handle", "detrend guard", "RT_MODE_RUNFILTER"):
        assert word in header.split("consecutive buffers of one recording")[1], word
    lib = _native.load_library()
    assert lib.rt_set_chain(None, 4) == _native.RT_E_INVALID
    assert lib.rt_set_chain(None, 0) == _native.RT_E_INVALID


def test_python_layer_refuses_lanes_and_float64_before_anything_native():
    with pytest.raises(ValueError, match="lanes"):
        BatchSignalAnalyzer(["a"], chain=4, lanes=2)
    with pytest.raises(ValueError, match="float64"):
        BatchSignalAnalyzer(["a"], chain=4, precision="float64")


class _Rows(BatchSignalAnalyzer):
    """``_chain_rows`` without a handle"""

    def __init__(self, R, L, B):
        self.run_devices, self.chain, self.sdr_callback_length = [str(r) for r in range(R)], L, B
        self.devices = [d for d in self.run_devices for _ in range(L)]
        self.masks = []

    def set_present(self, present=None):
        self.masks.append(list(present))

    def __del__(self):
        pass


def test_row_packing_of_the_python_layer():
    a = _Rows(2, 4, 8)
    x = np.arange(2 * 32).reshape(2, 32).astype(np.complex64)
    rows = a._chain_rows(x, 1, None)
    assert rows.shape == (8, 8) and np.array_equal(rows[5], x[1, 8:16]) and a.masks[-1] == [True] * 8 and a._chain_call == (4, 8)
    rows = a._chain_rows(x[:, :16], 1, None)  # two of four links: the suffix mask, rows of the absent links in place
    assert rows.shape == (8, 8) and np.array_equal(rows[4], x[1, :8]) and np.array_equal(rows[1], x[0, 8:16])
    assert a.masks[-1] == [True, True, False, False] * 2 and a._chain_call == (2, 8)
    rows = a._chain_rows(x[:, :5], 1, None)  # a short last buffer: one link
    assert rows.shape == (8, 5) and a.masks[-1] == [True, False, False, False] * 2 and a._chain_call == (1, 5)
    raw = np.arange(2 * 24, dtype=np.uint8).reshape(2, 24)  # interleaved I, Q: links=3 buffers of 4 samples
    rows = a._chain_rows(raw, 2, 3)
    assert rows.shape == (8, 8) and np.array_equal(rows[6], raw[1, 16:24]) and a.masks[-1] == [True, True, True, False] * 2
    assert a.run_of(np.array([0, 3, 4, 7])).tolist() == [0, 0, 1, 1] and a.link_of(np.array([0, 3, 4, 7])).tolist() == [0, 3, 0, 3]
    with pytest.raises(ValueError):
        a._chain_rows(x[:, :20], 1, None)  # no whole number of buffers
    with pytest.raises(ValueError):
        a._chain_rows(np.zeros((2, 40), np.complex64), 1, None)  # five buffers on a chain of four
    with pytest.raises(ValueError):
        a._chain_rows(np.zeros((3, 8), np.complex64), 1, None)  # three rows for two recordings
