"""CPU tests of RT_MODE_AUTO's state machine (csrc/rt_core.h: AutoPolicy, overflow_step), driven through _rt_hostcheck.so operation
by operation as rt_analyze.hip drives it: begin a call (rt_process), overflow step and climb (rt_fetch's re-run loop), settle
(rt_fetch, once a call's result stands), restore (a failed or rolled-back enqueue).

Every expected state below is written out by hand from the rules (rt_core.h), not computed: state = (level, dense_sticky,
sticky_len, abs_hot_seen, abs_hot_valid).  No GPU."""
import ctypes as C

import pytest

from pyradiotracking_amd import _native, build

A, D, S, P, R = _native.RT_MODE_AUTO, _native.RT_MODE_DENSE, _native.RT_MODE_SPARSE, _native.RT_MODE_PREFILTER, _native.RT_MODE_RUNFILTER
LISTS = 16 * 1024    # kBuckets x hot_capacity: cells a stream's sparse lists hold
CELLS = 1171 * 256   # T x N of a call
K_SLOTS = 2          # calls in flight: what a probe sets dense_sticky to


@pytest.fixture(scope="module")
def hc():
    lib = C.CDLL(build.build_hostcheck())
    lib.hc_auto_new.restype = C.c_void_p
    lib.hc_auto_new.argtypes = [C.c_int, C.c_int]
    lib.hc_auto_free.argtypes = [C.c_void_p]
    lib.hc_auto_begin_call.argtypes = [C.c_void_p, C.c_int, C.c_ulonglong, C.c_ulonglong, C.POINTER(C.c_int)]
    lib.hc_auto_restore.argtypes = [C.c_void_p, C.c_int]
    lib.hc_auto_overflow_step.argtypes = [C.c_int] * 8
    lib.hc_auto_climb.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.hc_auto_settle.argtypes = [C.c_void_p] + [C.c_int] * 5 + [C.c_longlong] * 5 + [C.c_int, C.c_uint, C.c_int]
    lib.hc_auto_state.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
    return lib


class Policy:
    """One hc_auto_* handle (no logic of its own: every method is one call into the library)."""

    def __init__(self, hc, pre, run):
        self.hc, self.p = hc, hc.hc_auto_new(pre, run)
        self.restore_point = None

    def __del__(self):
        self.hc.hc_auto_free(self.p)

    def begin(self, cfg=A, lists=LISTS, cells=CELLS):
        rp = C.c_int(-1)
        mode = self.hc.hc_auto_begin_call(self.p, cfg, lists, cells, C.byref(rp))
        self.restore_point = rp.value
        return mode

    def restore(self, point):
        self.hc.hc_auto_restore(self.p, point)

    def climb(self, frm, first):
        return self.hc.hc_auto_climb(self.p, frm, int(first))

    def settle(self, mode, fell_back=0, settled=0, cfg=A, counts=1, n_hot=0, seg_total=-1, n_took_part=8, n_seg=100, N=256,
               abs_counted=0, abs_hot=0, n_dense=0):
        self.hc.hc_auto_settle(self.p, settled, cfg, mode, fell_back, counts, n_hot, seg_total, n_took_part, n_seg, N, abs_counted, abs_hot, n_dense)

    @property
    def state(self):
        out = (C.c_longlong * 5)()
        self.hc.hc_auto_state(self.p, out)
        return tuple(out)

    def stay(self, n, level):
        """`n` calls that run on the handle's level and go through there."""
        for i in range(n):
            assert self.begin() == level, i
            self.settle(level)


def test_a_new_handle_runs_sparse_and_a_pinned_one_runs_its_mode(hc):
    p = Policy(hc, 1, 1)
    assert p.state == (S, 0, 16, 0, 0)
    assert p.begin() == S and p.state == (S, 0, 16, 0, 0)  # (sparse has no level below: not a probe)
    for mode in (D, S, P, R):
        assert p.begin(cfg=mode) == mode
        p.settle(mode, cfg=mode, n_hot=10**9, seg_total=10**6)
        assert p.state == (S, 0, 16, 0, 0)


@pytest.mark.parametrize("pre,run,up", [(0, 0, D), (1, 0, P), (0, 1, R), (1, 1, P)])
def test_a_level_up_holds_for_16_calls_and_the_17th_probes(hc, pre, run, up):
    p = Policy(hc, pre, run)
    assert p.begin() == S
    assert p.climb(S, True) == up  # (its sparse lists overflowed)
    p.settle(up, fell_back=1)
    assert p.state[:3] == (up, 16, 32)
    for left in (15, 14, 13, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0):
        assert p.begin() == up
        assert p.state[:3] == (up, left, 32)
        p.settle(up)
    assert p.begin() == S  # the probe: one at a time, the calls enqueued behind it stay on the level
    assert p.state[:3] == (up, K_SLOTS, 32)
    assert p.begin() == up and p.begin() == up
    assert p.state[:3] == (up, 0, 32)


def test_failed_probes_double_the_interval_up_to_1024(hc):
    p = Policy(hc, 0, 1)
    assert p.begin() == S
    for interval, nxt in ((16, 32), (32, 64), (64, 128), (128, 256), (256, 512), (512, 1024), (1024, 1024), (1024, 1024), (1024, 1024)):
        assert p.climb(S, True) == R
        p.settle(R, fell_back=1)
        assert p.state[:3] == (R, interval, nxt)
        p.stay(interval, R)
        assert p.state[:3] == (R, 0, nxt)
        assert p.begin() == S
        assert p.state[:3] == (R, K_SLOTS, nxt)


def test_a_call_that_climbs_two_levels_doubles_the_interval_once(hc):
    p = Policy(hc, 1, 1)
    assert p.begin() == S
    assert p.climb(S, True) == P
    assert p.state[:3] == (P, 16, 32)
    assert p.climb(P, False) == R
    assert p.state[:3] == (R, 16, 32)
    assert p.climb(R, False) == D
    p.settle(D, fell_back=1)
    assert p.state[:3] == (D, 16, 32)
    # (the same call climbing as if each level were its first: what `first` guards against)
    q = Policy(hc, 1, 1)
    q.begin()
    q.climb(S, True)
    q.climb(P, True)
    assert q.state[:3] == (R, 32, 64)


def test_a_probe_that_goes_through_moves_the_handle_down(hc):
    p = Policy(hc, 1, 0)  # sparse < chunk bits < dense
    assert p.begin() == S
    assert p.climb(S, True) == P and p.climb(P, False) == D
    p.settle(D, fell_back=1)
    p.stay(16, D)
    assert p.state[:3] == (D, 0, 32)
    assert p.begin() == P
    assert p.state[:3] == (D, K_SLOTS, 32)
    p.settle(P)
    assert p.state[:3] == (P, 16, 16)  # on a pre-filter level: the usual interval before sparse is probed
    p.stay(16, P)
    assert p.begin() == S
    assert p.state[:3] == (P, K_SLOTS, 16)
    p.settle(S)
    assert p.state[:3] == (S, 0, 16)
    assert p.begin() == S and p.state[:3] == (S, 0, 16)


def _on_exact_level(hc):
    p = Policy(hc, 1, 1)
    assert p.climb(P, True) == R
    assert p.begin() == R
    assert p.state[:3] == (R, 15, 32)
    return p


@pytest.mark.parametrize("n_took_part,at,over", [(8, 400, 401), (4, 200, 201)])
def test_more_than_half_of_the_segments_makes_the_exact_level_unselective(hc, n_took_part, at, over):
    """seg_total * 2 > n_took_part * n_seg, n_seg = 100: the streams that took part count, not the batch."""
    p = _on_exact_level(hc)
    p.settle(R, seg_total=at, n_took_part=n_took_part)
    assert p.state[:3] == (R, 15, 32)
    p = _on_exact_level(hc)
    p.settle(R, seg_total=over, n_took_part=n_took_part)
    assert p.state[:3] == (D, 32, 64)  # up without a re-run (no fell_back), the interval doubles
    # only the exact pre-filter keeps that count
    p = Policy(hc, 1, 1)
    assert p.climb(S, True) == P and p.begin() == P
    p.settle(P, seg_total=10**6, n_took_part=n_took_part)
    assert p.state[:3] == (P, 15, 32)


@pytest.mark.parametrize("mode,frm", [(R, P), (P, S)])
def test_more_than_a_32nd_of_the_cells_makes_a_prefilter_level_unselective(hc, mode, frm):
    """n_hot * 32 > n_took_part * n_seg * N = 8 * 100 * 256 = 204 800 = 32 * 6 400."""
    up = {R: D, P: R}[mode]
    p = Policy(hc, 1, 1)
    assert p.climb(frm, True) == mode and p.begin() == mode
    p.settle(mode, n_hot=6400)
    assert p.state[:3] == (mode, 15, 32)
    p.settle(mode, n_hot=6401)
    assert p.state[:3] == (up, 32, 64)
    # half the streams present: half the cells
    p = Policy(hc, 1, 1)
    assert p.climb(frm, True) == mode and p.begin() == mode
    p.settle(mode, n_hot=3200, n_took_part=4)
    assert p.state[:3] == (mode, 15, 32)
    p.settle(mode, n_hot=3201, n_took_part=4)
    assert p.state[:3] == (up, 32, 64)


def test_the_sparse_and_dense_levels_are_never_unselective_and_calls_that_do_not_count_say_nothing(hc):
    p = Policy(hc, 1, 1)
    assert p.begin() == S
    p.settle(S, n_hot=10**9, seg_total=10**6)
    assert p.state[:3] == (S, 0, 16)
    p = _on_exact_level(hc)
    p.settle(D, n_hot=10**9, seg_total=10**6)
    p.settle(R, n_hot=10**9, seg_total=10**6, counts=0)  # (an rt_extract, or a call without segments)
    p.settle(S, counts=0)
    assert p.state[:3] == (R, 15, 32)


def test_an_unselective_probe_does_not_move_the_handle_down(hc):
    p = Policy(hc, 0, 1)  # sparse < exact < dense
    assert p.begin() == S
    assert p.climb(S, True) == R and p.climb(R, False) == D
    p.settle(D, fell_back=1)
    p.stay(16, D)
    assert p.begin() == R
    assert p.state[:3] == (D, K_SLOTS, 32)
    p.settle(R, seg_total=401)
    assert p.state[:3] == (D, 32, 64)


def test_settling_a_call_twice_equals_settling_it_once(hc):
    """rt_fetch passes over a call twice (size query or peek, then delivery); the second pass says so."""
    once, twice, unguarded = _on_exact_level(hc), _on_exact_level(hc), _on_exact_level(hc)
    once.settle(R, seg_total=401)
    twice.settle(R, seg_total=401)
    twice.settle(R, seg_total=401, settled=1)
    assert once.state == (D, 32, 64, 0, 0) and twice.state == (D, 32, 64, 0, 0)
    unguarded.settle(R, seg_total=401)
    unguarded.settle(R, seg_total=401)  # (what the mark prevents: the interval doubled once per pass)
    assert unguarded.state == (D, 64, 128, 0, 0)
    # a probe that went through
    for passes in (1, 2):
        p = Policy(hc, 1, 0)
        p.climb(S, True)
        p.stay(16, P)
        assert p.begin() == S
        for k in range(passes):
            p.settle(S, settled=k)
        assert p.state == (S, 0, 16, 0, 0)


def test_a_probe_the_last_count_rules_out_is_not_made(hc):
    p = Policy(hc, 0, 1)
    assert p.begin() == S and p.climb(S, True) == R
    p.settle(R, fell_back=1, abs_counted=1, abs_hot=LISTS + 1)  # one cell more than the sparse lists hold
    assert p.state == (R, 16, 32, LISTS + 1, 1)
    p.stay(16, R)
    assert p.state == (R, 0, 32, LISTS + 1, 1)
    for _ in range(3):  # the call runs on the level, no back-off, the next call looks again
        assert p.begin() == R
        assert p.state == (R, 0, 32, LISTS + 1, 1)
        p.settle(R)
    p.settle(R, abs_counted=1, abs_hot=LISTS)  # exactly full still fits
    assert p.begin() == S
    assert p.state == (R, K_SLOTS, 32, LISTS, 1)
    # the chunk bits from the exact level while more than 3/4 of a stream's cells pass the absolute threshold
    q = Policy(hc, 1, 1)
    assert q.climb(P, True) == R
    q.settle(R, fell_back=1, abs_counted=1, abs_hot=3 * CELLS // 4 + 1)
    q.stay(16, R)
    assert q.begin() == R and q.state[:3] == (R, 0, 32)
    q.settle(R, abs_counted=1, abs_hot=3 * CELLS // 4)
    assert q.begin() == P and q.state[:3] == (R, K_SLOTS, 32)


def test_restore_puts_the_probe_counter_back_and_nothing_else(hc):
    p = Policy(hc, 1, 0)
    assert p.begin() == S and p.climb(S, True) == P
    p.settle(P, fell_back=1, abs_counted=1, abs_hot=7)
    assert p.begin() == P
    assert p.restore_point == 16 and p.state == (P, 15, 32, 7, 1)
    p.restore(16)
    assert p.state == (P, 16, 32, 7, 1)
    p.stay(16, P)
    assert p.begin() == S  # a probe whose enqueue fails: the next call is the probe again
    assert p.restore_point == 0 and p.state == (P, K_SLOTS, 32, 7, 1)
    p.restore(0)
    assert p.state == (P, 0, 32, 7, 1)
    assert p.begin() == S


def test_the_count_over_the_absolute_threshold_stands_until_a_whole_batch_runs_dense(hc):
    p = Policy(hc, 1, 1)
    p.settle(P, abs_counted=1, abs_hot=777)
    assert p.state[3:] == (777, 1)
    p.settle(S)  # a call without a count leaves it
    assert p.state[3:] == (777, 1)
    p.settle(D, fell_back=1, n_dense=3)  # ... and so does one that counts as dense for a few streams only
    assert p.state[3:] == (777, 1)
    p.settle(R, abs_counted=1, abs_hot=5)
    assert p.state[3:] == (5, 1)
    p.settle(D, fell_back=1, n_dense=0)  # the whole batch dense: the dense path keeps no count
    assert p.state[3:] == (5, 0)
    p.settle(R, abs_counted=1, abs_hot=9, settled=1)  # (the count is the call's, on either pass)
    assert p.state[3:] == (9, 1)


# overflow_step: O = again on its own row means, F = RT_E_HOT_OVERFLOW, P = partial dense, U = level up
_STEP = {"O": 0, "F": 1, "P": 2, "U": 3}
_N_BAD = (0, 1, 32, 33)
_N_STREAMS = (4, 128, 129, 4096)  # 4 * 32 <= 128: the quarter rule's boundary
# a grid: one row per n_bad, one letter per n_streams
_UP = "UUUU UUUU UUUU UUUU"
_FEW = "UUUU PPPP UPPP UUUU"        # a few of many: at most 32 and a quarter of the batch
_STALE_FEW = "OOOO PPPP OPPP OOOO"  # stale thresholds: the few still go dense on their own, otherwise the same level again
_FAIL = "FFFF FFFF FFFF FFFF"
_OWN = "OOOO OOOO OOOO OOOO"
# (configured mode is AUTO, mode the call ran on, kFlagThrStale, thr_rerun) -> (grid without a middle level, grid with one)
_TABLE = {
    (1, S, 0, 0): (_FEW, _UP),  # sparse with a middle level still ahead: the whole batch goes there
    (1, S, 0, 1): (_FEW, _UP),
    (1, S, 1, 0): (_FEW, _UP),  # (the stale bit means something on the exact level only)
    (1, S, 1, 1): (_FEW, _UP),
    (1, P, 0, 0): (_FEW, _FEW),
    (1, P, 0, 1): (_FEW, _FEW),
    (1, P, 1, 0): (_FEW, _FEW),
    (1, P, 1, 1): (_FEW, _FEW),
    (1, R, 0, 0): (_FEW, _FEW),
    (1, R, 0, 1): (_FEW, _FEW),
    (1, R, 1, 0): (_STALE_FEW, _STALE_FEW),
    (1, R, 1, 1): (_FEW, _FEW),  # once per call
    (1, D, 0, 0): (_FEW, _FEW),
    (1, D, 0, 1): (_FEW, _FEW),
    (1, D, 1, 0): (_FEW, _FEW),
    (1, D, 1, 1): (_FEW, _FEW),
    (0, S, 0, 0): (_FAIL, _FAIL),
    (0, S, 0, 1): (_FAIL, _FAIL),
    (0, S, 1, 0): (_FAIL, _FAIL),
    (0, S, 1, 1): (_FAIL, _FAIL),
    (0, P, 0, 0): (_FAIL, _FAIL),
    (0, P, 0, 1): (_FAIL, _FAIL),
    (0, P, 1, 0): (_FAIL, _FAIL),
    (0, P, 1, 1): (_FAIL, _FAIL),
    (0, R, 0, 0): (_FAIL, _FAIL),
    (0, R, 0, 1): (_FAIL, _FAIL),
    (0, R, 1, 0): (_OWN, _OWN),  # an explicit RT_MODE_RUNFILTER handle does not fail
    (0, R, 1, 1): (_FAIL, _FAIL),
    (0, D, 0, 0): (_FAIL, _FAIL),
    (0, D, 0, 1): (_FAIL, _FAIL),
    (0, D, 1, 0): (_FAIL, _FAIL),
    (0, D, 1, 1): (_FAIL, _FAIL),
}


@pytest.mark.parametrize("pre,run", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_overflow_step_decision_table(hc, pre, run):
    for (is_auto, mode, stale, thr_rerun), grids in _TABLE.items():
        rows = grids[1 if (pre or run) else 0].split()
        # a handle pinned to a mode is pinned to the mode its calls run on
        for cfg in ((A,) if is_auto else (mode,)):
            for n_bad, row in zip(_N_BAD, rows):
                for n_streams, want in zip(_N_STREAMS, row):
                    got = hc.hc_auto_overflow_step(mode, thr_rerun, stale, n_bad, n_streams, cfg, pre, run)
                    assert got == _STEP[want], (is_auto, mode, stale, thr_rerun, n_bad, n_streams, pre, run)
