"""The look-back ledger (csrc/rt_ledger.h: StreamLedger, LedgerCall) -- the one driver of a handle's look-back state, float32 and
float64 alike -- through ``_rt_hostcheck.so``.  tests/test_present_contract.py, test_chain_contract.py and
test_record_iq_contract.py hold the same object to their NumPy models in the per-stream regime; here is what those never covered:

* the lock-step regime (one segment count per handle) against hand-written traces: resets, a T = 0 call, rollbacks, forget_all;
* lock-step and "per-stream rows on, every stream present" see the same look-back rows and the same rotation in every call of 200
  seeded random schedules, and ``any_reset()`` says what ``reset_pending`` holds after every step of them;
* switching to the per-stream regime in mid-sequence inherits the handle's one count and leaves the call in flight alone;
* a plain call (lock-step, nothing pending, record-IQ off) touches none of its snapshot's vectors: no per-stream work, no allocation;
* the same walk as a stand-alone program under AddressSanitizer and UBSan (tests/c/ledger_walk.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from pyradiotracking_amd import build

S, K = 5, 3
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hc():
    lib = C.CDLL(build.build_hostcheck())
    vp = C.c_void_p
    lib.hc_ledger_new.argtypes = [C.c_int, C.c_int]
    lib.hc_ledger_new.restype = vp
    lib.hc_ledger_call.argtypes = [vp, C.c_int, vp, vp, vp]
    lib.hc_ledger_call.restype = C.c_longlong
    lib.hc_ledger_snapshot.argtypes = [vp, C.c_ulonglong, vp, vp]
    lib.hc_ledger_mark_changed.argtypes = [vp, vp]
    lib.hc_ledger_mark_changed.restype = None
    lib.hc_ledger_activate_presence.argtypes = [vp]
    lib.hc_ledger_activate_presence.restype = None
    lib.hc_ledger_state.argtypes = [vp, vp, vp, vp]
    lib.hc_ledger_state.restype = None
    lib.hc_ledger_call_footprint.argtypes = [vp, C.c_int, vp]
    # (one object behind every family of exports: these four act on a ledger handle as they do on a presence handle)
    lib.hc_presence_free.argtypes = [vp]
    lib.hc_presence_free.restype = None
    lib.hc_presence_reset_stream.argtypes = [vp, C.c_int]
    lib.hc_presence_reset_stream.restype = None
    lib.hc_presence_reset_all.argtypes = [vp]
    lib.hc_presence_reset_all.restype = None
    lib.hc_presence_rollback.argtypes = [vp]
    lib.hc_presence_rollback.restype = None
    return lib


class Ledger:
    def __init__(self, hc, per_stream=False):
        self.hc = hc
        self.h = hc.hc_ledger_new(S, -1)
        if per_stream:
            hc.hc_ledger_activate_presence(self.h)

    def close(self):
        self.hc.hc_presence_free(self.h)

    def call(self, T):
        rows, tails, took = np.zeros(S, np.int32), np.zeros(2, np.int32), np.zeros(S, np.uint8)
        k = self.hc.hc_ledger_call(self.h, T, rows.ctypes.data, tails.ctypes.data, took.ctypes.data)
        return k, rows.tolist(), tails.tolist(), took.tolist()

    def snapshot(self, k):
        rows, tails = np.zeros(S, np.int32), np.zeros(2, np.int32)
        regime = self.hc.hc_ledger_snapshot(self.h, k, rows.ctypes.data, tails.ctypes.data)
        return regime, rows.tolist(), tails.tolist()

    def reset_stream(self, s):
        self.hc.hc_presence_reset_stream(self.h, s)

    def mark_changed(self, changed):
        a = np.asarray(changed, np.uint8)
        self.hc.hc_ledger_mark_changed(self.h, a.ctypes.data)

    def rollback(self):
        self.hc.hc_presence_rollback(self.h)

    def forget_all(self):
        self.hc.hc_presence_reset_all(self.h)

    def activate_presence(self):
        self.hc.hc_ledger_activate_presence(self.h)

    def state(self):
        sc, rp, ps = np.zeros(4, np.int32), np.zeros(S, np.uint8), np.full(S, -99, np.int32)
        self.hc.hc_ledger_state(self.h, sc.ctypes.data, rp.ctypes.data, ps.ctypes.data)
        return dict(tail_cur=int(sc[0]), n_seg_last=int(sc[1]), any_reset=bool(sc[2]), per_stream_on=bool(sc[3]), reset_pending=rp.tolist(),
                    per_stream=ps.tolist() if sc[3] else None)

    def footprint(self, slot):
        out = np.zeros(64, np.uint64)
        n = self.hc.hc_ledger_call_footprint(self.h, slot, out.ctypes.data)
        return out[: 2 * n].tolist()


@pytest.fixture
def led(hc):
    l = Ledger(hc)
    yield l
    l.close()


# ---- the lock-step regime against hand-written traces ----------------------------------------------------------------------------
def test_a_reset_is_taken_by_the_next_call_and_by_no_later_one(led):
    assert led.call(7) == (0, [-1] * 5, [0, 1], [0] * 5)
    led.reset_stream(2)
    assert led.state()["reset_pending"] == [0, 0, 1, 0, 0] and led.state()["any_reset"]
    assert led.call(3) == (1, [7, 7, -1, 7, 7], [1, 2], [0, 0, 1, 0, 0])
    assert led.state()["reset_pending"] == [0] * 5 and not led.state()["any_reset"]
    assert led.call(2) == (2, [3] * 5, [2, 0], [0] * 5)
    assert led.call(7) == (3, [2] * 5, [0, 1], [0] * 5)


def test_two_resets_pending_on_different_streams(led):
    led.call(7)
    led.reset_stream(0)
    led.mark_changed([0, 0, 0, 0, 1])
    assert led.state()["reset_pending"] == [1, 0, 0, 0, 1]
    assert led.call(2)[1:] == ([-1, 7, 7, 7, -1], [1, 2], [1, 0, 0, 0, 1])
    assert led.call(3)[1:] == ([2] * 5, [2, 0], [0] * 5)


def test_an_empty_call_leaves_a_count_of_zero_not_none(led):
    led.call(7)
    assert led.call(0)[1] == [7] * 5
    assert led.state()["n_seg_last"] == 0
    assert led.call(3)[1] == [0] * 5  # (`_spectrogram_last` is an empty map, not None)


def test_a_rolled_back_call_leaves_no_trace(led):
    led.call(7)
    led.call(3)
    before = led.state()
    assert before["tail_cur"] == 2 and before["n_seg_last"] == 3
    led.call(2)
    assert led.state()["n_seg_last"] == 2
    led.rollback()
    assert led.state() == before
    assert led.snapshot(2)[0] == -1 and led.snapshot(1) == (0, [7] * 5, [1, 2])  # (the older call in flight keeps its snapshot)
    # ... and after it took resets: they are pending again, on the same streams
    led.reset_stream(1)
    led.reset_stream(3)
    before = led.state()
    assert before["reset_pending"] == [0, 1, 0, 1, 0] and before["any_reset"]
    assert led.call(7)[1:] == ([3, -1, 3, -1, 3], [2, 0], [0, 1, 0, 1, 0])
    assert not led.state()["any_reset"]
    led.rollback()
    assert led.state() == before
    assert led.call(2)[1:] == ([3, -1, 3, -1, 3], [2, 0], [0, 1, 0, 1, 0])  # the next call takes them instead


def test_forget_all(led):
    led.call(7)
    led.call(3)
    led.reset_stream(4)
    led.forget_all()
    st = led.state()
    assert st["n_seg_last"] == -1 and st["reset_pending"] == [0] * 5 and not st["any_reset"]
    assert st["tail_cur"] == 2  # (the rotation goes on: calls in flight still read their buffers)
    assert led.call(2)[1:] == ([-1] * 5, [2, 0], [0] * 5)


# ---- lock-step against the per-stream regime with every stream present -----------------------------------------------------------
def schedule(seed):
    rng = np.random.default_rng(seed)
    ops = []
    for _ in range(int(rng.integers(1, 13))):
        op = int(rng.integers(0, 8))
        if op < 4:
            ops.append(("call", int(rng.choice([0, 2, 3, 7]))))
        elif op == 4:
            ops.append(("reset_stream", int(rng.integers(0, S))))
        elif op == 5:
            ops.append(("mark_changed", (rng.integers(0, 3, S) == 0).astype(np.uint8).tolist()))
        elif op == 6:
            ops.append(("rollback", None))
        else:
            ops.append(("forget_all", None))
    return ops


def run(hc, ops, per_stream):
    """What every call of the schedule saw, and any_reset() against reset_pending after every step."""
    l = Ledger(hc, per_stream)
    seen, can_undo = [], False
    try:
        for op, arg in ops:
            if op == "call":
                _, rows, tails, _ = l.call(arg)
                seen.append((rows, tails))
                can_undo = True
            elif op == "rollback":
                if can_undo:  # (the newest call, once)
                    l.rollback()
                    seen.append("undone")
                can_undo = False
            elif op == "forget_all":
                l.forget_all()
                can_undo = False  # (a handle never rolls a call back across an rt_reset)
            else:
                getattr(l, op)(arg)
            st = l.state()
            assert st["any_reset"] == any(st["reset_pending"]), (ops, op)
            assert st["per_stream_on"] == per_stream
            seen.append(st["reset_pending"])
    finally:
        l.close()
    return seen


def test_both_regimes_see_the_same_rows_in_200_random_schedules(hc):
    n_calls = n_undone = 0
    for seed in range(200):
        ops = schedule(seed)
        a, b = run(hc, ops, False), run(hc, ops, True)
        assert a == b, (seed, ops)
        n_calls += sum(isinstance(x, tuple) for x in a)
        n_undone += a.count("undone")
    assert n_calls > 400 and n_undone > 40  # (the schedules did exercise both)


def test_switching_to_per_stream_rows_in_mid_sequence(led):
    led.call(7)
    led.call(3)  # in flight
    led.reset_stream(2)  # still pending
    in_flight = led.snapshot(1)
    assert in_flight == (0, [7] * 5, [1, 2])
    led.activate_presence()
    st = led.state()
    assert st["per_stream_on"] and st["per_stream"] == [3] * 5  # every stream inherits the handle's one count
    assert st["reset_pending"] == [0, 0, 1, 0, 0] and st["any_reset"] and st["tail_cur"] == 2
    assert led.snapshot(1) == in_flight
    assert led.call(2)[1:3] == ([3, 3, -1, 3, 3], [2, 0])
    assert led.snapshot(2)[0] == 1 and led.snapshot(1) == in_flight
    assert led.state()["per_stream"] == [2] * 5 and not led.state()["any_reset"]


# ---- no per-stream work on the plain path ----------------------------------------------------------------------------------------
def test_a_plain_call_leaves_its_snapshots_vectors_alone(led):
    led.reset_stream(0)
    for T in (7, 3):  # warm-up: both slots have held a call, the first with a reset
        led.call(T)
    before = [led.footprint(0), led.footprint(1)]
    assert len(before[0]) == 40  # 20 vectors: (data, capacity) each
    for T in (7, 2, 0, 3):
        k, rows, _, took = led.call(T)
        assert took == [0] * 5
    assert [led.footprint(0), led.footprint(1)] == before


# ---- the walk under sanitizers ---------------------------------------------------------------------------------------------------
def test_ledger_walk_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "ledger_walk"
    # (the runtimes linked statically: the program then runs the same whatever else the environment loads into a process)
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(REPO, "pyradiotracking_amd", "csrc"), "-o", str(exe), os.path.join(REPO, "tests", "c", "ledger_walk.cpp")],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr)
