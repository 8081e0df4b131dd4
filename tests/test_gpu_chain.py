"""Consecutive buffers of a recording as the streams of one call, on the GPU (``rt_set_chain``).

The yardstick is a plain handle of R = 2 streams on the same build, made with the same explicit ``segs_per_chunk`` (the order of
the row sums' partial sums) and fed the same buffers one call after another; the chained handle (R x links streams, ``links``
buffers per call) must deliver the same records byte for byte after mapping (call, stream) -> (recording, buffer) -- row means and
record cells too where the flags are on.  The inputs are the chain schedules of tests/chain_cases.py (the generator of
tests/sequence_cases.py; the CPU file shows that they hold reach-backs across link boundaries, across call boundaries and ones
ending at t = 0 of a link), and without a mask the yardstick's runs are held to ``sequence_cases.oracle_run`` by
``sequence_cases.hold_sequence``'s own tolerances, so that a fault common to both handles cannot hide.  The inputs carry no constant
offset, so the detrend guard marks nothing (``rt_call_info`` has no field for it; one case runs ``RT_FLAG_NO_LIN_DETREND``).

``-s`` prints per case the trace ``call:mode_used/fell_back/dense streams/records`` of the chained handle."""
import datetime

import numpy as np
import pytest

from pyradiotracking_amd import _native
from pyradiotracking_amd.analyze import BatchSignalAnalyzer, SignalAnalyzer
from tests import chain_cases as cc
from tests import sequence_cases as sq
from tests.test_gpu_float64 import form_of

pytestmark = pytest.mark.gpu
R = cc.R


@pytest.fixture(autouse=True)
def _need_gpu():
    if _native.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")


def _spc(nperseg):
    """what a batch this small gets by default (rt_core.h: choose_chunk), given explicitly to both handles"""
    return 8 if nperseg >= 8192 else 4


def _handle(n_streams, name, nperseg, mode, fmt="c64", min_hops=sq.MIN_HOPS, **extra):
    kw = dict(segs_per_chunk=_spc(nperseg))
    kw.update(extra)
    return BatchSignalAnalyzer([str(i) for i in range(n_streams)], sdr_callback_length=sq.max_samples(sq.SCHEDULES[name], nperseg), mode=mode,
                               **sq.case_settings(nperseg, fmt, min_hops=min_hops), **kw)


def _chained(name, nperseg, links, mode, fmt="c64", min_hops=sq.MIN_HOPS, **extra):
    b = _handle(R * links, name, nperseg, mode, fmt, min_hops, **extra)
    b.native.set_chain(links)
    return b


def _equal(chained_runs, plain_runs, links, what):
    mapped = cc.by_buffer(chained_runs, links)
    assert len(mapped) == len(plain_runs)
    for k, (mine, (want, _)) in enumerate(zip(mapped, plain_runs)):
        assert sq.rec_key(mine) == sq.rec_key(want), f"{what} buffer {k} (call {k // links} link {k % links}): records\n got  {sq.rec_key(mine)}\n want {sq.rec_key(want)}"
        assert mine.tobytes() == want.tobytes(), f"{what} buffer {k} (call {k // links} link {k % links}): the same records with other bytes"


def _case(base, links, nperseg, mode, fmt="c64", min_hops=sq.MIN_HOPS, present=None, pipelined=False, events=(), oracle=True, plain_mode=None,
          before_call=None, before_buffer=None, after_fetch=None, expect_mode=None, **extra):
    name = cc.schedule(base, links)
    what = f"chain {name} nperseg {nperseg} {mode} {fmt} {extra}"
    b = _chained(name, nperseg, links, mode, fmt, min_hops, **extra)
    try:
        runs = cc.run_chained(b, name, nperseg, links, fmt, present, pipelined, before_call, after_fetch)
    finally:
        b.close()
    print(f"\n{what}: {sq.trace(runs)}")
    p = _handle(R, name, nperseg, plain_mode or mode, fmt, min_hops, **extra)
    try:
        plain = cc.run_plain(p, name, nperseg, fmt, present, before_buffer)
    finally:
        p.close()
    _equal(runs, plain, links, what)
    n_neg = sum(int((rec["start"] < 0).sum()) for rec, _ in runs)
    assert n_neg >= 2 * len(runs), (what, n_neg)
    if expect_mode is not None:
        assert all(i.mode_used == expect_mode for _, i in runs), sq.trace(runs)
    if oracle and present is None:
        form = form_of(nperseg, sq.WINDOW, extra.get("subtract_first", False), fmt == "u8")
        n_rec, n_neg = sq.hold_sequence(plain, name, nperseg, fmt, events, min_hops, form, None, None, what, S=R)
        assert n_rec > len(plain) and n_neg > len(plain) // 2, (n_rec, n_neg)
    return runs, plain


# ---- every scan family and level, at the smallest shape ---------------------------------------------------------------------------
def test_auto_schedule_a_links_4():
    """R = 2, links = 4 (S = 8), five calls of schedule A's lengths: another T every call, 33 < K, T = 2"""
    _case("A", 4, 256, "auto")


def test_links_3():
    """S = 6: no power of two"""
    _case("A", 3, 256, "auto")


LEVELS = [("sparse", _native.RT_MODE_SPARSE, {}), ("dense", _native.RT_MODE_DENSE, {}),
          ("runfilter", _native.RT_MODE_RUNFILTER, {})]


@pytest.mark.parametrize("mode,expect,extra", LEVELS, ids=[m for m, _, _ in LEVELS])
def test_levels_at_256(mode, expect, extra):
    _case("P", 4, 256, mode, expect_mode=expect, **extra)


def test_auto_levels_up_on_a_noisy_call_and_keeps_the_chain():
    """Calls 2 and 3 carry schedule C's raised noise floors: the sparse lists overflow, rt_fetch analyses the call again one level up
    -- the re-scan rewrites the look-back columns, chain_tails copies them again in front of the new detection."""
    runs, _ = _case("Pn", 4, 256, "auto", min_hops=sq.C_MIN_HOPS, hot_capacity=128)
    assert any(i.fell_back for _, i in runs), sq.trace(runs)


# nperseg 64 (QS form), 1024 (persistent grid), 4096 (stft_scan64), 8192 (stft_wg), 300 (the dense general path)
@pytest.mark.parametrize("nperseg", [64, 1024, 4096, 8192, 300])
def test_scan_families(nperseg):
    _case("P", 4, nperseg, "auto")


@pytest.mark.parametrize("fmt", ["u8", "i16"])
def test_wire_formats(fmt):
    _case("P", 4, 256, "auto", fmt)


def test_subtract_first():
    """RT_FLAG_NO_LIN_DETREND: the form a stream takes once the detrend guard has marked it, from the start on both handles"""
    _case("P", 4, 256, "auto", subtract_first=True)


def test_two_calls_in_flight():
    serial, _ = _case("P", 4, 256, "auto", oracle=False)
    piped, _ = _case("P", 4, 256, "auto", pipelined=True)
    for c, ((a, _), (b, _)) in enumerate(zip(serial, piped)):
        assert a.tobytes() == b.tobytes(), f"call {c}"


def test_row_means_and_record_cells():
    links, nperseg = 4, 256
    chained, plain = {}, {}

    def keep(store):
        def after(b, c, rec):
            store[c] = (b.fetch_row_means(), b.fetch_record_cells(), rec)
        return after

    name = cc.schedule("P", links)
    what = "side outputs"
    b = _chained(name, nperseg, links, "auto", row_means=True, record_cells=True)
    try:
        runs = cc.run_chained(b, name, nperseg, links, after_fetch=keep(chained))
    finally:
        b.close()
    p = _handle(R, name, nperseg, "auto", row_means=True, record_cells=True)
    try:
        pruns = []
        for k in range(len(sq.SCHEDULES[name].T)):
            sq.enqueue(p, cc.feed_of(name, nperseg, k, "c64"), "c64")
            rec = p.fetch_records()
            pruns.append((rec, p.native.call_info()))
            keep(plain)(p, k, rec)
    finally:
        p.close()
    _equal(runs, pruns, links, what)
    n_back = 0
    for c, (rm, (off, cells), rec) in chained.items():
        assert rm.shape == (R * links, nperseg)
        for j in range(links):
            prm, (poff, pcells), prec = plain[c * links + j]
            for r in range(R):
                assert rm[r * links + j].tobytes() == prm[r].tobytes(), f"{what}: row means of call {c} link {j} recording {r}"
            idx = np.flatnonzero(rec["stream"] % links == j)
            assert len(idx) == len(prec)
            for i, q in zip(idx, range(len(prec))):
                mine, want = cells[off[i]:off[i + 1]], pcells[poff[q]:poff[q + 1]]
                assert mine.tobytes() == want.tobytes(), f"{what}: cells of call {c} link {j} record {rec[i]}"
                assert np.float32(mine.max()) == rec[i]["max_p"]
                n_back += int(rec[i]["start"] < 0)
    assert n_back >= 8  # (cells gathered through the chained look-back among them)


# ---- masks: the rows of absent buffers poisoned -----------------------------------------------------------------------------------
def _present(name, holes):
    p = np.ones((len(sq.SCHEDULES[name].T), R), bool)
    for k, r in holes:
        p[k, r] = False
    return p


def test_suffix_mask_last_call_with_2_of_4_links():
    name = cc.schedule("P", 4)
    _case("P", 4, 256, "auto", present=_present(name, [(18, 0), (19, 0), (18, 1), (19, 1)]))


def test_hole_mask_link_2_follows_link_0():
    name = cc.schedule("P", 4)
    # link 1 absent in calls 1 and 2 of recording 0, in call 3 of recording 1; recording 1 has one buffer fewer at its end
    _case("P", 4, 256, "auto", present=_present(name, [(5, 0), (9, 0), (13, 1), (19, 1)]))


def test_run_absent_for_four_calls():
    name = cc.schedule("P7", 4)
    holes = [(k, 1) for k in range(4, 20)]  # recording 1 sits out calls 1 ... 4 and finds call 0's last link in call 5
    runs, _ = _case("P7", 4, 256, "auto", present=_present(name, holes))
    back = runs[5][0]
    assert ((back["stream"] == 4) & (back["start"] < 0)).any(), "no reach-back across the four absent calls"


# ---- cuts -------------------------------------------------------------------------------------------------------------------------
def test_reset_stream_on_a_middle_link():
    """rt_reset_stream(r * links + 2) before call 2 is a cut in front of buffer 10 of recording r; link 3 chains on"""
    links = 4

    def before_call(b, c):
        if c == 2:
            b.reset_stream(1 * links + 2)

    def before_buffer(p, k):
        if k == 2 * links + 2:
            p.reset_stream(1)

    _case("P", links, 256, "auto", events=(("reset", 2 * links + 2, 1),), before_call=before_call, before_buffer=before_buffer)


def test_threshold_change_for_a_whole_run_between_calls():
    """A changed threshold restarts every stream index it changes: on the chained handle every link of run 1 in call 2 starts without
    look-back (the yardstick: the change before buffer 8, rt_reset_stream before buffers 9 ... 11)."""
    links = 4
    thr = np.float32(10.0 ** (-88.0 / 10.0))

    def before_call(b, c):
        if c == 2:
            v = np.full(R * links, np.float32(10.0 ** (-90.0 / 10.0)), np.float32)
            v[links:] = thr
            b.native.set_stream_params(v, None)

    def before_buffer(p, k):
        if k == 2 * links:
            p.native.set_stream_params(np.array([10.0 ** (-90.0 / 10.0), thr], np.float32), None)
        elif 2 * links < k < 3 * links:
            p.reset_stream(1)

    _case("P", links, 256, "auto", oracle=False, before_call=before_call, before_buffer=before_buffer)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_undisturbed():
    links, nperseg = 4, 256
    name = cc.schedule("P", links)
    S = R * links
    seen = []

    def refuse(b, c):
        nat = b.native
        if c == 1:
            v = np.full(S, np.float32(1e-9), np.float32)
            v[links + 1] = np.float32(2e-9)
            with pytest.raises(_native.NativeError, match="run 1") as e:
                nat.set_stream_params(v, None)
            assert e.value.code == _native.RT_E_INVALID
            snr = np.full(S, np.float32(2.0), np.float32)
            snr[2] = np.float32(3.0)
            with pytest.raises(_native.NativeError, match="run 0"):
                nat.set_stream_settings(snr, None, None)
            with pytest.raises(_native.NativeError, match="does not divide") as e:
                nat.set_chain(3)
            assert e.value.code == _native.RT_E_INVALID
            with pytest.raises(_native.NativeError):
                nat.set_chain(-1)
            seen.append("args")

    def pending(b, c, rec):
        if c == 2:  # a call in flight: refused, and the call still delivers what the twin's does
            nat = b.native
            nat.process_host(cc.chained_feed(name, nperseg, 3, links, "c64"))
            with pytest.raises(_native.NativeError, match="pending") as e:
                nat.set_chain(2)
            assert e.value.code == _native.RT_E_INVALID
            extra = b.fetch_records()
            seen.append(extra)

    b = _chained(name, nperseg, links, "auto")
    try:
        runs = cc.run_chained(b, name, nperseg, links, before_call=refuse, after_fetch=pending)
    finally:
        b.close()
    t = _chained(name, nperseg, links, "auto")
    try:
        t.native.set_chain(links)  # (the value it has: nothing happens)
        twin = []
        for c in range(cc.n_calls("P")):
            t.native.process_host(cc.chained_feed(name, nperseg, c, links, "c64"))
            twin.append(t.fetch_records())
            if c == 2:  # the refused handle analysed call 3 twice: once in flight under the refusal, once in its turn
                t.native.process_host(cc.chained_feed(name, nperseg, 3, links, "c64"))
                extra = t.fetch_records()
    finally:
        t.close()
    assert seen[0] == "args" and seen[1].tobytes() == extra.tobytes()
    for c, ((rec, _), want) in enumerate(zip(runs, twin)):
        assert rec.tobytes() == want.tobytes(), f"call {c} after a refusal"


@pytest.mark.parametrize("kind", ["lanes", "float64"])
def test_unsupported_handles_refuse_and_go_on(kind):
    nperseg, links = 256, 4
    name = cc.schedule("P", links)
    extra = dict(lanes=2) if kind == "lanes" else dict(precision="float64")
    mode = "auto"
    fmt = "c64" if kind == "lanes" else "c128"

    def records(refuse):
        b = _handle(R * links, name, nperseg, mode, fmt, **extra)
        try:
            out = []
            for c in range(2):
                if refuse and c == 1:
                    with pytest.raises(_native.NativeError) as e:
                        b.native.set_chain(links)
                    assert e.value.code == _native.RT_E_UNSUPPORTED
                feed = cc.chained_feed(name, nperseg, c, links, "c64")
                b.enqueue(feed.astype(np.complex128) if kind == "float64" else feed)
                out.append(b.fetch_records())
            return out
        finally:
            b.close()

    for a, w in zip(records(True), records(False)):
        assert a.tobytes() == w.tobytes()


# ---- the Python layer -------------------------------------------------------------------------------------------------------------
def _same_signals(a, b):
    fields = ("device", "ts", "frequency", "duration", "max", "avg", "std", "noise", "snr")
    assert len(a) == len(b), (len(a), len(b))
    for x, y in zip(a, b):
        assert all(getattr(x, f) == getattr(y, f) for f in fields), (vars(x), vars(y))


def _recording(nperseg, n_samples):
    """One array: the first buffers of stream 0 of schedule B (96 segments each, tones across every boundary), joined and cut"""
    return np.concatenate([sq.buffer(sq.SCHEDULES["B"], nperseg, k, 1)[0] for k in range(5)])[:n_samples]


def test_replay_equals_process_samples_called_five_times():
    nperseg, B = 256, 96 * 256
    x = _recording(nperseg, 4 * B + B // 2)
    kw = dict(sq.case_settings(nperseg), sdr_callback_length=B)
    ts0 = datetime.datetime.now()

    class Q(list):
        put = list.append

    a = SignalAnalyzer("0", signal_queue=Q(), **kw)
    got = a.replay(x, ts0, chain=3)  # calls of 3 buffers, of 1 (fewer links), and of the half buffer that is left
    ref = SignalAnalyzer("0", signal_queue=Q(), **kw)
    ref._ts = ts0
    ref.last_data_ts.value = 1.0
    for k in range(5):
        ref.process_samples(x[k * B:(k + 1) * B])
    want = [s for s in ref.signal_queue if hasattr(s, "frequency")]
    assert len(want) >= 3  # (what the shadow filter leaves of five buffers' tones)
    _same_signals(got, want)
    _same_signals([s for s in a.signal_queue if hasattr(s, "frequency")], want)
    a._replay_batch.close()


def test_process_batch_of_a_chained_analyzer():
    """[R, l * B] through ``BatchSignalAnalyzer(chain=4)`` with l = 4, then l = 2 (the suffix mask), against R plain analyzers"""
    nperseg, B, L = 256, 96 * 256, 4
    sched = sq.SCHEDULES["B"]
    bufs = [sq.buffer(sched, nperseg, k, R) for k in range(6)]
    kw = dict(sq.case_settings(nperseg), sdr_callback_length=B, segs_per_chunk=4)
    ts0 = datetime.datetime(2024, 5, 1, 12, 0, 0)
    step = datetime.timedelta(seconds=B / sq.FS)
    ch = BatchSignalAnalyzer(["a", "b"], chain=L, **kw)
    plain = BatchSignalAnalyzer(["a", "b"], **kw)
    try:
        first = ch.process_batch(np.concatenate(bufs[:4], axis=1), ts0, filtered=False, lazy=False)
        second = ch.process_batch(np.concatenate(bufs[4:], axis=1), [ts0 + 4 * step] * R, filtered=False, lazy=False)
        want = [[], []]
        for k in range(6):
            for r, sigs in enumerate(plain.process_batch(bufs[k], ts0 + k * step, filtered=False, lazy=False)):
                want[r].extend(sigs)
        for r in range(R):
            _same_signals(list(first[r]) + list(second[r]), want[r])
            assert len(want[r]) > 10
    finally:
        ch.close()
        plain.close()
