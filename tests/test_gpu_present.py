"""Streams that sit out a call, on the GPU (``rt_set_present``): one handle per case, every call of a schedule of
tests/sequence_cases.py through it under the presence table of tests/present_cases.py, the rows of absent streams poisoned.

In every case: a present stream equals the gapped oracle on every call (identity and shadow verdicts exactly, the float fields
within the precision64 model -- ``sequence_cases.hold_sequence``'s rules, unchanged); an absent stream delivers nothing; and stream
0's records are byte for byte those of a twin handle on which the entry was never called, fed the same buffers -- its other streams
see the poison; streams are independent.  tests/test_present_contract.py shows on the CPU that every pattern holds reach-back records
across gaps of one, two and three or more absent calls, and that the two wrong models of an absent stream fail.

``-s`` prints per case the trace ``call:mode_used/fell_back/dense streams/records``."""
import datetime

import numpy as np
import pytest

from pyradiotracking_amd import _native
from pyradiotracking_amd.analyze import BatchSignalAnalyzer
from tests import present_cases as pc
from tests import sequence_cases as sq
from tests import test_gpu_record_cells as trc
from tests import test_gpu_row_means as trm
from tests.test_gpu_float64 import form_of
from tests.test_gpu_float64_path import DB_TOL as F64_DB_TOL, STD_TOL as F64_STD_TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _need_gpu():
    if _native.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")


def _handle(name, nperseg, mode, fmt="c64", min_hops=sq.MIN_HOPS, **extra):
    sched = sq.SCHEDULES[name]
    if fmt in ("c128", "u8f64"):
        extra["precision"] = "float64"
    return BatchSignalAnalyzer([str(i) for i in range(sq.n_streams(nperseg))], sdr_callback_length=sq.max_samples(sched, nperseg), mode=mode,
                               **sq.case_settings(nperseg, fmt, min_hops=min_hops), **extra)


def _twin_mode(mode, fmt):
    """The twin sees the poison: NaN rows fill its candidate lists, which a handle pinned to a sparse level refuses
    (RT_E_HOT_OVERFLOW) -- it runs on AUTO, whose levels deliver the same records bit for bit."""
    return "auto" if mode in ("sparse", "prefilter", "runfilter") else mode


def _case(name, nperseg, mode, fmt="c64", min_hops=sq.MIN_HOPS, events=(), pipelined=False, before_call=None, after_fetch=None, expect_mode=None,
          twin=True, **extra):
    """One handle under the presence table, the whole schedule, every call and stream against the gapped oracle; then the twin."""
    sched = sq.SCHEDULES[name]
    what = f"present {name} nperseg {nperseg} {mode} {fmt} {extra}"
    b = _handle(name, nperseg, mode, fmt, min_hops, **extra)
    try:
        runs = pc.run_handle(b, name, nperseg, fmt, pipelined=pipelined, before_call=before_call and (lambda k: before_call(b, k)),
                             after_fetch=after_fetch and (lambda k, rec: after_fetch(b, k, rec)))
    finally:
        b.close()
    print(f"\n{what}: {sq.trace(runs)}")
    f64 = fmt in ("c128", "u8f64")
    form = form_of(nperseg, sq.WINDOW, extra.get("subtract_first", False), fmt == "u8")
    n_rec, n_neg, n_gap = pc.hold_sequence(runs, name, nperseg, fmt, events, min_hops, form, (F64_DB_TOL, F64_STD_TOL) if f64 else None, None, what)
    assert n_rec > len(sched.T) and n_neg > len(sched.T) // 2 and n_gap >= 3, (n_rec, n_neg, n_gap)
    if expect_mode is not None:
        assert all(i.mode_used == expect_mode for (r, i), t in zip(runs, sched.T) if t > 0), sq.trace(runs)
    if twin:
        t = _handle(name, nperseg, _twin_mode(mode, fmt), fmt, min_hops, **extra)
        try:
            plain = pc.run_handle(t, name, nperseg, fmt, before_call=before_call and (lambda k: before_call(t, k)), masked=False)
        finally:
            t.close()
        present = pc.table(name, sq.n_streams(nperseg))
        # (up to the one call every stream sits out: from there on the twin's stream 0 has analysed a poisoned buffer the masked
        # handle's never saw, and looks back into it)
        first_absent = int(np.flatnonzero(~present[:, 0])[0]) if not present[:, 0].all() else len(runs)
        assert first_absent >= 8
        for k, ((a, _), (p, _)) in enumerate(zip(runs, plain)):
            if k < first_absent:
                assert a[a["stream"] == 0].tobytes() == p[p["stream"] == 0].tobytes(), f"{what} call {k}: stream 0 differs from the handle without a mask"
    return runs


# every scan family, sparse: stft_scan (128, 256, 1024), stft_scan64 (4096), stft_wg (8192)
@pytest.mark.parametrize("nperseg", [128, 256, 1024, 4096, 8192])
def test_sparse(nperseg):
    _case("A", nperseg, "sparse", expect_mode=_native.RT_MODE_SPARSE)


# dense: the scans' MODE 1 (256), stft_general (16), stft_bluestein (300)
DENSE = [(256, "dense"), (16, "auto"), (300, "auto")]


@pytest.mark.parametrize("nperseg,mode", DENSE)
def test_dense(nperseg, mode):
    _case("A", nperseg, mode, expect_mode=_native.RT_MODE_DENSE if mode == "dense" else None)


# the float64 path (stft_f64), from complex128 and from wire bytes
@pytest.mark.parametrize("fmt", ["c128", "u8f64"])
def test_float64(fmt):
    _case("A", 256, "auto", fmt)


# the wire formats (absent rows: a full-scale tone)
@pytest.mark.parametrize("fmt", ["u8", "i16", "i8"])
def test_wire_formats(fmt):
    _case("A", 256, "sparse", fmt)


# lanes (every lane takes its slice of the mask) and the one-wave-per-stream detection
LANES = [dict(lanes=2), dict(lanes=3), dict(group_detect=True)]


@pytest.mark.parametrize("extra", LANES, ids=["-".join(f"{k}{v}" for k, v in e.items()) for e in LANES])
def test_lanes_and_detection_form(extra):
    _case("A", 256, "sparse", **extra)


# two calls in flight, the mask changed between the two enqueues: each call keeps the mask it was enqueued with
@pytest.mark.parametrize("nperseg", [256, 4096])
def test_pipelined_equals_serial(nperseg):
    serial = _case("A", nperseg, "sparse", twin=False)
    piped = _case("A", nperseg, "sparse", pipelined=True)  # (with its twin: a snapshot mixed up between the two calls in flight would show in stream 0)
    for k, ((a, _), (b, _)) in enumerate(zip(serial, piped)):
        assert a.tobytes() == b.tobytes(), f"call {k}"


# the chunk-bit pre-filter pinned (its own condition: segs_per_chunk 4, a minimum of 8 hops, runs of at least 10 segments)
def test_prefilter():
    _case("B10", 256, "prefilter", min_hops=8.0, expect_mode=_native.RT_MODE_PREFILTER, segs_per_chunk=4)


# the exact pre-filter pinned, and AUTO, over the noise regimes of schedule C, stream 1 absent through the noisy calls: its
# thresholds behind the gap come from an older buffer of its own and are held by check_bin_thresholds
def test_runfilter_over_noise_regimes():
    _case("C", 256, "runfilter", min_hops=sq.C_MIN_HOPS, expect_mode=_native.RT_MODE_RUNFILTER, hot_capacity=16384)


def test_auto_over_noise_regimes():
    runs = _case("C", 256, "auto", min_hops=sq.C_MIN_HOPS, segs_per_chunk=4, hot_capacity=512)
    assert any(i.fell_back for _, i in runs), sq.trace(runs)


# side outputs
@pytest.mark.parametrize("nperseg", [256, 4096])
def test_side_outputs(nperseg):
    """rt_fetch_row_means: NaN rows for absent streams, ``r.row_mean`` bit for bit for present ones; rt_fetch_record_cells:
    ``max(cells) == max_p`` for every record, reach-backs across a gap among them."""
    S = sq.n_streams(nperseg)
    present = pc.table("A", S)
    sched = sq.SCHEDULES["A"]
    last_present = [None] * S
    n_gap_cells = [0]

    def after_fetch(b, k, rec):
        rm = b.fetch_row_means()
        off, cells = b.fetch_record_cells()
        assert rm.shape == (S, nperseg) and rm.dtype == np.float32
        assert len(off) == len(rec) + 1 and np.array_equal(np.diff(off), rec["end"] - rec["start"]) and len(cells) == off[-1]
        for s in range(S):
            if not present[k, s] or sched.T[k] == 0:
                assert np.isnan(rm[s]).all(), f"call {k} stream {s}: row means of an absent stream"
            else:
                assert not np.isnan(rm[s]).any(), f"call {k} stream {s}"
        if len(rec):
            trm._check_records_bits(rec, rm, nperseg, f"call {k}")
        for r, o0, o1 in zip(rec, off[:-1], off[1:]):
            c = cells[o0:o1]
            assert np.float32(c.max()) == r["max_p"], f"call {k} record {r}: max(cells) {c.max()!r}"
            s = int(r["stream"])
            if r["start"] < 0 and last_present[s] is not None and k - last_present[s] > 1:
                n_gap_cells[0] += 1
        for s in range(S):
            if present[k, s]:
                last_present[s] = k

    _case("A", nperseg, "sparse", after_fetch=after_fetch, row_means=True, record_cells=True, twin=False)
    assert n_gap_cells[0] >= 3


# the detrend guard under a mask
@pytest.mark.parametrize("nperseg", [256, 4096])
def test_detrend_guard_under_a_mask_with_two_calls_in_flight(nperseg):
    """Stream 1 carries a DC offset 80 dB over its noise from call 1 on, so the guard of the linearity form marks it when call 1 is
    fetched -- with call 2, which stream 1 sits out, already enqueued.  rt_fetch analyses call 1 again (stream 1 now on the
    subtract-first launch: the mask rows are split anew), carries stream 1's rewritten look-back columns into call 2's buffer again
    and analyses call 2 again.  Pipelined on device buffers against the same masked calls made one at a time: the same bytes;
    the runs are those of a masked handle that was subtract-first from the start; absent streams deliver nothing; and stream 1's
    pulse across its gap (calls 1 -> 3) is one record that starts in its buffer of call 1."""
    from oracle import analyze_oracle as oracle
    from pyradiotracking_amd import synth

    fs, n, S = 2048000, 24 * 4096, 3
    w = oracle.window_coefficients("hamming", nperseg)
    rng = np.random.default_rng(nperseg + 7)
    present = np.ones((5, S), bool)
    present[2, 1] = False  # (in flight while the guard re-analyses call 1)
    present[1, 2] = False
    present[3, 0] = False
    amp = synth.amp_for_peak_dbw(-55.0, w, fs)
    f_gap = 0.2 * fs
    bufs = []
    for k in range(5):
        rows = []
        for s in range(S):
            pulses = synth.random_pulses(rng, n, fs, w, 3, dur_ms=(3, 9), peak_dbw=(-80.0, -60.0))
            if s == 1 and k == 1:
                pulses.append(synth.Pulse(n - int(0.004 * fs), int(0.004 * fs), f_gap, amp, 0.5))
            if s == 1 and k == 3:
                pulses.append(synth.Pulse(0, int(0.004 * fs), f_gap, amp, 0.5))
            dc = complex(0.1, -0.07) if (s == 1 and k >= 1) else 0j
            rows.append(synth.make_stream(synth.StreamSpec(n, fs, pulses, noise_sigma=1e-5, dc=dc), 700 + 10 * k + s))
        x = np.stack(rows)
        x[~present[k]] = np.nan + 1j * np.nan
        bufs.append(x)
    kw = dict(sample_rate=fs, fft_nperseg=nperseg, fft_window="hamming", signal_min_duration_ms=2, signal_threshold_dbw=-90.0)

    def handle(**extra):
        return BatchSignalAnalyzer([str(i) for i in range(S)], sdr_callback_length=n, mode="sparse", **kw, **extra)

    serial, first, piped = handle(), handle(subtract_first=True), handle()
    try:
        want, ref = [], []
        for k, buf in enumerate(bufs):
            for b, out in ((serial, want), (first, ref)):
                b.set_present(present[k])
                b.enqueue(buf)
                out.append(b.fetch_records())
        devs = []
        for buf in bufs:
            d = _native.DeviceBuffer(0, buf.nbytes)
            d.upload(buf)
            devs.append(d)
        got = []
        piped.set_present(present[0])
        piped.enqueue(devs[0].ptr, n_samples=n)
        for k in range(len(bufs)):
            if k + 1 < len(bufs):
                piped.set_present(present[k + 1])
                piped.enqueue(devs[k + 1].ptr, n_samples=n)
            got.append(piped.fetch_records())
    finally:
        for b in (serial, first, piped):
            b.close()
    key = lambda a: [(int(v["stream"]), int(v["fi"]), int(v["start"]), int(v["end"])) for v in a]
    for k, (g, x, r) in enumerate(zip(got, want, ref)):
        assert g.tobytes() == x.tobytes(), (nperseg, k)
        assert not np.isin(g["stream"], np.flatnonzero(~present[k])).any(), (nperseg, k)
        if k >= 1:  # (a clean buffer analysed in the linearity form may differ from subtract-first by an ulp at a threshold)
            assert key(g) == key(r), (nperseg, k)
    across = got[3][(got[3]["stream"] == 1) & (got[3]["start"] < 0)]
    assert len(across) >= 1 and sum(len(g) for g in got) > 8, (key(got[3]), [len(g) for g in got])


# stream events issued while their stream is absent (the events of test_gpu_sequences.test_stream_events_in_mid_sequence: stream 1
# sits out call 5, stream 2 calls 5 .. 7)
EVENTS = (("reset", 5, 1), ("snr", 7, 2, 6.0))


@pytest.mark.parametrize("mode", ["sparse", "dense"])
def test_events_while_absent_take_effect_at_the_next_present_call(mode):
    present = pc.table("A")
    assert not present[5, 1] and present[6, 1] and not present[7, 2] and present[8, 2]

    def before_call(b, k):
        if k == 5:
            b.reset_stream(1)
        if k == 7:
            snr = [sq.SNR_DB] * sq.n_streams(256)
            snr[2] = 6.0
            b.set_stream_settings(snr_threshold_db=snr)

    runs = _case("A", 256, mode, events=EVENTS, before_call=before_call)
    # the events took something away: without them these streams reach back across their gaps at calls 6 and 8
    plain = pc.oracle_run("A", 256)
    with_events = pc.oracle_run("A", 256, "c64", EVENTS)
    assert any(r.start < 0 for r in plain[6][1].records) and not (runs[6][0][runs[6][0]["stream"] == 1]["start"] < 0).any()
    assert not any(r.start < 0 for r in with_events[8][2].records)
    for s in (0, 3, 4):
        assert all(plain[k][s] is None or sq.key(plain[k][s].records) == sq.key(with_events[k][s].records) for k in range(len(plain)))


# BatchRunner(skip_absent=True)
T0 = 1700000000.0


class _Q:
    def __init__(self):
        self.items = []

    def put(self, m):
        self.items.append(m)


def _runner_streams():
    from oracle import analyze_oracle as oracle
    from pyradiotracking_amd import synth

    fs, nperseg = 2048000, 256
    blen, n_buf = 400 * nperseg, 6
    w = oracle.window_coefficients("hamming", nperseg)
    rng = np.random.default_rng(12)
    iq = []
    for s in range(4):
        pulses = synth.random_pulses(rng, n_buf * blen, fs, w, 30, dur_ms=(9, 30), peak_dbw=(-95.0, -70.0))
        for k in range(1, n_buf):  # a pulse across every buffer boundary of the stream's own sample sequence
            pulses.append(synth.Pulse(k * blen - int(0.006 * fs), int(0.015 * fs), (0.1 + 0.07 * s) * fs, synth.amp_for_peak_dbw(-66.0, w, fs), 0.5))
        iq.append(synth.make_stream(synth.StreamSpec(n_buf * blen, fs, pulses), 60 + s))
    return fs, nperseg, blen, n_buf, np.stack(iq)


# (one absence per SDR: every missed step adds a buffer length to its clock drift, and more than two are fatal, analyze.py:226-229)
RUNNER_PRESENT = {1: [True, True, False, True], 2: [False, True, True, True], 3: [True, False, True, False]}


@pytest.mark.parametrize("tensor", [False, True], ids=["host", "device-tensor"])
def test_runner_skip_absent_matches_per_sdr_oracles(tensor):
    """Four SDRs, each absent from one step: with ``skip_absent=True`` every SDR's buffers are contiguous in ITS samples, and every
    published Signal equals what a per-SDR reference analyzer that was simply not called in that step produces -- the pulse across
    the boundary around the gap included.  The absent rows hold NaN."""
    from oracle import analyze_oracle as oracle
    from pyradiotracking_amd import Signal
    from pyradiotracking_amd.runner import BatchRunner

    fs, nperseg, blen, n_buf, iq = _runner_streams()
    kw = dict(sample_rate=fs, fft_nperseg=nperseg)
    q = _Q()
    r = BatchRunner(device=["0", "1", "2", "3"], gpus=[0], sdr_timeout_s=100, signal_queue=q, sdr_callback_length=blen, skip_absent=True, **kw)
    r.start_analyzers()
    oas = [oracle.OracleAnalyzer(device=str(s), **kw) for s in range(4)]
    dt = blen / fs
    nxt = [0] * 4  # each SDR's next buffer of its own sequence
    clocks = [None] * 4
    want = []
    n_across = 0
    for k in range(n_buf):
        now = T0 + k * dt
        pres = RUNNER_PRESENT.get(k, [True] * 4)
        chunk = np.full((4, blen), np.nan + 1j * np.nan, np.complex64)
        for s in range(4):
            if not pres[s]:
                continue
            chunk[s] = iq[s, nxt[s] * blen:(nxt[s] + 1) * blen]
            nxt[s] += 1
            recv = datetime.datetime.fromtimestamp(now)
            clocks[s] = recv if clocks[s] is None else clocks[s] + datetime.timedelta(seconds=dt)
            sigs, kept = oas[s].process(chunk[s], clocks[s] - datetime.timedelta(seconds=dt))
            want += kept
            if k > 0 and not RUNNER_PRESENT.get(k - 1, [True] * 4)[s]:
                start = clocks[s] - datetime.timedelta(seconds=dt)
                n_across += sum(1 for x in kept if x.ts.timestamp() < start.timestamp())  # (a Signal's ts is UTC, the clock naive local time)
        if tensor:
            import torch

            r.process({0: torch.from_numpy(chunk).cuda()}, present=pres, now=now)
        else:
            r.process(chunk, present=pres, now=now)
    got = [m for m in q.items if isinstance(m, Signal)]
    assert len(got) == len(want) > 20 and n_across >= 3, (len(got), len(want), n_across)
    for g, x in zip(got, want):
        assert (g.device, g.ts, g.duration, g.frequency) == (x.device, x.ts, x.duration, x.frequency)
        for name in ("max", "avg", "noise", "snr", "std"):
            assert abs(getattr(g, name) - getattr(x, name)) < 0.01
    assert all(st.alive and not st.stale and st.restarts == 0 for st in r.streams)
    r.stop_analyzers()


def test_runner_without_skip_absent_is_unchanged():
    """The same station in lock-step with the default ``skip_absent=False``: an absent SDR's row is analysed as zeros and its next
    buffer starts without look-back -- the per-SDR oracles are reset at those points, as in tests/test_runner.py."""
    from oracle import analyze_oracle as oracle
    from pyradiotracking_amd import Signal
    from pyradiotracking_amd.runner import BatchRunner

    fs, nperseg, blen, n_buf, iq = _runner_streams()
    kw = dict(sample_rate=fs, fft_nperseg=nperseg)
    q = _Q()
    r = BatchRunner(device=["0", "1", "2", "3"], gpus=[0], sdr_timeout_s=100, signal_queue=q, sdr_callback_length=blen, **kw)
    r.start_analyzers()
    oas = [oracle.OracleAnalyzer(device=str(s), **kw) for s in range(4)]
    dt = blen / fs
    clocks = [None] * 4
    want = []
    for k in range(n_buf):
        now = T0 + k * dt
        pres = RUNNER_PRESENT.get(k, [True] * 4)
        chunk = np.ascontiguousarray(iq[:, k * blen:(k + 1) * blen])
        for s in range(4):
            if not pres[s]:
                continue
            if k > 0 and not RUNNER_PRESENT.get(k - 1, [True] * 4)[s]:
                oas[s].reset()
            recv = datetime.datetime.fromtimestamp(now)
            clocks[s] = recv if clocks[s] is None else clocks[s] + datetime.timedelta(seconds=dt)
            want += oas[s].process(chunk[s], clocks[s] - datetime.timedelta(seconds=dt))[1]
        r.process(chunk, present=pres, now=now)
    got = [m for m in q.items if isinstance(m, Signal)]
    assert len(got) == len(want) > 20
    for g, x in zip(got, want):
        assert (g.device, g.ts, g.duration, g.frequency) == (x.device, x.ts, x.duration, x.frequency)
    r.stop_analyzers()


def oracle_keys():
    """Every (schedule, nperseg, format, events, minimum) the cases above ask the gapped oracle for (tests/test_present_contract.py
    runs them all on the CPU)."""
    keys = [("A", n, "c64", (), sq.MIN_HOPS) for n in (128, 256, 1024, 4096, 8192)] + [("A", n, "c64", (), sq.MIN_HOPS) for n, _ in DENSE]
    keys += [("A", 256, f, (), sq.MIN_HOPS) for f in ("c128", "u8f64", "u8", "i16", "i8")]
    keys += [("B10", 256, "c64", (), 8.0), ("C", 256, "c64", (), sq.C_MIN_HOPS), ("A", 256, "c64", EVENTS, sq.MIN_HOPS)]
    return sorted(set(keys), key=str)
