"""Per-stream detection settings (rt_set_stream_settings[_f64]) on the GPU.  Every stream of a batch gets the SAME IQ
(tests/stream_settings_cases.py), so only the settings can make the streams' records differ; the ground truth is one
OracleAnalyzer per stream, built with that stream's keywords.  Comparison and tolerances are those of tests/test_gpu_parity.py
(float32) and tests/test_gpu_float64_path.py (float64 handles)."""
import numpy as np
import pytest

from oracle import analyze_oracle as oracle
from pyradiotracking_amd import Signal, _native, synth
from pyradiotracking_amd.analyze import BatchSignalAnalyzer
from pyradiotracking_amd.runner import BatchRunner
from tests import stream_settings_cases as sc
from tests.test_gpu_float64_path import DB_TOL as F64_DB_TOL, STD_TOL as F64_STD_TOL
from tests.test_gpu_parity import POWER_TOL_DB, _need_gpu, _std_tolerance

pytestmark = pytest.mark.gpu

N = len(sc.STREAMS)
DEVICES = [str(i) for i in range(N)]


def _cells(rec):
    return list(zip(rec["fi"].tolist(), rec["start"].tolist(), rec["end"].tolist()))


def _same_iq(buf, n=N):
    return np.ascontiguousarray(np.broadcast_to(buf, (n,) + buf.shape))


def _mixed(nperseg, mode, blen, threshold_shift_db=0.0, **extra):
    return BatchSignalAnalyzer(DEVICES, sdr_callback_length=blen, mode=mode, **sc.batch_kwargs(nperseg, threshold_shift_db), **extra)


def _guard(res, sigma):
    """the oracle's record sets of the settings that were chosen to differ are pairwise different: the comparison below
    cannot pass with the settings ignored"""
    names = sc.DIFFER_QUIET if sigma == sc.SIGMA_QUIET else sc.DIFFER_FLOOR
    sets = {n: tuple(tuple(sc.keys(per[0])) for per in res[sc.NAMES.index(n)]) for n in names}
    for a in names:
        for b in names:
            assert a == b or sets[a] != sets[b], f"the oracle finds the same records with {a} and {b}: the input does not separate them"
    assert any(x.start < 0 for x in res[0][1][0]), "no record of the second buffer reaches back into the first"


def _assert_stream_equals_oracle(b, mine, every, kept, spec, prev, what, f64=False):
    assert [(int(r["fi"]), int(r["start"]), int(r["end"])) for r in mine] == sc.keys(every), what
    kept_ids = {id(x) for x in kept}
    assert [bool(r["shadowed"]) for r in mine] == [id(x) not in kept_ids for x in every], what
    sigs = b._decoder.signals(mine, DEVICES, [sc_ts()] * N)
    for g, x in zip(sigs, every):
        assert g.ts == x.ts and g.duration == x.duration and g.frequency == x.frequency, (what, g, x)
        for name in ("max", "avg", "noise", "snr"):
            assert abs(getattr(g, name) - getattr(x, name)) <= (F64_DB_TOL if f64 else POWER_TOL_DB), (what, name, getattr(g, name), getattr(x, name))
        tol = F64_STD_TOL if f64 else _std_tolerance(x, spec, prev)
        assert abs(g.std - x.std) <= tol, (what, "std", g.std, x.std, tol)


def sc_ts():
    import datetime

    import pytz

    return datetime.datetime(2024, 3, 1, 12, 0, 0, tzinfo=pytz.utc)


def _run_against_oracle(nperseg, sigma, mode, wire="c64", **extra):
    """Both buffers through a mixed handle; every stream against its own OracleAnalyzer."""
    _need_gpu()
    bufs = sc.buffers(nperseg, sigma)
    blen = bufs.shape[1]
    shift, f64 = 0.0, extra.get("precision") == "float64"
    if wire == "u8":
        raw = synth.quantize_u8(bufs, gain=20.0)  # [2, 2 B]; the gain of 20 is 26 dB
        shift = 26.0
        feed = raw
        seen = synth.u8_to_complex64_like_kernel(raw)
    elif f64:
        feed = seen = bufs.astype(np.complex128)
    else:
        feed = seen = bufs
    res = sc.oracle_run(seen, nperseg, threshold_shift_db=shift, ts=sc_ts())
    _guard(res, sigma)
    b = _mixed(nperseg, mode, blen, shift, **extra)
    try:
        assert isinstance(b.snr_threshold, list) and isinstance(b.signal_min_duration, list) and isinstance(b.center_freq, list)
        n_records = 0
        for k in range(2):
            if wire == "u8":
                b.enqueue_bytes(_same_iq(feed[k]))
            else:
                b.enqueue(_same_iq(feed[k]))
            rec = b.fetch_records()
            for s in range(N):
                every, kept, spec, prev = res[s][k]
                mine = rec[rec["stream"] == s]
                print(f"nperseg {nperseg} sigma {sigma} {mode} {wire} buffer {k} {sc.NAMES[s]}: {len(mine)} records, oracle {len(every)}")
                _assert_stream_equals_oracle(b, mine, every, kept, spec, prev, f"nperseg {nperseg} buffer {k} stream {sc.NAMES[s]}", f64)
                n_records += len(mine)
        assert n_records > 2 * N
    finally:
        b.close()


# ---------------------------------------------------------------------------
# 1. against the oracle
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [sc.SIGMA_QUIET, sc.SIGMA_FLOOR])
@pytest.mark.parametrize("nperseg", [128, 256, 1024, 4096, 8192, 300])
def test_mixed_batch_equals_one_oracle_per_stream(nperseg, sigma):
    """Each stream of a batch with eight different settings equals an OracleAnalyzer built with that stream's keywords, over
    two buffers with a pulse across their edge (nperseg 128: detection by groups of lists; 300: Bluestein, dense path)."""
    extra = dict(group_detect=True) if nperseg == 128 else {}
    _run_against_oracle(nperseg, sigma, "auto", **extra)


@pytest.mark.parametrize("mode,sigma,wire,extra", [
    ("sparse", sc.SIGMA_QUIET, "c64", {}),
    ("dense", sc.SIGMA_QUIET, "c64", {}),
    ("dense", sc.SIGMA_FLOOR, "c64", {}),
    ("sparse", sc.SIGMA_QUIET, "c64", dict(lanes=3)),
    ("auto", sc.SIGMA_FLOOR, "c64", dict(lanes=3)),
    ("dense", sc.SIGMA_QUIET, "c64", dict(lanes=3)),
    ("auto", sc.SIGMA_FLOOR, "u8", {}),
    ("auto", sc.SIGMA_FLOOR, "u8", dict(lanes=3)),
    ("auto", sc.SIGMA_QUIET, "c64", dict(precision="float64")),
    ("dense", sc.SIGMA_FLOOR, "c64", dict(precision="float64")),
])
def test_mixed_batch_in_every_mode_lane_split_and_input_format(mode, sigma, wire, extra):
    """The same at nperseg 256 with the mode pinned, with three lanes (every lane takes its slice of the settings), with the
    RTL-SDR wire format, and on a float64 handle with complex128 input against the oracle on complex128."""
    _run_against_oracle(256, sigma, mode, wire, **extra)


# ---------------------------------------------------------------------------
# 2. a stream's result does not depend on its batch
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["sparse", "dense"])
def test_a_streams_records_do_not_depend_on_its_batch(mode):
    """Stream s of the mixed handle is bit for bit stream s of a plain handle -- scalar keywords equal to stream s's settings,
    the new entry never called -- that analyses the same batch."""
    _need_gpu()
    nperseg = 256
    bufs = sc.buffers(nperseg, sc.SIGMA_QUIET)
    blen = bufs.shape[1]
    mixed = _mixed(nperseg, mode, blen)
    got = []
    for k in range(2):
        mixed.enqueue(_same_iq(bufs[k]))
        got.append(mixed.fetch_records())
    mixed.close()
    distinct = set()
    for s in range(N):
        plain = BatchSignalAnalyzer(DEVICES, sdr_callback_length=blen, mode=mode, sample_rate=sc.FS, fft_nperseg=nperseg,
                                    fft_window=sc.WINDOW, **sc.stream_kwargs(s, nperseg))
        assert not isinstance(plain.snr_threshold, list)
        for k in range(2):
            plain.enqueue(_same_iq(bufs[k]))
            rec = plain.fetch_records()
            want, mine = rec[rec["stream"] == s], got[k][got[k]["stream"] == s]
            assert len(want) > 0 and mine.tobytes() == want.tobytes(), (mode, sc.NAMES[s], k, len(mine), len(want))
            distinct.add((k, tuple(_cells(want))))
        plain.close()
    assert len(distinct) >= 2 * len(sc.DIFFER_QUIET)


# ---------------------------------------------------------------------------
# 3. the pre-filters
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("extra,modes", [
    (dict(segs_per_chunk=32), ("runfilter", "auto")),  # chunks as a batch that fills the chip gets them: no chunk-bit level at 8 ms
    ({}, ("prefilter", "runfilter", "auto")),         # a small batch's chunks of 4 segments: the envelope (8 ms = 9.4 hops) allows chunk bits
])
def test_prefilter_levels_equal_dense_with_mixed_settings(extra, modes):
    """Noise floor near the threshold: the pre-filter levels of a mixed handle return its dense path's records byte for byte
    -- the exact pre-filter's per-bin thresholds take each stream's SNR threshold, its run length and the chunk bits the
    envelope's minimum --, also after two streams have exchanged their SNR settings between two calls."""
    _need_gpu()
    nperseg = 256
    bufs = sc.buffers(nperseg, sc.SIGMA_FLOOR)
    blen = bufs.shape[1]
    dense = _mixed(nperseg, "dense", blen, **extra)
    others = {m: _mixed(nperseg, m, blen, **extra) for m in modes}
    i3, i12 = sc.NAMES.index("snr3"), sc.NAMES.index("snr12")
    snr_db = list(sc.batch_kwargs(nperseg)["snr_threshold_db"])
    seen = []
    for k, buf in enumerate((bufs[0], bufs[1], bufs[0], bufs[1])):
        if k == 2:
            snr_db[i3], snr_db[i12] = snr_db[i12], snr_db[i3]
            for b in [dense] + list(others.values()):
                b.set_stream_settings(snr_threshold_db=snr_db)
        for b in [dense] + list(others.values()):
            b.enqueue(_same_iq(buf))
        want = dense.fetch_records()
        assert len(want) > N
        for m, b in others.items():
            got = b.fetch_records()
            info = b.native.call_info()
            print(f"{extra} buffer {k} mode {m}: {len(got)} records, dense {len(want)}, mode_used {info.mode_used}, fell_back {info.fell_back}")
            assert got.tobytes() == want.tobytes(), (extra, k, m, len(got), len(want))
            if m != "auto":
                assert info.mode_used == {"prefilter": _native.RT_MODE_PREFILTER, "runfilter": _native.RT_MODE_RUNFILTER}[m]
        seen.append([_cells(want[want["stream"] == s]) for s in (i3, i12)])
    assert seen[1][0] != seen[1][1]  # the two SNR settings separate on this input ...
    # ... and the exchange took effect: same IQ, same look-back, so each stream now finds what the other found before
    assert seen[3][0] == seen[1][1] and seen[3][1] == seen[1][0]
    for b in [dense] + list(others.values()):
        b.close()


# ---------------------------------------------------------------------------
# 4. no change by default
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode,sigma", [("sparse", sc.SIGMA_QUIET), ("dense", sc.SIGMA_QUIET), ("prefilter", sc.SIGMA_QUIET),
                                        ("runfilter", sc.SIGMA_FLOOR), ("auto", sc.SIGMA_QUIET), ("auto", sc.SIGMA_FLOOR)])
def test_settings_equal_to_the_handles_change_nothing(mode, sigma):
    """Arrays equal to rt_config's values: records, record cells and row means byte-identical to a handle on which the entry
    was never called -- and no stream loses its look-back over a call that changes nothing."""
    _need_gpu()
    nperseg = 256
    bufs = sc.buffers(nperseg, sigma)
    blen = bufs.shape[1]
    kw = dict(sdr_callback_length=blen, mode=mode, sample_rate=sc.FS, fft_nperseg=nperseg, fft_window=sc.WINDOW, record_cells=True, row_means=True)
    never, called = BatchSignalAnalyzer(DEVICES, **kw), BatchSignalAnalyzer(DEVICES, **kw)
    snr = np.full(N, np.float32(called.snr_threshold), np.float32)
    lo, hi = np.full(N, called.signal_min_duration), np.full(N, called.signal_max_duration)
    n_neg = 0
    for k in range(2):
        called.native.set_stream_settings(snr, lo, hi)
        for b in (never, called):
            b.enqueue(_same_iq(bufs[k]))
        want, got = never.fetch_records(), called.fetch_records()
        assert len(want) >= N and got.tobytes() == want.tobytes(), (mode, k, len(got), len(want))
        (wo, wc), (go, gc) = never.fetch_record_cells(), called.fetch_record_cells()
        assert go.tobytes() == wo.tobytes() and gc.tobytes() == wc.tobytes() and len(wc) > 0
        assert called.fetch_row_means().tobytes() == never.fetch_row_means().tobytes()
        n_neg += int((got["start"] < 0).sum())
    assert n_neg >= N  # the edge pulse of every stream reached back
    never.close()
    called.close()


# ---------------------------------------------------------------------------
# 5. change rules
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("precision,lanes", [("float32", 1), ("float32", 3), ("float64", 1)])
def test_a_changed_setting_starts_that_stream_without_look_back(precision, lanes):
    """A stream whose minimum changes between the buffers is a new analyzer in the reference (analyze.py:113, 128): it drops
    the pulse across the edge; every other stream keeps it."""
    _need_gpu()
    nperseg, changed = 256, 2
    bufs = sc.buffers(nperseg, sc.SIGMA_QUIET)
    feed = bufs.astype(np.complex128) if precision == "float64" else bufs
    blen = bufs.shape[1]
    b = BatchSignalAnalyzer(DEVICES, sdr_callback_length=blen, mode="auto", sample_rate=sc.FS, fft_nperseg=nperseg, fft_window=sc.WINDOW,
                            signal_min_duration_ms=[8.0] * N, precision=precision, lanes=lanes)
    b.enqueue(_same_iq(feed[0]))
    b.fetch_records()
    mins = [8.0] * N
    mins[changed] = 9.0
    b.set_stream_settings(signal_min_duration_ms=mins)
    assert b.signal_min_duration[changed] == 9.0 / 1000
    b.enqueue(_same_iq(feed[1]))
    rec = b.fetch_records()
    kw = dict(sample_rate=sc.FS, fft_nperseg=nperseg, fft_window=sc.WINDOW)
    for s in range(N):
        oa = oracle.OracleAnalyzer(device=str(s), signal_min_duration_ms=mins[s], **kw)
        if s != changed:
            oa.process(feed[0], sc_ts())
        want, _ = oa.process(feed[1], sc_ts())
        mine = rec[rec["stream"] == s]
        assert [(int(r["fi"]), int(r["start"]), int(r["end"])) for r in mine] == sc.keys(want), s
        if s == changed:
            assert not (mine["start"] < 0).any()
        else:
            assert (mine["start"] < 0).any()
    b.close()


@pytest.mark.parametrize("precision", ["float32", "float64"])
def test_refused_calls_leave_the_handle_undisturbed(precision):
    """A call pending, a minimum under the envelope, a maximum over it, snr <= 0 and values that are not finite are refused with
    RT_E_INVALID; after each refusal the next buffer's records are those of an undisturbed handle."""
    _need_gpu()
    nperseg = 256
    bufs = sc.buffers(nperseg, sc.SIGMA_QUIET)
    feed = bufs.astype(np.complex128) if precision == "float64" else bufs
    blen = bufs.shape[1]
    kw = dict(sdr_callback_length=blen, mode="auto", precision=precision, **sc.batch_kwargs(nperseg))
    calm, b = BatchSignalAnalyzer(DEVICES, **kw), BatchSignalAnalyzer(DEVICES, **kw)
    sdt = np.float64 if precision == "float64" else np.float32
    ok_snr = np.array(b.snr_threshold, dtype=np.float64).astype(sdt)
    ok_lo, ok_hi = np.array(b.signal_min_duration), np.array(b.signal_max_duration)
    env_lo, env_hi = ok_lo.min(), ok_hi.max()

    def vary(a, i, v):
        a = a.copy()
        a[i] = v
        return a

    refusals = [
        ("pending", None),
        ("min under the envelope", (ok_snr, vary(ok_lo, 5, env_lo * 0.875), ok_hi)),
        ("max over the envelope", (ok_snr, ok_lo, vary(ok_hi, 1, env_hi * 1.025))),
        ("snr zero", (vary(ok_snr, 3, 0.0), ok_lo, ok_hi)),
        ("snr negative", (vary(ok_snr, 7, -2.0), None, None)),
        ("snr not finite", (vary(ok_snr, 0, np.inf), ok_lo, ok_hi)),
        ("min not finite", (None, vary(ok_lo, 4, np.nan), None)),
        ("max not finite", (ok_snr, ok_lo, vary(ok_hi, 6, np.nan))),
    ]
    for h in (calm, b):
        h.enqueue(_same_iq(feed[0]))
        h.fetch_records()
    for k, (what, args) in enumerate(refusals):
        buf = _same_iq(feed[(k + 1) % 2])
        if args is None:
            b.enqueue(buf)
            with pytest.raises(_native.NativeError) as ei:
                b.native.set_stream_settings(ok_snr, ok_lo, ok_hi)
            assert ei.value.code == _native.RT_E_INVALID and "pending" in str(ei.value), what
        else:
            with pytest.raises(_native.NativeError) as ei:
                b.native.set_stream_settings(*args)
            assert ei.value.code == _native.RT_E_INVALID and "stream " in str(ei.value), (what, str(ei.value))
            b.enqueue(buf)
        calm.enqueue(buf)
        got, want = b.fetch_records(), calm.fetch_records()
        assert len(want) > N and got.tobytes() == want.tobytes(), what
        if (k + 1) % 2 == 1:
            assert (got["start"] < 0).any(), what  # (the refused call cost no stream its look-back)
    # the entry of the other precision is refused as well
    other = b.native._lib.rt_set_stream_settings if precision == "float64" else b.native._lib.rt_set_stream_settings_f64
    assert other(b.native._handle, None, None, None) == _native.RT_E_INVALID
    # min > max is accepted, as the reference accepts it: such a stream finds nothing
    b.native.set_stream_settings(None, vary(ok_lo, 0, 0.030), vary(ok_hi, 0, 0.020))
    b.enqueue(_same_iq(feed[0]))
    rec = b.fetch_records()
    assert not (rec["stream"] == 0).any() and (rec["stream"] == 1).any()
    calm.close()
    b.close()


# ---------------------------------------------------------------------------
# 6. rt_extract
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["float32", "float64"])
def test_extract_on_a_planted_map_with_two_streams_of_different_durations(precision):
    """rt_extract[_f64] runs the same detection kernel: two streams with the same planted map and previous map, gated by their
    own durations, against the oracle's extractor with each stream's parameters."""
    _need_gpu()
    fs, nperseg, F, T, T_last = sc.FS, 256, 48, 400, 120
    rng = np.random.default_rng(5)
    cur = rng.exponential(1.0, (F, T)) * 1e-12
    last = rng.exponential(1.0, (F, T_last)) * 1e-12
    for fi, a, n in ((3, 20, 8), (7, 60, 14), (11, 100, 21), (15, 150, 33), (19, 200, 45), (23, 260, 64), (40, 0, 10)):
        cur[fi, a:a + n] = 2e-7 * (1.0 + 0.1 * rng.random(n))
    last[40, T_last - 9:] = 2e-7  # ... the run through t = 0 goes on from the previous map: 19 cells in all
    sdt = np.float64 if precision == "float64" else np.float32
    cur, last = cur.astype(sdt), last.astype(sdt)
    times = (nperseg / 2 + np.arange(T) * nperseg) / float(fs)
    mins, maxs = [8.0, 15.0], [40.0, 25.0]
    b = BatchSignalAnalyzer(["0", "1"], sdr_callback_length=nperseg * T, sample_rate=fs, fft_nperseg=nperseg, signal_min_duration_ms=mins,
                            signal_max_duration_ms=maxs, precision=precision)
    maps = np.ascontiguousarray(np.stack([cur.T, cur.T]))      # [S][T][F]
    lasts = np.ascontiguousarray(np.stack([last.T, last.T]))
    d_cur, d_last = _native.DeviceBuffer(0, maps.nbytes), _native.DeviceBuffer(0, lasts.nbytes)
    d_cur.upload(maps)
    d_last.upload(lasts)
    try:
        b.native.extract_device(d_cur.ptr, T, F, d_last.ptr, T_last)
        rec = b.native.fetch()
    finally:
        d_cur.free()
        d_last.free()
    found = []
    for s in range(2):
        p = oracle.ExtractParams(-90.0, 5.0, mins[s], maxs[s], 0.0)
        want = oracle.extract_records(times, cur, last, p)
        mine = rec[rec["stream"] == s]
        assert [(int(r["fi"]), int(r["start"]), int(r["end"])) for r in mine] == [(x.fi, x.start, x.end) for x in want], s
        tol = F64_DB_TOL if precision == "float64" else POWER_TOL_DB
        np.testing.assert_allclose(oracle.to_db(mine["max_p"]), [x.max_dbw for x in want], rtol=0, atol=tol)
        np.testing.assert_allclose(oracle.to_db(mine["mean_p"]), [x.avg_dbw for x in want], rtol=0, atol=tol)
        found.append([(x.fi, x.start, x.end) for x in want])
    assert len(found[0]) >= 4 and len(found[1]) >= 2 and found[0] != found[1]
    assert any(st < 0 for _, st, _ in found[0])
    b.close()


# ---------------------------------------------------------------------------
# 7. BatchRunner
# ---------------------------------------------------------------------------
def test_batch_runner_queues_every_devices_signals_with_its_own_settings():
    _need_gpu()

    class Q:
        def __init__(self):
            self.items = []

        def put(self, x):
            self.items.append(x)

    nperseg = 256
    picks = [sc.NAMES.index(n) for n in ("defaults", "min15", "centre", "max25")]
    devices = [sc.NAMES[i] for i in picks]
    bufs = sc.buffers(nperseg, sc.SIGMA_QUIET)
    blen = bufs.shape[1]
    kw = sc.batch_kwargs(nperseg, streams=picks)
    q = Q()
    t0 = 1_700_000_000.0
    r = BatchRunner(device=devices, gpus=[0], signal_queue=q, sdr_callback_length=blen, **kw)
    r.start_analyzers()
    res = sc.oracle_run(bufs, nperseg, streams=picks)
    for k in range(2):
        q.items.clear()
        r.process(_same_iq(bufs[k], len(picks)), now=t0 + k * blen / sc.FS)
        for j, name in enumerate(devices):
            got = [(m.frequency, m.duration) for m in q.items if isinstance(m, Signal) and m.device == name]
            want = [(x.frequency, x.duration) for x in res[j][k][1]]  # what the reference queues: after the shadow filter
            assert len(want) > 0 and got == want, (k, name, got, want)
    centre = [m.frequency for m in q.items if isinstance(m, Signal) and m.device == "centre"]
    plain = [m.frequency for m in q.items if isinstance(m, Signal) and m.device == "defaults"]
    assert [c - p for c, p in zip(centre, plain)] == [433920000 - 150150000] * len(plain)
    r.stop_analyzers()
