"""Every bin's noise level (``row_means=True``, RT_FLAG_ROW_MEANS) on the GPU: the row means of every size family within the
float32 round-off model of ``tests/precision64.py``, every record's ``row_mean`` equal to its bin's entry bit for bit, the same
bits on every mode, lane split and detection form, after AUTO's partial re-runs and record growth; which call they belong to
with two calls in flight; the float64 handle; and ``SignalAnalyzer.noise_dbw`` against the oracle."""
import math

import numpy as np
import pytest

from oracle import analyze_oracle as oracle
from pyradiotracking_amd import _native, dB, synth
from pyradiotracking_amd.analyze import BatchSignalAnalyzer, SignalAnalyzer
from tests import float64_cases as fc
from tests import golden_util as gu
from tests import precision64 as p64

pytestmark = pytest.mark.gpu

LIN_WINDOWS = ("hamming", "hann", "boxcar")
U64 = 2.0 ** -53


@pytest.fixture(autouse=True)
def _need_gpu():
    if _native.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")


def _batch(S, blen, fs=2048000, nperseg=256, window="hamming", mode="auto", **kw):
    return BatchSignalAnalyzer([str(i) for i in range(S)], sdr_callback_length=blen, sample_rate=fs, fft_nperseg=nperseg,
                               fft_window=window, mode=mode, **kw)


def _streams(S, n, fs, nperseg, window, seed, pulses=4, sigma=synth.NOISE_SIGMA, peak=(-80.0, -60.0), dur_ms=(2, 12)):
    w = oracle.window_coefficients(window, nperseg)
    out = []
    for s in range(S):
        rng = np.random.default_rng([seed, s])
        p = synth.random_pulses(rng, n, fs, w, pulses, dur_ms=dur_ms, peak_dbw=peak) if pulses else []
        out.append(synth.make_stream(synth.StreamSpec(n, fs, p, noise_sigma=sigma), seed * 1000 + s))
    return np.stack(out)


def _check_records_bits(rec, rm, nperseg, what=""):
    """Every record's row_mean is its bin's entry, bit for bit."""
    flat = rm.reshape(-1)
    idx = rec["stream"].astype(np.int64) * nperseg + rec["fi"].astype(np.int64)
    got = flat[idx]
    assert np.array_equal(got.view(np.uint32 if rm.dtype == np.float32 else np.uint64),
                          np.ascontiguousarray(rec["row_mean"]).view(np.uint32 if rm.dtype == np.float32 else np.uint64)), what


def _run(b, bufs, u8=False):
    """bufs [n_buffers] of [S, B] (or uint8 [S, 2B]) -> [(records, row means, call info)] one call at a time."""
    out = []
    for chunk in bufs:
        (b.enqueue_bytes if u8 else b.enqueue)(np.ascontiguousarray(chunk))
        rec = b.fetch_records()
        rm = b.fetch_row_means()
        _check_records_bits(rec, rm, b.fft_nperseg)
        out.append((rec, rm, b.native.call_info()))
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


# ----------------------------------------------------------------------------------------------------------------------
# 1. every size family, within the float32 model
# ----------------------------------------------------------------------------------------------------------------------
_SIZES = (8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 300, 1000)
_WINDOWS = ("hamming", ("tukey", 0.3))  # (a tukey window is no cosine sum: the subtract-first form everywhere)


@pytest.mark.parametrize("u8", [False, True], ids=["c64", "u8"])
@pytest.mark.parametrize("window", _WINDOWS, ids=["hamming", "tukey"])
@pytest.mark.parametrize("nperseg", _SIZES)
def test_every_size_family_within_the_model(nperseg, window, u8):
    fs = 2048000
    S = 3
    T = max(12, 300000 // nperseg)
    n = T * nperseg + nperseg // 3
    iq = _streams(S, n, fs, nperseg, window, seed=nperseg + (7 if u8 else 0), dur_ms=(9, 14))
    raw = synth.quantize_u8(iq, gain=8.0) if u8 else None
    b = _batch(S, n, fs, nperseg, window, row_means=True, signal_threshold_dbw=-75.0)
    (rec, rm, info), = _run(b, [raw if u8 else iq], u8=u8)
    b.close()
    assert rm.shape == (S, nperseg) and rm.dtype == np.float32
    assert len(rec) > 0
    L = max(1, int(info.segs_per_chunk))
    lin = (isinstance(window, str) and window in LIN_WINDOWS and 32 <= nperseg <= 4096 and nperseg & (nperseg - 1) == 0 and not u8)
    for s in range(S):
        x = synth.u8_to_complex64_like_kernel(raw[s]) if u8 else iq[s]
        ref = p64.stft_power_f64(x, fs, window, nperseg)
        bound = p64.row_mean_bound(ref, p64.cell_bounds(ref, "lin" if lin else "sub"), L)
        err = np.abs(rm[s].astype(np.float64) - ref.P.mean(axis=0))
        k = int(np.argmax(err / bound))
        assert np.all(err <= bound), f"nperseg {nperseg} stream {s} bin {k}: {rm[s][k]!r} vs {ref.P.mean(axis=0)[k]!r} (bound {bound[k]:.3g})"


# ----------------------------------------------------------------------------------------------------------------------
# 2. modes
# ----------------------------------------------------------------------------------------------------------------------
def _mode_runs(bufs, modes, **kw):
    geometry = (kw.pop("sample_rate", 2048000), kw.pop("fft_nperseg", 256), kw.pop("fft_window", "hamming"))
    runs = {}
    for mode in modes:
        try:
            b = _batch(bufs[0].shape[0], bufs[0].shape[1], *geometry, mode=mode, row_means=True, **kw)
        except _native.NativeError as e:
            assert e.code == _native.RT_E_UNSUPPORTED, (mode, e)  # (a pre-filter level the geometry does not have)
            continue
        try:
            runs[mode] = _run(b, bufs)
        except _native.NativeError as e:
            assert e.code == _native.RT_E_HOT_OVERFLOW and mode != "auto" and mode != "dense", (mode, e)  # (a pinned level too narrow)
        b.close()
    return runs


def _assert_same(runs, base="dense"):
    want = runs[base]
    for mode, got in runs.items():
        for k, ((r0, m0, _), (r1, m1, _)) in enumerate(zip(want, got)):
            assert np.array_equal(_bits(m0), _bits(m1)), (mode, k)


def test_modes_give_the_same_bits_on_clean_input():
    fs, nperseg = 2048000, 256
    B = 700 * nperseg + 40
    iq = _streams(4, 2 * B, fs, nperseg, "hamming", seed=21, pulses=8, dur_ms=(9, 14))
    runs = _mode_runs([iq[:, :B], iq[:, B:]], ("dense", "sparse", "prefilter", "runfilter", "auto"), sample_rate=fs,
                      signal_min_duration_ms=8)
    assert {"dense", "sparse", "auto"} <= set(runs) and len(runs) >= 4, sorted(runs)
    _assert_same(runs)


@pytest.mark.parametrize("floor_db", [0.0, 4.0])
def test_modes_give_the_same_bits_under_the_noise_floor(floor_db):
    bufs, _, kw = gu.reference_noise_floor_case(floor_db)
    S = 3
    bufs = [np.stack([b] * S) for b in bufs]
    runs = _mode_runs(bufs, ("dense", "sparse", "prefilter", "runfilter", "auto"), **kw)
    assert {"dense", "auto"} <= set(runs) and len(runs) >= 3, sorted(runs)
    _assert_same(runs)


def test_auto_partial_dense_rerun_equals_the_dense_run():
    """One noisy stream among clean ones overflows its candidate lists: AUTO re-runs it alone, densely."""
    fs, nperseg, B, S = 300000, 256, 256 * 700, 12
    w = oracle.window_coefficients("hamming", nperseg)
    iq = []
    for s in range(S):
        rng = np.random.default_rng([45, s])
        p = synth.random_pulses(rng, 2 * B, fs, w, 6, peak_dbw=(-80.0, -62.0))
        sigma = float(np.sqrt(10 ** (-88.0 / 10) * fs / 2)) if s == 5 else synth.NOISE_SIGMA
        iq.append(synth.make_stream(synth.StreamSpec(2 * B, fs, p, noise_sigma=sigma), seed=800 + s))
    iq = np.stack(iq)
    bufs = [iq[:, :B], iq[:, B:]]
    runs = _mode_runs(bufs, ("dense", "auto"), sample_rate=fs, record_capacity=2048)
    assert any(info.n_dense_streams > 0 for _, _, info in runs["auto"]), [i.n_dense_streams for _, _, i in runs["auto"]]
    _assert_same(runs)


# ----------------------------------------------------------------------------------------------------------------------
# 3. lanes and detection forms
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nperseg", [256, 128, 1000])
def test_lanes_and_group_detect_give_the_same_bits(nperseg):
    fs, S = 2048000, 7
    B = (200000 // nperseg) * nperseg + 5
    iq = _streams(S, 2 * B, fs, nperseg, "hamming", seed=33 + nperseg, pulses=6)
    bufs = [iq[:, :B], iq[:, B:]]
    want = None
    for lanes in (1, 2, 3):
        for gd in (False, True):
            b = _batch(S, B, fs, nperseg, lanes=lanes, group_detect=gd, row_means=True)
            got = _run(b, bufs)
            b.close()
            if want is None:
                want = got
                continue
            for k in range(len(bufs)):
                assert np.array_equal(_bits(want[k][1]), _bits(got[k][1])), (lanes, gd, k)
                assert np.array_equal(want[k][0], got[k][0]), (lanes, gd, k)


# ----------------------------------------------------------------------------------------------------------------------
# 4. two calls in flight
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [1, 2])
def test_pipelined_calls_and_invalidation(lanes):
    fs, nperseg, S = 2048000, 256, 4
    B = 300 * nperseg
    iq = _streams(S, 4 * B, fs, nperseg, "hamming", seed=44, pulses=10)
    bufs = [iq[:, k * B:(k + 1) * B] for k in range(4)]
    b = _batch(S, B, row_means=True, lanes=lanes)
    seq = _run(b, bufs)
    b.reset()
    with pytest.raises(_native.NativeError) as ei:
        b.fetch_row_means()  # (reset: nothing delivered since)
    assert ei.value.code == _native.RT_E_INVALID
    b.close()

    b = _batch(S, B, row_means=True, lanes=lanes)
    with pytest.raises(_native.NativeError):
        b.fetch_row_means()  # (nothing delivered yet)
    b.enqueue(bufs[0])
    b.enqueue(bufs[1])
    r0 = b.fetch_records()
    m0 = b.fetch_row_means()
    assert np.array_equal(_bits(m0), _bits(seq[0][1]))
    assert np.array_equal(_bits(b.fetch_row_means(dbw=True)), _bits(dB(seq[0][1])))
    _check_records_bits(r0, m0, nperseg)
    r1 = b.fetch_records()
    m1 = b.fetch_row_means()
    assert np.array_equal(_bits(m1), _bits(seq[1][1]))
    _check_records_bits(r1, m1, nperseg)
    b.enqueue(bufs[2])
    with pytest.raises(_native.NativeError) as ei:
        b.fetch_row_means()
    assert ei.value.code == _native.RT_E_INVALID
    b.fetch_records()
    assert np.array_equal(_bits(b.fetch_row_means()), _bits(seq[2][1]))
    b.reset()
    with pytest.raises(_native.NativeError) as ei:
        b.fetch_row_means()
    assert ei.value.code == _native.RT_E_INVALID
    b.close()


# ----------------------------------------------------------------------------------------------------------------------
# 5. record growth
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["auto", "dense"])
def test_record_growth_keeps_the_row_means(mode):
    fs, nperseg, S = 2048000, 256, 3
    B = 2000 * nperseg
    iq = _streams(S, B, fs, nperseg, "hamming", seed=55, pulses=120, dur_ms=(2, 4))
    small = _batch(S, B, mode=mode, row_means=True, record_capacity=16, signal_min_duration_ms=1)
    (rs, ms, _), = _run(small, [iq])
    small.close()
    big = _batch(S, B, mode=mode, row_means=True, record_capacity=4096, signal_min_duration_ms=1)
    (rb, mb, _), = _run(big, [iq])
    big.close()
    assert max(int((rb["stream"] == s).sum()) for s in range(S)) > 16  # (a stream outgrew the first capacity)
    assert np.array_equal(rs, rb)
    assert np.array_equal(_bits(ms), _bits(mb))


# ----------------------------------------------------------------------------------------------------------------------
# 6. edge cases and the flag
# ----------------------------------------------------------------------------------------------------------------------
def test_short_buffer_gives_nan():
    for nperseg in (256, 300):
        b = _batch(2, 4 * nperseg, nperseg=nperseg, row_means=True)
        b.enqueue(np.zeros((2, nperseg - 1), np.complex64))
        assert len(b.fetch_records()) == 0
        rm = b.fetch_row_means()
        assert rm.shape == (2, nperseg) and np.all(np.isnan(rm))
        b.close()


def test_flag_off_refuses_and_leaves_records_alone():
    fs, nperseg, S = 2048000, 256, 4
    B = 500 * nperseg
    iq = _streams(S, 2 * B, fs, nperseg, "hamming", seed=66, pulses=8)
    recs = {}
    for flag in (False, True):
        b = _batch(S, B, row_means=flag)
        recs[flag] = []
        for k in range(2):
            b.enqueue(iq[:, k * B:(k + 1) * B])
            recs[flag].append(b.fetch_records())
            if not flag:
                with pytest.raises(_native.NativeError) as ei:
                    b.fetch_row_means()
                assert ei.value.code == _native.RT_E_INVALID
        b.close()
    for a, c in zip(recs[False], recs[True]):
        assert a.tobytes() == c.tobytes()


def test_extract_call_has_no_row_means():
    nperseg, S, T = 256, 2, 400
    b = _batch(S, T * nperseg, row_means=True)
    b.enqueue(_streams(S, T * nperseg, 2048000, nperseg, "hamming", seed=77))
    b.fetch_records()
    b.fetch_row_means()
    spec = np.full((S, T, nperseg), 1e-12, np.float32)
    spec[:, 50:150, 7] = 1e-6  # (a plateau of 12.5 ms)
    d = _native.DeviceBuffer(0, spec.nbytes)
    d.upload(spec)
    b.native.extract_device(d.ptr, T, nperseg, None, 0)
    with pytest.raises(_native.NativeError):
        b.fetch_row_means()  # (an rt_extract was enqueued since)
    assert len(b.native.fetch()) > 0
    with pytest.raises(_native.NativeError) as ei:
        b.fetch_row_means()  # (the delivered call was an rt_extract)
    assert ei.value.code == _native.RT_E_INVALID
    d.free()
    b.close()


def test_twin_entry_points_refuse_the_other_precision():
    import ctypes as C

    lib = _native.load_library()
    for precision in ("float32", "float64"):
        b = _batch(1, 4096, precision=precision, row_means=True)
        out = np.zeros(256, np.float64)
        fn = lib.rt_fetch_row_means if precision == "float64" else lib.rt_fetch_row_means_f64
        assert fn(b.native._handle, out.ctypes.data, C.c_size_t(256)) == _native.RT_E_INVALID
        b.enqueue(np.zeros((1, 4096), np.complex64))
        b.fetch_records()
        good = lib.rt_fetch_row_means_f64 if precision == "float64" else lib.rt_fetch_row_means
        assert good(b.native._handle, out.ctypes.data, C.c_size_t(255)) == _native.RT_E_INVALID  # (wrong n)
        assert good(b.native._handle, None, C.c_size_t(256)) == _native.RT_E_INVALID
        assert good(b.native._handle, out.ctypes.data, C.c_size_t(256)) == _native.RT_OK
        b.close()


# ----------------------------------------------------------------------------------------------------------------------
# 7. float64 handles
# ----------------------------------------------------------------------------------------------------------------------
def _f64_bound(x, nperseg, want):
    """|got - np.mean(row)| <= (T + 1) u want + 3 log2(M) 64 u mean_t sqrt(P[t, k] E_t): the sequential float64 sum of T positive
    cells against NumPy's pairwise one (each within (T - 1) u of the exact sum), plus a float64 transform's per-cell error --
    M the transform length (Bluestein's padded one), E_t the segment's mean cell power (|dX_k| ~ log2(M) u ||X|| / sqrt(N))."""
    _, _, spec = oracle.stft_power(x, fc.FS, "hamming", nperseg)  # [F, T] float64
    T = spec.shape[1]
    m = 1
    while m < (nperseg if nperseg & (nperseg - 1) == 0 else 2 * nperseg - 1):
        m <<= 1
    e_t = spec.mean(axis=0)
    return (T + 1) * U64 * want + 3 * math.log2(m) * 64 * U64 * np.sqrt(spec * e_t[None, :]).mean(axis=1)


@pytest.mark.parametrize("u8", [False, True], ids=["c128", "u8"])
@pytest.mark.parametrize("nperseg", [256, 300, 4096, 8192])
def test_float64_row_means(nperseg, u8):
    n = 300000
    x = fc.threshold_buffer(3, n)
    if u8:
        raw = synth.quantize_u8(x.astype(np.complex64), gain=2.0e7)
        x = synth.u8_to_complex128_like_pyrtlsdr(raw)
    b = BatchSignalAnalyzer(["0"], sdr_callback_length=n, sample_rate=fc.FS, fft_nperseg=nperseg, precision="float64", row_means=True)
    (b.enqueue_bytes if u8 else b.enqueue)((raw if u8 else x).reshape(1, -1))
    rec = b.fetch_records()
    rm = b.fetch_row_means()
    assert rm.dtype == np.float64 and rm.shape == (1, nperseg)
    _check_records_bits(rec, rm, nperseg, "float64")
    _, _, spec = oracle.stft_power(x, fc.FS, "hamming", nperseg)
    want = spec.mean(axis=1)  # np.mean(row), float64
    bound = _f64_bound(x, nperseg, want)
    err = np.abs(rm[0] - want)
    k = int(np.argmax(err / bound))
    assert np.all(err <= bound), f"bin {k}: {rm[0][k]!r} vs {want[k]!r} (bound {bound[k]:.3g})"
    # a short buffer: NaN, and the next call's row means again
    b.enqueue(np.zeros((1, nperseg - 1), np.complex128))
    b.fetch_records()
    assert np.all(np.isnan(b.fetch_row_means()))
    b.close()


# ----------------------------------------------------------------------------------------------------------------------
# 8. drop-in
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gu.iq_case_names())
def test_signal_analyzer_noise_dbw(name):
    meta, kwargs, buffers, ts_starts, expected = gu.iq_case(name)
    an = SignalAnalyzer("0", sdr_callback_length=meta["buffer_len"], row_means=True, **kwargs)
    assert an.noise_dbw is None
    fs = kwargs.get("sample_rate", 300000)
    nperseg = kwargs.get("fft_nperseg", 256)
    window = kwargs.get("fft_window", "hamming")
    n_sig = 0
    for buf, ts in zip(buffers, ts_starts):
        sigs = an.analyze_buffer(buf, ts, filtered=False)
        freqs, _, spec = oracle.stft_power(np.asarray(buf, dtype=np.complex64), fs, window, nperseg)
        nd = an.noise_dbw
        assert nd.shape == (nperseg,) and nd.dtype == np.float32
        with np.errstate(divide="ignore"):
            want = dB(spec.mean(axis=1).astype(np.float64))
        np.testing.assert_allclose(nd, want, rtol=0, atol=0.01)
        cf = kwargs.get("center_freq", 150150000)
        for sg in sigs:
            fi = int(np.argmin(np.abs(freqs + cf - sg.frequency)))
            assert np.float32(sg.noise).tobytes() == nd[fi].tobytes(), (name, sg)
        n_sig += len(sigs)
    an.extract_signals(np.arange(nperseg, dtype=np.float64), np.arange(4) * nperseg / fs, np.full((nperseg, 4), 1e-15), ts_starts[0])
    assert an.noise_dbw is None
    plain = SignalAnalyzer("0", sdr_callback_length=meta["buffer_len"], **kwargs)
    plain.analyze_buffer(buffers[0], ts_starts[0])
    assert plain.noise_dbw is None
