"""The float64 handle (precision="float64", rt_create_f64) on the GPU against the oracle on complex128 input -- the
reference's own precision.  Family (a) (tests/float64_cases.py) holds buffers whose complex64 and complex128 answers differ:
the float32 path gives the complex64 one."""
import datetime

import numpy as np
import pytest

from oracle import analyze_oracle as oracle
from pyradiotracking_amd import _native, synth
from pyradiotracking_amd.analyze import BatchSignalAnalyzer, SignalAnalyzer
from tests import float64_cases as fc

pytestmark = pytest.mark.gpu

DB_TOL = 1e-9   # max / avg / noise / snr, dB
STD_TOL = 1e-5  # std, dB


@pytest.fixture(autouse=True)
def _need_gpu():
    if _native.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")


def _check(rec, want, cal=0.0):
    """rt_record_f64 rows of one stream against oracle records (all of them, shadow verdicts from the oracle's filter)."""
    sig = oracle.records_to_signals(want, np.zeros(16384), fc.TS0, "0", 0.0)
    kept = {(s.fi, s.start) for s in oracle.filter_shadows(sig)}
    assert [(int(r["fi"]), int(r["start"]), int(r["end"])) for r in rec] == fc.key(want)
    assert [int(r["shadowed"]) for r in rec] == [0 if (w.fi, w.start) in kept else 1 for w in want]
    if not len(want):
        return
    np.testing.assert_allclose(oracle.to_db(rec["max_p"]) - cal, [w.max_dbw for w in want], rtol=0, atol=DB_TOL)
    np.testing.assert_allclose(oracle.to_db(rec["mean_p"]) - cal, [w.avg_dbw for w in want], rtol=0, atol=DB_TOL)
    np.testing.assert_allclose(oracle.to_db(rec["row_mean"]), [w.noise_dbw for w in want], rtol=0, atol=DB_TOL)
    np.testing.assert_allclose(oracle.to_db(rec["mean_p"] / rec["row_mean"]), [w.snr_db for w in want], rtol=0, atol=DB_TOL)
    np.testing.assert_allclose(rec["std_db"], [w.std_db for w in want], rtol=0, atol=STD_TOL)


def _run(x, feed, nperseg=fc.NPERSEG, window="hamming", fs=fc.FS, **kw):
    import torch

    b = BatchSignalAnalyzer(["0"], precision="float64", sdr_callback_length=len(x), fft_nperseg=nperseg, fft_window=window,
                            sample_rate=fs, **kw)
    try:
        if feed == "host":
            b.enqueue(x[None, :])
        elif feed == "device":
            b.enqueue(torch.from_numpy(x[None, :].copy()).cuda())
        else:
            b.enqueue_bytes(x[None, :])
        return b.fetch_records()
    finally:
        b.close()


SEEDS = fc.threshold_seeds(120)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("feed", ["host", "device"])
def test_threshold_level_matches_complex128_reference(seed, feed):
    x = fc.threshold_buffer(seed)
    want, _ = fc.oracle_records(x)
    _check(_run(x, feed), want)


def _pulses(n, fs, nperseg, window, seed, sigma=synth.NOISE_SIGMA, n_pulses=4):
    """complex128 buffer: noise and ``n_pulses`` random pulses (synth.random_pulses), added in float64."""
    rng = np.random.default_rng([128, seed])
    w = oracle.window_coefficients(window, nperseg)
    x = sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for p in synth.random_pulses(rng, n, fs, w, n_pulses, dur_ms=(10.0, 30.0), peak_dbw=(-80.0, -60.0)):
        a, b = max(0, p.start), min(n, p.start + p.length)
        if b > a:
            t = np.arange(a, b, dtype=np.float64) / fs
            x[a:b] += p.amp * np.exp(2j * np.pi * (p.freq * t + p.phase))
    return x


CASES = [
    (256, "hamming", 0.0), (256, ("tukey", 0.25), 0.0), (256, ("kaiser", 8.0), 2.5), (8, "hamming", 0.0), (128, "hann", 0.0),
    (300, "hamming", 0.0), (1000, "hamming", 0.0), (4096, "hamming", 0.0), (8192, "hamming", 0.0),
]


@pytest.mark.parametrize("nperseg,window,cal", CASES)
def test_records_match_complex128_reference(nperseg, window, cal):
    fs = 300000
    n = max(300000, nperseg * 64)
    x = _pulses(n, fs, nperseg, window, nperseg)
    want, _ = fc.oracle_records(x, nperseg, window, fs, calibration_db=cal)
    for feed in ("host", "device"):
        _check(_run(x, feed, nperseg, window, fs, calibration_db=cal), want, cal)


def test_wire_format_bytes():
    rng = np.random.default_rng(77)
    x = _pulses(300000, fc.FS, 256, "hamming", 3, sigma=0.05)
    raw = synth.quantize_u8(x / np.abs(x).max() * 0.9)
    want, _ = fc.oracle_records(synth.u8_to_complex128_like_pyrtlsdr(raw), signal_threshold_dbw=-60.0)
    rec = _run(raw, "bytes", signal_threshold_dbw=-60.0)
    _check(rec, want)


@pytest.mark.parametrize("nperseg", [8, 16, 100, 256, 300, 1000, 1024, 4096, 8192])
def test_spectrogram_f64_against_scipy(nperseg):
    import torch

    fs, S = 300000, 2
    n = nperseg * 40
    rng = np.random.default_rng(nperseg)
    x = rng.standard_normal((S, n)) + 1j * rng.standard_normal((S, n)) + 0.3
    x[:, ::7] *= 1e3  # a dynamic range for the bound to mean something
    b = BatchSignalAnalyzer([str(i) for i in range(S)], precision="float64", sdr_callback_length=n, fft_nperseg=nperseg, sample_rate=fs)
    d = torch.from_numpy(x).cuda()
    T = n // nperseg
    out = torch.zeros((S, T, nperseg), dtype=torch.float64, device="cuda")
    b.native.spectrogram_device(d.data_ptr(), n, n, out.data_ptr())
    got = out.cpu().numpy()
    b.close()
    for s in range(S):
        _, _, ref = oracle.stft_power(x[s], fs, "hamming", nperseg)
        ref = np.moveaxis(ref, 0, -1)  # [T, N]
        bound = 1e-13 * np.log2(max(nperseg, 2)) * ref.max(axis=1, keepdims=True)
        assert np.all(np.abs(got[s] - ref) <= bound), float(np.max(np.abs(got[s] - ref) / bound))


def test_lookback_reset_and_two_in_flight():
    fs, nperseg, n = fc.FS, 256, 60000
    rng = np.random.default_rng(5)
    w = oracle.window_coefficients("hamming", nperseg)
    x = 1e-9 * (rng.standard_normal(3 * n) + 1j * rng.standard_normal(3 * n))
    amp = np.sqrt(10 ** (-70 / 10) * fs * (w * w).sum()) / w.sum()
    for start in (n - 3000, 2 * n - 5000):  # pulses straddling the buffer boundaries
        k = np.arange(6000)
        x[start:start + 6000] += amp * np.exp(2j * np.pi * 20 * (start + k) / nperseg)
    bufs = [x[i * n:(i + 1) * n] for i in range(3)]
    oa = oracle.OracleAnalyzer()
    want = [oa.process(bb, fc.TS0)[0] for bb in bufs]
    b = BatchSignalAnalyzer(["0"], precision="float64", sdr_callback_length=n)
    b.enqueue(bufs[0][None, :])
    b.enqueue(bufs[1][None, :])  # two calls in flight
    got0 = b.fetch_records()
    b.enqueue(bufs[2][None, :])
    got1, got2 = b.fetch_records(), b.fetch_records()
    assert [(int(r["fi"]), int(r["start"]), int(r["end"])) for r in got1] == [(s.fi, s.start, s.end) for s in want[1]]
    assert any(int(r["start"]) < 0 for r in got1) and any(int(r["start"]) < 0 for r in got2)
    for g, wnt in ((got0, want[0]), (got2, want[2])):
        assert [(int(r["fi"]), int(r["start"]), int(r["end"])) for r in g] == [(s.fi, s.start, s.end) for s in wnt]
    # reset_stream: the next buffer without look-back, as a fresh analyzer
    b.enqueue(bufs[0][None, :])
    b.fetch_records()
    b.reset_stream(0)
    b.enqueue(bufs[1][None, :])
    fresh = oracle.OracleAnalyzer().process(bufs[1], fc.TS0)[0]
    assert [(int(r["fi"]), int(r["start"]), int(r["end"])) for r in b.fetch_records()] == [(s.fi, s.start, s.end) for s in fresh]
    assert b.call_info().mode_used == _native.RT_MODE_DENSE
    b.close()


def test_per_stream_calibration_and_growth():
    fs, nperseg, n = fc.FS, 256, 300000
    cal = [0.0, 3.0, -2.0]
    bufs = [_pulses(n, fs, nperseg, "hamming", 40 + s) for s in range(3)]
    # stream 0: hundreds of plateaus (a pulse train in many bins), from record_capacity=4
    rng = np.random.default_rng(9)
    w = oracle.window_coefficients("hamming", nperseg)
    amp = np.sqrt(10 ** (-60 / 10) * fs * (w * w).sum()) / w.sum()
    for k0 in range(0, n - 6000, 9000):
        fb = int(rng.integers(1, 250))
        k = np.arange(4000)
        bufs[0][k0:k0 + 4000] += amp * np.exp(2j * np.pi * fb * (k0 + k) / nperseg)
    b = BatchSignalAnalyzer(["a", "b", "c"], precision="float64", calibration_db=cal, sdr_callback_length=n, record_capacity=4)
    b.enqueue(np.stack(bufs))
    rec = b.fetch_records()
    b.close()
    for s in range(3):
        want, _ = fc.oracle_records(bufs[s], calibration_db=cal[s])
        _check(rec[rec["stream"] == s], want, cal[s])
    assert (rec["stream"] == 0).sum() >= 30


def test_lanes_refused():
    with pytest.raises(_native.NativeError) as ei:
        BatchSignalAnalyzer(["0", "1"], precision="float64", lanes=2, sdr_callback_length=4096)
    assert ei.value.code == _native.RT_E_UNSUPPORTED


def test_sparse_mode_refused():
    with pytest.raises(_native.NativeError) as ei:
        BatchSignalAnalyzer(["0"], precision="float64", mode="sparse", sdr_callback_length=4096)
    assert ei.value.code == _native.RT_E_UNSUPPORTED


def test_signal_analyzer_drop_in():
    import queue

    x = fc.threshold_buffer(SEEDS[0] if SEEDS else 0)
    q = queue.Queue()
    sa = SignalAnalyzer("0", precision="float64", signal_queue=q, sdr_callback_length=len(x))
    ts = datetime.datetime(2024, 1, 1, tzinfo=datetime.timezone.utc)
    got = sa.analyze_buffer(x, ts)
    _, kept = oracle.OracleAnalyzer().process(x, ts)
    assert [(s.frequency, s.ts, s.duration) for s in got] == [(k.frequency, k.ts, k.duration) for k in kept]
    for g, k in zip(got, kept):
        assert abs(g.max - k.max) < DB_TOL and abs(g.avg - k.avg) < DB_TOL and abs(g.snr - k.snr) < DB_TOL
        assert abs(g.noise - k.noise) < DB_TOL and abs(g.std - k.std) < STD_TOL
    # extract_signals on a float64 map
    freqs, times, spec = oracle.stft_power(x, fc.FS, "hamming", fc.NPERSEG)
    ex = sa.extract_signals(freqs, times, spec, ts)
    want = oracle.extract_records(times, spec, None, oracle.ExtractParams())
    assert len(ex) == len(want)
    for e, w in zip(ex, want):
        assert abs(e.max - w.max_dbw) < DB_TOL and abs(e.std - w.std_db) < STD_TOL
    # process_bytes: the wire format through pyrtlsdr's conversion, in float64
    raw = synth.quantize_u8(_pulses(60000, fc.FS, 256, "hamming", 11, sigma=0.05) * 4)
    sa2 = SignalAnalyzer("0", precision="float64", signal_queue=q, sdr_callback_length=60000, signal_threshold_dbw=-60.0)
    sa2.process_bytes(raw)
    sa2._batch.close()
    sa._batch.close()
