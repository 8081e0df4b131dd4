"""The float64 handle's contract without a GPU: record layout, argument checks of rt_create_f64 before any device is touched,
the precision keyword, and the rt_core.h predicates instantiated on double (through _rt_hostcheck.so) against the oracle."""
import ctypes as C

import numpy as np
import pytest

from oracle import analyze_oracle as oracle
from pyradiotracking_amd import _native, build
from pyradiotracking_amd.analyze import BatchSignalAnalyzer, SignalAnalyzer
from tests import float64_cases as fc


class _RecF64(C.Structure):  # include/rt_analyze.h: rt_record_f64
    _fields_ = [("stream", C.c_int32), ("fi", C.c_int32), ("start", C.c_int32), ("end", C.c_int32), ("max_p", C.c_double),
                ("mean_p", C.c_double), ("std_db", C.c_double), ("row_mean", C.c_double), ("shadowed", C.c_int32),
                ("reserved", C.c_int32)]


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _native.load_library()


@pytest.fixture(scope="module")
def hc():
    build.build_hostcheck()
    h = C.CDLL(build.HOSTCHECK)
    dp, ip, d = C.POINTER(C.c_double), C.c_int, C.c_double
    h.hc_extract_f64.argtypes = [dp, ip, ip, dp, ip, ip, ip, d, d, d, d, d, d, C.c_void_p, ip]
    h.hc_extract_f64.restype = ip
    return h


def test_record_f64_layout():
    dt = _native.RECORD_F64_DTYPE
    assert dt.itemsize == 56 == C.sizeof(_RecF64)
    for name, _ in _RecF64._fields_:
        assert dt.fields[name][1] == getattr(_RecF64, name).offset, name
    assert C.sizeof(_native.RtConfigF64) == 40


def _create(lib, nperseg=256, mode=_native.RT_MODE_DENSE, window=True, lanes=1):
    cfg = _native.RtConfig()
    cfg.n_streams, cfg.nperseg, cfg.mode, cfg.max_samples, cfg.sample_rate = 1, nperseg, mode, 1 << 16, 300000.0
    cfg.min_duration_s, cfg.max_duration_s, cfg.lanes = 0.008, 0.04, lanes
    w = np.hamming(max(nperseg, 8))
    c64 = _native.RtConfigF64()
    c64.window = w.ctypes.data_as(C.POINTER(C.c_double)) if window else None
    c64.scale, c64.threshold, c64.snr_threshold = 1.0, 1e-9, 3.0
    h = C.c_void_p()
    rc = lib.rt_create_f64(C.byref(cfg), C.byref(c64), C.byref(h))
    msg = lib.rt_last_error(None).decode()
    if rc == _native.RT_OK:
        lib.rt_destroy(h)
    return rc, msg


def test_create_f64_checks_arguments_first(lib):
    assert _create(lib, window=False)[0] == _native.RT_E_INVALID
    for kw in ({"mode": _native.RT_MODE_SPARSE}, {"mode": _native.RT_MODE_PREFILTER}, {"mode": _native.RT_MODE_RUNFILTER},
               {"nperseg": 16384}, {"nperseg": 5000}, {"nperseg": 4}, {"lanes": 2}):
        rc, msg = _create(lib, **kw)
        assert rc == _native.RT_E_UNSUPPORTED, kw
        assert "float64" in msg, (kw, msg)


def test_create_f64_without_gpu_fails_loudly(lib):
    n = C.c_int(0)
    lib.rt_device_count(C.byref(n))
    if n.value > 0:
        pytest.skip("a GPU is present")
    for nperseg in (256, 300, 8192):
        assert _create(lib, nperseg=nperseg)[0] == _native.RT_E_NO_DEVICE
    with pytest.raises(_native.NativeError) as ei:
        BatchSignalAnalyzer(["0"], precision="float64", sdr_callback_length=4096)
    assert ei.value.code == _native.RT_E_NO_DEVICE


def test_precision_keyword():
    with pytest.raises(ValueError):
        BatchSignalAnalyzer(["0"], precision="bogus")
    with pytest.raises(ValueError):
        SignalAnalyzer("0", precision="float16")


def _rand_map(rng, n_seg, n_bins, thr):
    """float64 map with plateaus, cells one ulp either side of the threshold, and noise under it."""
    spec = thr * 10 ** rng.uniform(-4, -2, size=(n_seg, n_bins))
    for fi in range(n_bins):
        t0 = int(rng.integers(-20, n_seg))
        ln = int(rng.integers(4, 50))
        a, b = max(t0, 0), max(0, min(t0 + ln, n_seg))
        if b <= a:
            continue
        spec[a:b, fi] = thr * 10 ** rng.uniform(0.8, 2.0, size=b - a)
        if b < n_seg and rng.random() < 0.5:  # a plateau that ends one ulp under the threshold, or on it
            spec[b, fi] = np.nextafter(thr, 0.0) if rng.random() < 0.5 else thr
    return spec


@pytest.mark.parametrize("seed", range(6))
def test_host_core_f64_against_oracle(hc, seed):
    rng = np.random.default_rng([6464, seed])
    p = oracle.ExtractParams(signal_threshold_dbw=-90.0, snr_threshold_db=5.0, calibration_db=float(rng.uniform(-3, 3)))
    fs, nperseg, n_bins = 300000.0, 256, 24
    n_seg, n_last = int(rng.integers(60, 200)), int(rng.integers(60, 200))
    thr = p.signal_threshold
    cur, last = _rand_map(rng, n_seg, n_bins, thr), _rand_map(rng, n_last, n_bins, thr)
    times = (nperseg / 2 + np.arange(n_seg) * nperseg) / fs
    want = oracle.extract_records(times, cur.T, last.T, p)
    sig = oracle.records_to_signals(want, np.arange(n_bins, dtype=np.float64), fc.TS0, "0", 0.0)
    kept = {(s.fi, s.start) for s in oracle.filter_shadows(sig)}
    out = np.zeros(4096, dtype=_native.RECORD_F64_DTYPE)
    dptr = C.POINTER(C.c_double)
    n = hc.hc_extract_f64(cur.ctypes.data_as(dptr), n_seg, n_bins, last.ctypes.data_as(dptr), n_last, n_last, nperseg, fs, thr,
                          p.snr_threshold, p.calibration_db, p.signal_min_duration, p.signal_max_duration, out.ctypes.data, len(out))
    got = out[:n]
    assert n == len(want)
    assert [(int(r["fi"]), int(r["start"]), int(r["end"])) for r in got] == fc.key(want)
    assert [int(r["shadowed"]) for r in got] == [0 if (w.fi, w.start) in kept else 1 for w in want]
    np.testing.assert_allclose(oracle.to_db(got["max_p"]) - p.calibration_db, [w.max_dbw for w in want], rtol=0, atol=1e-9)
    np.testing.assert_allclose(oracle.to_db(got["mean_p"]) - p.calibration_db, [w.avg_dbw for w in want], rtol=0, atol=1e-9)
    np.testing.assert_allclose(oracle.to_db(got["row_mean"]), [w.noise_dbw for w in want], rtol=0, atol=1e-9)
    np.testing.assert_allclose(got["std_db"], [w.std_db for w in want], rtol=0, atol=1e-9)


def test_threshold_family_exists():
    """Family (a) holds cases where the complex64 and the complex128 reference disagree (the GPU test's ground)."""
    assert len(fc.threshold_seeds(40)) >= 2
