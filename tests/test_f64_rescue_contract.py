"""RT_FLAG_F64_RESCUE without a GPU: the flag's argument checks before any device is touched, the keyword, the round arithmetic of
the rescue scratch (rt_core.h: f64_rescue_rounds) and the sequential twin of the rescue detection (hc_extract_rescue_f64: dense
row walk, row sums given, the previous map as the tail).  On every map the map-free contract test draws the twin's records are
hc_extract_sparse_f64's byte for byte -- a cell the emission rule leaves out is below the absolute threshold, the statistics run
over the same cells in the same order and the row mean comes from the same sum -- and the oracle's keys and verdicts."""
import ctypes as C

import numpy as np
import pytest

from oracle import analyze_oracle as oracle
from pyradiotracking_amd import _native, build
from pyradiotracking_amd.analyze import BatchSignalAnalyzer, SignalAnalyzer
from tests import f64_sparse_cases as sc
from tests import float64_cases as fc
from tests import golden_util as gu
from tests import test_f64_sparse_contract as base

F64_SPARSE, F64_RESCUE = 64, 128
MIB = 1 << 20


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _native.load_library()


@pytest.fixture(scope="module")
def hc():
    build.build_hostcheck()
    h = C.CDLL(build.HOSTCHECK)
    dp, ip, d, vp = C.POINTER(C.c_double), C.c_int, C.c_double, C.c_void_p
    h.hc_extract_sparse_f64.argtypes = [vp, dp, ip, dp, ip, ip, dp, ip, ip, ip, d, d, d, d, d, d, vp, ip]
    h.hc_extract_sparse_f64.restype = ip
    h.hc_extract_rescue_f64.argtypes = [dp, dp, ip, ip, dp, ip, ip, ip, d, d, d, d, d, d, vp, ip]
    h.hc_extract_rescue_f64.restype = ip
    h.hc_f64_rescue_rounds.argtypes = [ip, ip, ip, C.c_longlong, C.POINTER(C.c_int)]
    h.hc_f64_rescue_rounds.restype = None
    h.hc_f64_rescue_budget.restype = C.c_longlong
    return h


# ---- flag rules ----
def test_flag_value():
    assert _native.RT_FLAG_F64_RESCUE == F64_RESCUE


@pytest.mark.parametrize("kw", [dict(flags=F64_RESCUE), dict(flags=F64_RESCUE | _native.RT_FLAG_ROW_MEANS),
                                dict(flags=F64_RESCUE, f64=False), dict(flags=F64_RESCUE | F64_SPARSE, f64=False)],
                         ids=["alone", "with-row-means", "rt_create", "rt_create-both"])
def test_flag_refusals(lib, kw):
    rc, msg = base._create(lib, **kw)
    assert rc == _native.RT_E_INVALID, (kw, rc, msg)
    assert "float64" in msg or "RT_FLAG_F64" in msg, msg


@pytest.mark.parametrize("kw", [dict(), dict(nperseg=32), dict(nperseg=4096), dict(hot_capacity=1024),
                                dict(extra=_native.RT_FLAG_ROW_MEANS | _native.RT_FLAG_TIMING)])
def test_valid_arguments_reach_the_device(lib, kw):
    """With RT_FLAG_F64_SPARSE the flag passes every argument check: RT_E_NO_DEVICE on a box without a GPU."""
    kw = dict(kw)
    flags = F64_SPARSE | F64_RESCUE | kw.pop("extra", 0)
    n = C.c_int(0)
    lib.rt_device_count(C.byref(n))
    rc, msg = base._create(lib, flags=flags, **kw)
    assert rc == (_native.RT_OK if n.value > 0 else _native.RT_E_NO_DEVICE), (kw, rc, msg)


def test_keyword():
    for cls, args in ((BatchSignalAnalyzer, (["0"],)), (SignalAnalyzer, ("0",))):
        with pytest.raises(ValueError):
            cls(*args, f64_rescue=True)  # no f64_sparse, float32
        with pytest.raises(ValueError):
            cls(*args, precision="float64", f64_rescue=True)  # no f64_sparse
        with pytest.raises(ValueError):
            cls(*args, f64_sparse=True, f64_rescue=True)  # precision="float32"
        with pytest.raises(ValueError):
            cls(*args, precision="float64", f64_sparse=True, f64_rescue=True, mode="dense")
    with pytest.raises(ValueError):
        _native.NativeAnalyzer(n_streams=1, nperseg=256, max_samples=4096, sample_rate=3e5, window_f32=np.hamming(256), scale=1.0,
                               threshold=1e-9, snr_threshold=3.0, calibration_db=0.0, min_duration_s=0.008, max_duration_s=0.04,
                               precision="float64", f64_rescue=True)
    if _native.device_count() < 1:
        with pytest.raises(_native.NativeError) as ei:
            BatchSignalAnalyzer(["0"], precision="float64", f64_sparse=True, f64_rescue=True, sdr_callback_length=4096)
        assert ei.value.code == _native.RT_E_NO_DEVICE


# ---- round arithmetic ----
def _rounds(hc, n_bad, T, N, budget):
    out = (C.c_int * 2)()
    hc.hc_f64_rescue_rounds(n_bad, T, N, budget, out)
    return out[0], out[1]


def test_round_arithmetic(hc):
    budget = hc.hc_f64_rescue_budget()
    assert budget == 256 * MIB
    T, N = 64, 4096  # 2 MiB a stream: 128 streams a round
    fit = budget // (T * N * 8)
    assert fit == 128
    assert _rounds(hc, 0, T, N, budget) == (0, 0)
    assert _rounds(hc, -3, T, N, budget) == (0, 0)
    assert _rounds(hc, 1, T, N, budget) == (1, 1)
    assert _rounds(hc, fit - 1, T, N, budget) == (fit - 1, 1)
    assert _rounds(hc, fit, T, N, budget) == (fit, 1)
    assert _rounds(hc, fit + 1, T, N, budget) == (fit, 2)
    assert _rounds(hc, 2 * fit, T, N, budget) == (fit, 2)
    assert _rounds(hc, 2 * fit + 1, T, N, budget) == (fit, 3)
    # one stream larger than the budget: a stream a round (the scratch is then that one stream's map)
    assert _rounds(hc, 5, 1 << 20, 4096, budget) == (1, 5)
    assert _rounds(hc, 1, 1 << 20, 4096, budget) == (1, 1)
    assert _rounds(hc, 3, 100, 256, 100 * 256 * 8 - 1) == (1, 3)
    assert _rounds(hc, 3, 100, 256, 100 * 256 * 8) == (1, 3)
    assert _rounds(hc, 3, 100, 256, 2 * 100 * 256 * 8) == (2, 2)


def test_every_bad_stream_in_exactly_one_round(hc):
    rng = np.random.default_rng(18)
    for _ in range(300):
        n_bad = int(rng.integers(1, 5000))
        T, N = int(rng.integers(2, 3000)), int(2 ** rng.integers(5, 13))
        budget = int(rng.integers(1, 1 << 30))
        per, rounds = _rounds(hc, n_bad, T, N, budget)
        assert 1 <= per <= n_bad
        assert per == 1 or per * T * N * 8 <= budget  # a round fits the scratch (one stream always does: the scratch is then its map)
        assert per == n_bad or (per + 1) * T * N * 8 > budget  # ... and takes what fits
        seen = np.zeros(n_bad, dtype=int)
        for r in range(rounds):  # round r: the list entries [r per, min(n_bad, (r + 1) per)) -- as rt_fetch_f64 walks them
            seen[r * per:min(n_bad, (r + 1) * per)] += 1
            assert r * per < n_bad  # (no empty round)
        assert np.all(seen == 1)


# ---- the twin ----
def rescue_records(hc, spec_ft, last_ft, p, nperseg=256, fs=300000.0):
    """hc_extract_rescue_f64 on one [F][T] map with the row sums the sparse twin is given and the previous map as the tail."""
    cur = np.ascontiguousarray(np.asarray(spec_ft, dtype=np.float64).T)  # [T][F]
    n_seg, n_bins = cur.shape
    sums = np.array([np.add.reduce(np.asarray(row, dtype=np.float64)) for row in spec_ft], dtype=np.float64)
    dptr = C.POINTER(C.c_double)
    last = None if last_ft is None else np.ascontiguousarray(np.asarray(last_ft, dtype=np.float64).T)
    n_last = 0 if last is None else last.shape[0]
    out = np.zeros(8192, dtype=_native.RECORD_F64_DTYPE)
    n = hc.hc_extract_rescue_f64(cur.ctypes.data_as(dptr), sums.ctypes.data_as(dptr), n_seg, n_bins,
                                 None if last is None else last.ctypes.data_as(dptr), n_last, n_last, nperseg, fs, p.signal_threshold,
                                 p.snr_threshold, p.calibration_db, p.signal_min_duration, p.signal_max_duration, out.ctypes.data, len(out))
    assert n <= len(out)
    return out[:n]


def both(hc, spec, last, p, nperseg=256, fs=300000.0, rng=None):
    """The two twins on one map: equal bytes.  Returns the records."""
    sparse, _ = base.sparse_records(hc, spec, last, p, nperseg, fs, rng)
    rescue = rescue_records(hc, spec, last, p, nperseg, fs)
    assert len(rescue) == len(sparse)
    assert rescue.tobytes() == sparse.tobytes()
    return rescue


@pytest.mark.parametrize("nperseg,window,cal", [c for c in sc.SIZE_CASES if c[0] in (32, 256, 2048)])
def test_twins_on_oracle_maps(hc, nperseg, window, cal):
    x = sc.size_buffer(nperseg, window, sc.SIZE_SEEDS[(nperseg, window, cal)])
    p = oracle.ExtractParams(calibration_db=cal)
    half = (len(x) // 2) // nperseg * nperseg
    _, t0, s0 = oracle.stft_power(x[:half], sc.FS, window, nperseg)
    _, t1, s1 = oracle.stft_power(x[half:], sc.FS, window, nperseg)
    found = 0
    for spec, last, times in ((s0, None, t0), (s1, s0, t1)):
        want = oracle.extract_records(times, spec, last, p)
        base.check(both(hc, spec, last, p, nperseg, float(sc.FS), np.random.default_rng(nperseg)), want, cal)
        found += len(want)
    assert found >= 1


def test_twins_on_straddling_pulses(hc):
    """Plateaus that reach into the previous buffer (with and without hot cells there), one that runs into the buffer's end."""
    nperseg, n = 256, 256 * 100
    x = sc.noise(2 * n, 1) + sc.tone(2 * n, nperseg, 40, 96, 10) + sc.tone(2 * n, nperseg, 90, 194, 6) + sc.tone(2 * n, nperseg, 7, 100, 9)
    p = oracle.ExtractParams()
    _, t0, s0 = oracle.stft_power(x[:n], sc.FS, "hamming", nperseg)
    _, t1, s1 = oracle.stft_power(x[n:], sc.FS, "hamming", nperseg)
    w0, w1 = oracle.extract_records(t0, s0, None, p), oracle.extract_records(t1, s1, s0, p)
    assert {(7, -1, 9), (40, -5, 6)} <= {(w.fi, w.start, w.end) for w in w1}
    base.check(both(hc, s0, None, p), w0)
    base.check(both(hc, s1, s0, p), w1)
    # a previous buffer of four columns: the plateau that reached five columns back stops at that buffer's edge (start_min, analyze.py:383)
    short = np.ascontiguousarray(s0[:, -4:])
    w2 = oracle.extract_records(t1, s1, short, p)
    assert (40, -3, 6) in {(w.fi, w.start, w.end) for w in w2}
    base.check(both(hc, s1, short, p), w2)


def test_twins_on_planted_maps(hc):
    """tests/golden/extract_cases.npz widened to float64: cells one ulp either side of the threshold, previous buffers shorter
    than the current one, no previous buffer."""
    index = gu.extract_index()
    found = back = 0
    for i in range(len(index)):
        c = gu.extract_case(i)
        kw = c["kwargs"]
        p = oracle.ExtractParams(kw["signal_threshold_dbw"], kw["snr_threshold_db"], kw["signal_min_duration_ms"],
                                 kw["signal_max_duration_ms"], kw["calibration_db"])
        spec = c["cur"].astype(np.float64)
        last = c["last"].astype(np.float64) if c["has_last"] and c["last"].shape[1] > 0 else None
        if spec.shape[1] < 2:
            continue
        want = oracle.extract_records(c["times"], spec, last, p)
        base.check(both(hc, spec, last, p, 256, float(kw["sample_rate"]), np.random.default_rng(i)), want, p.calibration_db)
        found += len(want)
        back += sum(w.start < 0 for w in want)
    assert found > 100 and back > 0


def test_twins_on_nan_cells(hc):
    """A NaN column (what one NaN sample makes of its segment), NaN cells inside and beside a plateau, a NaN in the previous
    buffer: the two twins agree byte for byte, NaN row means included."""
    nperseg, n = 256, 256 * 60
    x = sc.noise(2 * n, 5) + sc.tone(2 * n, nperseg, 30, 20, 14) + sc.tone(2 * n, nperseg, 99, 56, 12) + sc.tone(2 * n, nperseg, 150, 70, 14)
    p = oracle.ExtractParams()
    _, t0, s0 = oracle.stft_power(x[:n], sc.FS, "hamming", nperseg)
    _, t1, s1 = oracle.stft_power(x[n:], sc.FS, "hamming", nperseg)
    total = 0
    for variant in range(4):
        a, b = s0.copy(), s1.copy()
        if variant == 0:
            b[:, 40] = np.nan          # a whole segment: every row mean is NaN
        elif variant == 1:
            b[150, 15] = np.nan        # inside a plateau (segments 10 .. 23 of the second buffer)
            b[30, 3] = np.nan
        elif variant == 2:
            a[99, 58] = np.nan         # in the previous buffer, inside the plateau that crosses the cut
        else:
            b[7, 0] = np.nan
            b[8, b.shape[1] - 1] = np.nan
        for spec, last, times in ((a, None, t0), (b, a, t1)):
            rec = both(hc, spec, last, p, rng=np.random.default_rng(variant))
            with np.errstate(all="ignore"):
                base.check(rec, oracle.extract_records(times, spec, last, p))
            total += len(rec)
    assert total >= 8
