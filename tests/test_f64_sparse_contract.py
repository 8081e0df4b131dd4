"""The map-free float64 path (RT_FLAG_F64_SPARSE) without a GPU: the argument checks of rt_create / rt_create_f64 before any
device is touched, the keyword, the host-side geometry (rt_core.h), and the sufficiency of the scan's emission rule -- the cell
list built by the rule in NumPy, through the sequential twin of the detection (hc_extract_sparse_f64), gives the oracle's
records."""
import ctypes as C

import numpy as np
import pytest

from oracle import analyze_oracle as oracle
from pyradiotracking_amd import _native, build
from pyradiotracking_amd.analyze import BatchSignalAnalyzer, SignalAnalyzer
from tests import f64_sparse_cases as sc
from tests import float64_cases as fc
from tests import golden_util as gu

DB_TOL = 1e-9   # max / avg / noise / snr, dB  (tests/test_gpu_float64_path.py)
STD_TOL = 1e-5  # std, dB
F64_SPARSE = 64


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
    h.hc_f64_cell_key.restype = C.c_uint
    h.hc_f64_key_bin.argtypes = h.hc_f64_key_seg.argtypes = [C.c_uint]
    return h


# ---- (a) create-time checks ----
def _create(lib, f64=True, nperseg=256, mode=_native.RT_MODE_AUTO, flags=F64_SPARSE, hot_capacity=0, lanes=1, max_samples=1 << 16):
    cfg = _native.RtConfig()
    cfg.n_streams, cfg.nperseg, cfg.mode, cfg.max_samples, cfg.sample_rate = 1, nperseg, mode, max_samples, 300000.0
    cfg.min_duration_s, cfg.max_duration_s, cfg.lanes, cfg.flags, cfg.hot_capacity = 0.008, 0.04, lanes, flags, hot_capacity
    w = np.hamming(max(nperseg, 8))
    w32 = w.astype(np.float32)
    h = C.c_void_p()
    if f64:
        c64 = _native.RtConfigF64()
        c64.window = w.ctypes.data_as(C.POINTER(C.c_double))
        c64.scale, c64.threshold, c64.snr_threshold = 1.0, 1e-9, 3.0
        rc = lib.rt_create_f64(C.byref(cfg), C.byref(c64), C.byref(h))
    else:
        cfg.window = w32.ctypes.data_as(C.POINTER(C.c_float))
        cfg.scale, cfg.threshold, cfg.snr_threshold = 1.0, 1e-9, 3.0
        rc = lib.rt_create(C.byref(cfg), C.byref(h))
    msg = lib.rt_last_error(None).decode()
    if rc == _native.RT_OK:
        lib.rt_destroy(h)
    return rc, msg


def test_flag_value():
    assert _native.RT_FLAG_F64_SPARSE == F64_SPARSE


REFUSALS = [
    (dict(f64=False), _native.RT_E_INVALID),
    (dict(mode=_native.RT_MODE_DENSE), _native.RT_E_INVALID),
    (dict(mode=_native.RT_MODE_SPARSE), _native.RT_E_INVALID),
    (dict(mode=_native.RT_MODE_PREFILTER), _native.RT_E_INVALID),
    (dict(mode=_native.RT_MODE_RUNFILTER), _native.RT_E_INVALID),
    (dict(nperseg=8), _native.RT_E_UNSUPPORTED),
    (dict(nperseg=16), _native.RT_E_UNSUPPORTED),
    (dict(nperseg=300), _native.RT_E_UNSUPPORTED),
    (dict(nperseg=1000), _native.RT_E_UNSUPPORTED),
    (dict(nperseg=8192), _native.RT_E_UNSUPPORTED),
    (dict(nperseg=16384), _native.RT_E_UNSUPPORTED),
    (dict(flags=F64_SPARSE | _native.RT_FLAG_RECORD_CELLS), _native.RT_E_UNSUPPORTED),
    (dict(hot_capacity=1023), _native.RT_E_INVALID),
    (dict(hot_capacity=8193), _native.RT_E_INVALID),
    (dict(hot_capacity=-1), _native.RT_E_INVALID),
    (dict(lanes=2), _native.RT_E_UNSUPPORTED),
    (dict(nperseg=32, max_samples=32 * ((1 << 20) + 1)), _native.RT_E_UNSUPPORTED),
]


@pytest.mark.parametrize("kw,status", REFUSALS, ids=[str(sorted(k.items())) for k, _ in REFUSALS])
def test_create_refusals(lib, kw, status):
    rc, msg = _create(lib, **kw)
    assert rc == status, (kw, rc, msg)
    assert "float64" in msg, (kw, msg)


@pytest.mark.parametrize("kw", [dict(), dict(nperseg=32), dict(nperseg=4096), dict(hot_capacity=1024), dict(hot_capacity=8192),
                                dict(flags=F64_SPARSE | _native.RT_FLAG_ROW_MEANS | _native.RT_FLAG_TIMING),
                                dict(nperseg=32, max_samples=32 << 20)])
def test_valid_arguments_reach_the_device(lib, kw):
    """On a box without a GPU the flag with valid arguments fails with RT_E_NO_DEVICE: every argument check has passed."""
    n = C.c_int(0)
    lib.rt_device_count(C.byref(n))
    rc, msg = _create(lib, **kw)
    assert rc == (_native.RT_OK if n.value > 0 else _native.RT_E_NO_DEVICE), (kw, rc, msg)


def test_keyword():
    for cls, args in ((BatchSignalAnalyzer, (["0"],)), (SignalAnalyzer, ("0",))):
        with pytest.raises(ValueError):
            cls(*args, f64_sparse=True)  # precision="float32"
        with pytest.raises(ValueError):
            cls(*args, precision="float64", f64_sparse=True, mode="dense")
        with pytest.raises(ValueError):
            cls(*args, precision="float64", f64_sparse=True, record_cells=True)
    if _native.device_count() < 1:
        with pytest.raises(_native.NativeError) as ei:
            BatchSignalAnalyzer(["0"], precision="float64", f64_sparse=True, sdr_callback_length=4096)
        assert ei.value.code == _native.RT_E_NO_DEVICE


# ---- (c) host geometry ----
def test_chunk_geometry(hc):
    for nperseg in sc.SIZES:
        g = hc.hc_f64_sparse_group(nperseg)
        assert g == max(1, min(32, 1024 // nperseg)) and 256 % g == 0 and nperseg * g % 256 == 0
        assert nperseg * g // 256 in (4, 8, 16)  # the scan kernel's instantiations
        t_max = min(hc.hc_f64_key_max_seg(), (1 << 31) // nperseg)
        for spc, n_streams in ((0, 1), (0, 16), (0, 4096), (3, 1), (4, 14), (71, 2)):
            L = hc.hc_f64_sparse_chunk(nperseg, spc, n_streams, t_max)
            assert L >= 1 and (spc == 0 or L == spc)
            if spc == 0:
                assert (L + 1) % min(g, L + 1) == 0  # the chunk and its halo segment: whole groups
            for T in sorted({2, max(2, L - 1), L, L + 1, 2 * L + 1, t_max}):
                chunks, last = hc.hc_f64_sparse_chunks(T, L), hc.hc_f64_sparse_last_chunk(T, L)
                assert chunks == -(-T // L) and 1 <= last <= L and (chunks - 1) * L + last == T, (nperseg, L, T)
    assert hc.hc_f64_sparse_chunks(0, 31) == 0 and hc.hc_f64_sparse_last_chunk(0, 31) == 0
    # a handle's chunk length comes from its largest call, not from the call at hand: small batches get short chunks
    assert hc.hc_f64_sparse_chunk(256, 0, 4096, 1171) == 31
    assert hc.hc_f64_sparse_chunk(256, 0, 1, 64) < 31


def test_key_round_trip(hc):
    t_max = hc.hc_f64_key_max_seg()
    assert t_max == 1 << 20
    keys = []
    for fi in (0, 1, 31, 2047, 4095):
        for t in (0, 1, t_max - 2, t_max - 1):  # the largest T the create check admits: segments 0 .. 2^20 - 1
            k = hc.hc_f64_cell_key(fi, t)
            assert (hc.hc_f64_key_bin(k), hc.hc_f64_key_seg(k)) == (fi, t)
            keys.append(((fi, t), k))
    assert [k for _, k in sorted(keys)] == sorted(k for _, k in keys)  # key order = (bin, segment) order
    assert len({k for _, k in keys}) == len(keys)


def test_hot_capacity_bounds(hc):
    assert hc.hc_f64_sparse_hot_capacity(0) == 4096
    for v in (1024, 4096, 5000, 8192):
        assert hc.hc_f64_sparse_hot_capacity(v) == v
    for v in (-1, 1, 1023, 8193, 1 << 20):
        assert hc.hc_f64_sparse_hot_capacity(v) == -1
    for n, ok in ((16, 0), (32, 1), (48, 0), (256, 1), (4096, 1), (8192, 0), (0, 0)):
        assert hc.hc_f64_sparse_nperseg_ok(n) == ok


# ---- (b) the emission rule is sufficient ----
def emit_cells(spec_tf, thr, rng=None):
    """The scan's rule on a [T][F] map: cell (fi, t) iff not (P < thr), or cell (fi, t + 1) is.  Returns (keys, powers)."""
    hot = ~(spec_tf < thr)
    need = hot.copy()
    need[:-1] |= hot[1:]
    t, fi = np.nonzero(need)
    keys = (fi.astype(np.uint32) << np.uint32(20)) | t.astype(np.uint32)
    vals = spec_tf[t, fi].astype(np.float64)
    if rng is not None:
        order = rng.permutation(len(keys))
        keys, vals = keys[order], vals[order]
    return np.ascontiguousarray(keys), np.ascontiguousarray(vals)


def sparse_records(hc, spec_ft, last_ft, p, nperseg=256, fs=300000.0, rng=None):
    """hc_extract_sparse_f64 on the rule's list of one [F][T] map, the true row sums and the previous map as the tail."""
    cur = np.ascontiguousarray(np.asarray(spec_ft, dtype=np.float64).T)  # [T][F]
    n_seg, n_bins = cur.shape
    keys, vals = emit_cells(cur, p.signal_threshold, rng)
    # the true row sums: np.mean(row)'s own sum (analyze.py:375), so that sum / T is the oracle's row mean to the bit
    sums = np.array([np.add.reduce(np.asarray(row, dtype=np.float64)) for row in spec_ft], dtype=np.float64)
    dptr = C.POINTER(C.c_double)
    last = None if last_ft is None else np.ascontiguousarray(np.asarray(last_ft, dtype=np.float64).T)
    n_last = 0 if last is None else last.shape[0]
    out = np.zeros(8192, dtype=_native.RECORD_F64_DTYPE)
    n = hc.hc_extract_sparse_f64(keys.ctypes.data, vals.ctypes.data_as(dptr), len(keys), sums.ctypes.data_as(dptr), n_seg, n_bins,
                                 None if last is None else last.ctypes.data_as(dptr), n_last, n_last, nperseg, fs, p.signal_threshold,
                                 p.snr_threshold, p.calibration_db, p.signal_min_duration, p.signal_max_duration, out.ctypes.data, len(out))
    assert n <= len(out)
    return out[:n], len(keys)


def check(rec, want, cal=0.0):
    sig = oracle.records_to_signals(want, np.zeros(8192), fc.TS0, "0", 0.0)
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


@pytest.mark.parametrize("nperseg,window,cal", [c for c in sc.SIZE_CASES if c[0] in (32, 256, 2048)])
@pytest.mark.parametrize("shuffle", [False, True])
def test_rule_on_oracle_maps(hc, nperseg, window, cal, shuffle):
    x = sc.size_buffer(nperseg, window, sc.SIZE_SEEDS[(nperseg, window, cal)])
    p = oracle.ExtractParams(calibration_db=cal)
    half = (len(x) // 2) // nperseg * nperseg  # two consecutive buffers: look-back plateaus where a pulse straddles the cut
    _, t0, s0 = oracle.stft_power(x[:half], sc.FS, window, nperseg)
    _, t1, s1 = oracle.stft_power(x[half:], sc.FS, window, nperseg)
    rng = np.random.default_rng(nperseg) if shuffle else None
    for spec, last, times in ((s0, None, t0), (s1, s0, t1)):
        want = oracle.extract_records(times, spec, last, p)
        got, n_cells = sparse_records(hc, spec, last, p, nperseg, float(sc.FS), rng)
        assert n_cells < spec.size // 8  # (the list is a small part of the map)
        check(got, want, cal)


def test_rule_on_straddling_pulses(hc):
    """A plateau whose first hot cell is t = 0 continues one of the previous buffer; one that reaches the buffer's end is skipped."""
    nperseg, n = 256, 256 * 100
    x = sc.noise(2 * n, 1) + sc.tone(2 * n, nperseg, 40, 96, 10) + sc.tone(2 * n, nperseg, 90, 194, 6) + sc.tone(2 * n, nperseg, 7, 100, 9)
    p = oracle.ExtractParams()
    _, t0, s0 = oracle.stft_power(x[:n], sc.FS, "hamming", nperseg)
    _, t1, s1 = oracle.stft_power(x[n:], sc.FS, "hamming", nperseg)
    rng = np.random.default_rng(2)
    w0, w1 = oracle.extract_records(t0, s0, None, p), oracle.extract_records(t1, s1, s0, p)
    got1 = {(w.fi, w.start, w.end) for w in w1}  # (the window's main lobe: the neighbouring bins too)
    assert {(7, -1, 9), (40, -5, 6)} <= got1  # first hot cell t = 0: without and with hot cells before it
    assert 40 not in [w.fi for w in w0]  # (reaches the first buffer's end)
    assert 90 not in [w.fi for w in w1] and s1[90, -1] > p.signal_threshold  # (runs into the second buffer's end)
    check(sparse_records(hc, s0, None, p, rng=rng)[0], w0)
    check(sparse_records(hc, s1, s0, p, rng=rng)[0], w1)


def test_rule_on_planted_maps(hc):
    """The planted maps of tests/golden/extract_cases.npz, widened to float64 (cells one ulp either side of the threshold
    included: the widening is exact and the row sums are the oracle's, so no decision is near a rounding)."""
    index = gu.extract_index()
    assert len(index) == 160
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
        got, _ = sparse_records(hc, spec, last, p, 256, float(kw["sample_rate"]), np.random.default_rng(i))
        check(got, want, p.calibration_db)
        found += len(want)
        back += sum(w.start < 0 for w in want)
    assert found > 100 and back > 0
