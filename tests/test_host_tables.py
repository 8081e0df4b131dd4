"""CPU tests of what a handle hands its kernels at creation: the geometry (csrc/rt_core.h: look-back columns, chunk length,
kernel family) and the tables (csrc/rt_tables.h: twiddles, window orders, the window's three-bin fit, Bluestein's tables).

The functions rt_create / rt_create_f64 call are compiled for the host (_rt_hostcheck.so, tests only) and every entry is
checked against its definition, stated here in NumPy from the kernels' comments -- each kernel family reads its tables in a
layout of its own, and host and kernel must agree on it.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from oracle import analyze_oracle as oracle
from pyradiotracking_amd import build

LD = np.longdouble
PI = LD("3.141592653589793238462643383279502884")
BLOCK = 256  # threads of a scan workgroup (rt_kernels.h: scan_block)


@pytest.fixture(scope="module")
def hc():
    assert np.finfo(LD).eps <= 2.0 ** -63, "the definitions below need an extended-precision long double"
    lib = C.CDLL(build.build_hostcheck())
    vp, i, d, f = C.c_void_p, C.c_int, C.c_double, C.c_float
    lib.hc_tail_cols.argtypes = [i, d, d]
    lib.hc_scan_family.argtypes = [i, vp]
    lib.hc_scan_family.restype = None
    lib.hc_choose_chunk.argtypes = [i, i, d, d, i, i, i]
    lib.hc_min_run_cells.argtypes = [i, d, d]
    lib.hc_min_run_cells.restype = C.c_longlong
    lib.hc_scan_twiddles.argtypes = [i, i, i, i, i, vp, vp, vp]
    lib.hc_scaled_window.argtypes = [vp, i, f, vp]
    lib.hc_window_thread_order.argtypes = [vp, i, i, vp]
    lib.hc_window_lane_order.argtypes = [vp, i, i, i, vp]
    lib.hc_fit_cosine_window.argtypes = [vp, i, vp, vp]
    lib.hc_transform_twiddles_f32.argtypes = [i, vp]
    lib.hc_transform_twiddles_f64.argtypes = [i, vp]
    lib.hc_bluestein_tables_f32.argtypes = [vp, i, i, i, f, vp, vp]
    lib.hc_bluestein_tables_f64.argtypes = [vp, i, i, i, vp, vp]
    return lib


def _family(hc, nperseg):
    out = np.zeros(6, np.int32)
    hc.hc_scan_family(nperseg, out.ctypes.data)
    return tuple(int(v) for v in out)  # R3, QS, big, general, bluestein, supported


def _unit(e, n):
    """exp(-2 pi i e / n) in long double, the exponent reduced in integers: (re, im)"""
    e = np.asarray(e, dtype=np.int64) % n
    ang = -2 * PI * e.astype(LD) / LD(n)
    return np.cos(ang), np.sin(ang)


def _check_twiddles(got, e, n, tol):
    """got [..., 2] against exp(-2 pi i e / n): within tol per component, exponent 0 exactly (1, 0)"""
    e = np.asarray(e, dtype=np.int64)
    assert got.shape == e.shape + (2,)
    re, im = _unit(e, n)
    assert np.max(np.abs(got[..., 0].astype(LD) - re)) <= tol
    assert np.max(np.abs(got[..., 1].astype(LD) - im)) <= tol
    zero = (e % n) == 0
    assert zero.any()
    assert np.all(got[zero, 0] == 1.0) and np.all(got[zero, 1] == 0.0)


def _scan_twiddles(hc, N, wave64):
    R3, QS, big = _family(hc, N)[:3]
    n = np.zeros(2, np.int32)
    hc.hc_scan_twiddles(N, R3, QS, big, int(wave64), None, None, n.ctypes.data)
    tw1, tw2 = np.zeros((n[0], 2), np.float32), np.zeros((n[1], 2), np.float32)
    hc.hc_scan_twiddles(N, R3, QS, big, int(wave64), tw1.ctypes.data, tw2.ctypes.data, n.ctypes.data)
    return tw1, tw2


def x1_rotation(R3, b):
    """column rotation of exchange 1 (rt_kernels.h, "Exchange layouts"): s1(b) = (16 / R3 - 2) * b mod 16"""
    return ((16 // R3 - 2) * b) % 16


F32_TOL = 2.0 ** -24  # half a float32 spacing at 1; the argument's error in double precision is nine orders below it
F64_TOL = 2.0 ** -53


# ---- twiddles ----

@pytest.mark.parametrize("N", [256, 512, 1024, 2048, 4096])
def test_scan_twiddles_of_the_fused_scans(hc, N):
    """stft_scan, nperseg 256 R3 (rt_kernels.h: StftParams::tw1 / tw2): tw1 [LG][16] = W_N^(a k1), LG = 16 R3 lanes; tw2 [R3][16] =
    W_LG^(b q1) times the phase W16^(-s q1) that undoes the rotation s = x1_rotation(b) of exchange 1, together W_LG^((b - s R3) q1)"""
    R3, LG = N // 256, N // 16
    assert _family(hc, N) == (R3, 0, 0, 0, 0, 1)
    tw1, tw2 = _scan_twiddles(hc, N, wave64=False)
    a, k1 = np.meshgrid(np.arange(LG), np.arange(16), indexing="ij")
    _check_twiddles(tw1.reshape(LG, 16, 2), a * k1, N, F32_TOL)
    b, q1 = np.meshgrid(np.arange(R3), np.arange(16), indexing="ij")
    s = np.array([x1_rotation(R3, int(v)) for v in range(R3)])[b]
    _check_twiddles(tw2.reshape(R3, 16, 2), (b - s * R3) * q1, LG, F32_TOL)
    # the same table as the unrotated W_LG^(b q1) with the rotation's phase W_16^(-s q1) multiplied on
    re, im = _unit(b * q1 * 16 - s * q1 * LG, LG * 16)
    assert np.max(np.abs(tw2.reshape(R3, 16, 2)[..., 0] - re)) <= F32_TOL and np.max(np.abs(tw2.reshape(R3, 16, 2)[..., 1] - im)) <= F32_TOL


@pytest.mark.parametrize("N", [32, 64, 128])
def test_scan_twiddles_of_the_short_lane_groups(hc, N):
    """stft_scan<1, .., QS>, nperseg 16 QS: register r = e QS + k1 of lane a holds A[n' = (16 / QS) a + e][k1] and takes W_N^(n' k1):
    tw1 [QS][16], entry [a][r]; tw2 [1][16] is all ones (one lane group row, no rotation)"""
    QS = N // 16
    assert _family(hc, N) == (1, QS, 0, 0, 0, 1)
    tw1, tw2 = _scan_twiddles(hc, N, wave64=False)
    a, r = np.meshgrid(np.arange(QS), np.arange(16), indexing="ij")
    _check_twiddles(tw1.reshape(QS, 16, 2), ((16 // QS) * a + r // QS) * (r % QS), N, F32_TOL)
    _check_twiddles(tw2.reshape(1, 16, 2), np.zeros((1, 16), np.int64), QS, F32_TOL)


def test_scan_twiddles_of_the_one_wave_scan(hc):
    """stft_scan64, nperseg 4096 (rt_scan64.h): tw1 [16][64], lane l: rows 0..6 W_N^(8 l d), d = 1..7; rows 7..13 W_N^(l c), c = 1..7;
    rows 14 and 15 unused, (1, 0).  tw2 as for stft_scan<16> (lane groups of 256)."""
    N = 4096
    tw1, tw2 = _scan_twiddles(hc, N, wave64=True)
    lane = np.arange(64)[None, :]
    row = np.arange(16)[:, None]
    e = np.where(row < 7, 8 * lane * (row + 1), np.where(row < 14, lane * (row - 6), 0))
    _check_twiddles(tw1.reshape(16, 64, 2), e, N, F32_TOL)
    assert np.all(tw1.reshape(16, 64, 2)[14:] == np.array([1.0, 0.0], np.float32))
    assert tw2.tobytes() == _scan_twiddles(hc, N, wave64=False)[1].tobytes()


@pytest.mark.parametrize("N", [8192, 16384])
def test_scan_twiddles_of_the_workgroup_scan(hc, N):
    """stft_wg, nperseg 8192 / 16 384 (rt_scan_wg.h), BLK = nperseg / 32 threads: tw1 [5][BLK] = W_N^(t 2^i) as [i][t];
    tw2 [BLK / 16][16] = W_BLK^(d p) as [d][p]"""
    BLK = N // 32
    assert _family(hc, N) == (1, 0, BLK, 0, 0, 1)
    tw1, tw2 = _scan_twiddles(hc, N, wave64=False)
    i, t = np.meshgrid(np.arange(5), np.arange(BLK), indexing="ij")
    _check_twiddles(tw1.reshape(5, BLK, 2), t * 2 ** i, N, F32_TOL)
    d, p = np.meshgrid(np.arange(BLK // 16), np.arange(16), indexing="ij")
    _check_twiddles(tw2.reshape(BLK // 16, 16, 2), d * p, BLK, F32_TOL)


@pytest.mark.parametrize("M", [8, 16, 16384])
def test_transform_twiddles_float32(hc, M):
    """the general transform (rt_general.h): W_M^j, j < M / 2"""
    tw = np.zeros((M // 2, 2), np.float32)
    hc.hc_transform_twiddles_f32(M, tw.ctypes.data)
    _check_twiddles(tw, np.arange(M // 2), M, F32_TOL)


@pytest.mark.parametrize("M", [8, 32, 8192])
def test_transform_twiddles_float64(hc, M):
    """a float64 handle's transform (rt_f64.h): W_M^j, j < M / 2, rounded once from long double"""
    tw = np.zeros((M // 2, 2), np.float64)
    hc.hc_transform_twiddles_f64(M, tw.ctypes.data)
    _check_twiddles(tw, np.arange(M // 2), M, F64_TOL)


def test_kernel_family_of_a_size(hc):
    """(R3, QS, big, general, bluestein, supported): which kernels an nperseg runs on"""
    assert _family(hc, 8) == (1, 0, 0, 1, 0, 1)        # the other powers of two: the general transform
    assert _family(hc, 16) == (1, 0, 0, 1, 0, 1)
    assert _family(hc, 12) == (1, 0, 0, 1, 1, 1)       # everything else up to 8192: Bluestein on it
    assert _family(hc, 100) == (1, 0, 0, 1, 1, 1)
    assert _family(hc, 8191) == (1, 0, 0, 1, 1, 1)
    assert _family(hc, 7)[5] == 0 and _family(hc, 0)[5] == 0 and _family(hc, -256)[5] == 0
    assert _family(hc, 8193)[5] == 0 and _family(hc, 32768)[5] == 0


# ---- windows ----

WINDOWS = ["hamming", "hann", "boxcar", "blackmanharris"]
SCALE = np.float32(1.0 / (300000.0 * 93.70))  # (as 1 / (fs * sum(w^2)) would be; anything but 1)


def _window32(name, N):
    return np.ascontiguousarray(oracle.window_coefficients(name, N), dtype=np.float32)


def _scaled(hc, w, scale=SCALE):
    ws = np.zeros(len(w), np.float32)
    hc.hc_scaled_window(w.ctypes.data, len(w), scale, ws.ctypes.data)
    return ws


@pytest.mark.parametrize("name", WINDOWS)
@pytest.mark.parametrize("N", [256, 4096, 8192])
def test_scaled_window_and_its_orders(hc, name, N):
    """ws = float32(float64(w) * sqrt(float64(scale))), and each kernel's order of it as a permutation, bit for bit"""
    w = _window32(name, N)
    ws = _scaled(hc, w)
    assert ws.tobytes() == (w.astype(np.float64) * np.sqrt(np.float64(SCALE))).astype(np.float32).tobytes()
    out = np.zeros(N, np.float32)
    # stft_scan<R3>: [l][16] = window[l + LG m], LG = N / 16 lanes (the product uploads it at nperseg 4096)
    LG = N // 16
    hc.hc_window_lane_order(ws.ctypes.data, N, LG, 0, out.ctypes.data)
    l, m = np.meshgrid(np.arange(LG), np.arange(16), indexing="ij")
    assert out.tobytes() == ws[l + LG * m].tobytes()
    if N == 4096:
        # stft_scan64: 16-byte pieces [n0][jq][lane][e] = window[lane + 64 m], m = n0 + 4 (4 jq + e)
        hc.hc_window_lane_order(ws.ctypes.data, N, 256, 1, out.ctypes.data)
        n0, jq, lane, e = np.meshgrid(np.arange(4), np.arange(4), np.arange(64), np.arange(4), indexing="ij")
        assert out.tobytes() == ws[lane + 64 * (n0 + 4 * (4 * jq + e))].tobytes()
    if N == 8192:
        # stft_wg: thread order [t][32] = window[t + BLK j]
        BLK = N // 32
        hc.hc_window_thread_order(ws.ctypes.data, N, BLK, out.ctypes.data)
        t, j = np.meshgrid(np.arange(BLK), np.arange(32), indexing="ij")
        assert out.tobytes() == ws[t + BLK * j].tobytes()


def _fit(hc, ws):
    wr, wi = np.zeros(3), np.zeros(3)
    ok = hc.hc_fit_cosine_window(ws.ctypes.data, len(ws), wr.ctypes.data, wi.ctypes.data)
    return bool(ok), wr, wi


@pytest.mark.parametrize("N", [256, 4096, 8192])
def test_cosine_fit(hc, N):
    """cosine sums of order <= 1 (hamming, hann, boxcar) qualify for the detrend by linearity, nothing else does; their three
    coefficients W[0] / N, W[1] / N, W[N-1] / N are those of the window's float64 DFT"""
    for name in ("hamming", "hann", "boxcar"):
        ws = _scaled(hc, _window32(name, N))
        ok, wr, wi = _fit(hc, ws)
        assert ok, name
        want = np.fft.fft(ws.astype(np.float64))[[0, 1, N - 1]].real / N
        lin_c = (wr / N).astype(np.float32)
        ulp = np.spacing(np.abs(lin_c[0]))
        assert np.all(np.abs(lin_c.astype(np.float64) - want.astype(np.float32).astype(np.float64)) <= ulp), name
    assert not _fit(hc, _scaled(hc, _window32("blackmanharris", N)))[0]
    bent = _window32("hann", N)
    bent[N // 3] += np.float32(1e-3)
    assert not _fit(hc, _scaled(hc, bent))[0]
    shifted = np.roll(_window32("hann", N), 1)
    ok, wr, wi = _fit(hc, _scaled(hc, shifted))
    assert not ok and abs(wi[1]) > 1e-6 * abs(wr[0])  # (still a cosine sum, but its transform is not real)


# ---- Bluestein's tables ----

def _bluestein_definition(window, N, M, log2m, root):
    """chirp w[n] = exp(-i pi n^2 / N) with n^2 reduced mod 2 N; cwin = window * root * w; the filter conj(w[m]) on -N < m < N
    wrapped to M, its DFT by the direct O(M^2) sum in long double, in bit-reversed order, divided by M.  (re, im) each."""
    n = np.arange(N, dtype=np.int64)
    cr, ci = _unit((n * n) % (2 * N), 2 * N)  # exp(-i pi e / N) = exp(-2 pi i e / (2 N))
    wv = window.astype(LD) * LD(root)
    cwin = (wv * cr, wv * ci)
    br, bi = np.zeros(M, LD), np.zeros(M, LD)
    br[:N], bi[:N] = cr, -ci
    br[M - n[1:]], bi[M - n[1:]] = cr[1:], -ci[1:]
    k, m = np.meshgrid(np.arange(M, dtype=np.int64), np.arange(M, dtype=np.int64), indexing="ij")
    tr, ti = _unit(k * m, M)
    Br = tr @ br - ti @ bi
    Bi = tr @ bi + ti @ br
    rev = np.array([int(format(v, "0%db" % log2m)[::-1], 2) for v in range(M)])
    return cwin, (Br[rev] / M, Bi[rev] / M)


def _within_one_ulp_at_the_largest(got, want, dtype):
    re, im = want
    ulp = LD(np.spacing(dtype(max(np.max(np.abs(re)), np.max(np.abs(im))))))
    assert np.max(np.abs(got[:, 0].astype(LD) - re)) <= ulp
    assert np.max(np.abs(got[:, 1].astype(LD) - im)) <= ulp


@pytest.mark.parametrize("N,M", [(12, 32), (100, 256)])
@pytest.mark.parametrize("name", ["hamming", "blackmanharris"])
def test_bluestein_tables_float32(hc, N, M, name):
    log2m = M.bit_length() - 1
    w = _window32(name, N)
    cwin, bfilt = np.zeros((N, 2), np.float32), np.zeros((M, 2), np.float32)
    hc.hc_bluestein_tables_f32(w.ctypes.data, N, M, log2m, SCALE, cwin.ctypes.data, bfilt.ctypes.data)
    want_cwin, want_bfilt = _bluestein_definition(w, N, M, log2m, np.sqrt(np.float64(SCALE)))
    _within_one_ulp_at_the_largest(cwin, want_cwin, np.float32)
    _within_one_ulp_at_the_largest(bfilt, want_bfilt, np.float32)


@pytest.mark.parametrize("N,M", [(12, 32), (100, 256)])
@pytest.mark.parametrize("name", ["hamming", "blackmanharris"])
def test_bluestein_tables_float64(hc, N, M, name):
    """a float64 handle: the float64 window as it is (root = 1; the powers are scaled in the kernel), tables rounded from long double"""
    log2m = M.bit_length() - 1
    w = np.ascontiguousarray(oracle.window_coefficients(name, N), dtype=np.float64)
    cwin, bfilt = np.zeros((N, 2), np.float64), np.zeros((M, 2), np.float64)
    hc.hc_bluestein_tables_f64(w.ctypes.data, N, M, log2m, cwin.ctypes.data, bfilt.ctypes.data)
    want_cwin, want_bfilt = _bluestein_definition(w, N, M, log2m, 1.0)
    _within_one_ulp_at_the_largest(cwin, want_cwin, np.float64)
    _within_one_ulp_at_the_largest(bfilt, want_bfilt, np.float64)


# ---- geometry ----

def _hop(nperseg, fs):
    times = np.arange(nperseg / 2, 50 * nperseg + 17 - nperseg / 2 + 1, nperseg) / float(fs)  # (scipy's segment times)
    return times[1] - times[0]


@pytest.mark.parametrize("nperseg,fs", [(256, 300000), (256, 2048000), (1024, 2400000), (4096, 3200000), (256, 1000000)])
def test_tail_cols(hc, nperseg, fs):
    """K = floor(max duration / hop) + 2 look-back columns, at most 1e6, at least 1"""
    hop = _hop(nperseg, fs)
    for max_d in (0.0, 0.04, 0.08, 0.1, 1.0, 7.3, 3 * hop, 3 * hop * (1 - 1e-16), 1e9, 1e300):
        want = max(1, int(min(np.floor(max_d / hop) + 2.0, 1.0e6)))
        assert hc.hc_tail_cols(nperseg, float(fs), max_d) == want, max_d
    assert hc.hc_tail_cols(nperseg, float(fs), 0.0) == 2
    assert hc.hc_tail_cols(nperseg, float(fs), 1e9) == 1000000


def test_min_run_cells(hc):
    """a run of fewer cells fails the duration gate unless it runs through t = 0: ceil(min duration (1 - 1e-9) / hop) - 1"""
    for nperseg, fs in [(256, 300000), (256, 2048000), (1024, 2400000), (4096, 3200000)]:
        hop = _hop(nperseg, fs)
        for min_d in (0.0, 0.001, 0.008, 0.017, 64 * hop, 1.0, 1e12):
            want = int(np.ceil(min(min_d * (1.0 - 1e-9) / hop, 1.0e9))) - 1
            assert hc.hc_min_run_cells(nperseg, float(fs), min_d) == want
    assert [hc.hc_key_tbits(n) for n in (0, 1, 2, 3, 4, 5, 1024, 1025)] == [1, 1, 1, 2, 2, 3, 10, 11]
    assert [hc.hc_next_pow2(n) for n in (0, 1, 2, 3, 64, 65, 1171)] == [1, 1, 2, 4, 64, 128, 2048]


# (nperseg, fs, min duration s, forced segs_per_chunk, n_streams, n_seg) -> segments per chunk.  The values are those of choose_chunk
# as it stood in rt_analyze.hip before it moved to rt_core.h (computed from that function, not from the moved one).
CHUNKS = [
    ((256, 300000, 0.008, 0, 4096, 1171), 25),   # the reference's default geometry, a batch that fills the chip
    ((256, 2048000, 0.008, 0, 256, 8000), 32),   # chunk bits exist (8 ms = 64 hops: keep_long), the chunks stay 32 long
    ((256, 2048000, 0.008, 0, 4, 8000), 32),     # ... for a small batch too
    ((256, 2048000, 0.008, 0, 4096, 8000), 32),
    ((256, 300000, 0.008, 0, 4, 1171), 4),       # a small batch without chunk bits: halved down to 4
    ((256, 2048000, 0.008, 0, 4096, 63), 20),    # too short a buffer for keep_long (n_seg < 64)
    ((512, 300000, 0.008, 0, 4096, 585), 25),
    ((4096, 3200000, 0.008, 0, 1024, 781), 71),  # 11 chunks, none short
    ((4096, 3200000, 0.008, 0, 4096, 781), 71),
    ((4096, 3200000, 0.008, 0, 8, 781), 4),
    ((1024, 2400000, 0.008, 0, 4096, 2343), 37),  # clears the eight-round cut-off of the search
    ((1024, 2400000, 0.008, 0, 128, 2343), 32),   # fills the chip (no halving) but not eight rounds: stays 32
    ((1024, 2400000, 0.008, 0, 16, 2343), 4),
    ((2048, 2400000, 0.008, 0, 4096, 1000), 72),
    ((2048, 2400000, 0.008, 0, 512, 1000), 42),   # the cut-off ends the search before 72
    ((2048, 2400000, 0.008, 0, 128, 1000), 32),
    ((8192, 2400000, 0.008, 0, 1024, 390), 39),   # stft_wg: 40, evened out over 10 chunks
    ((8192, 2400000, 0.008, 0, 4, 390), 8),
    ((16384, 2400000, 0.008, 0, 1024, 195), 39),
    ((128, 300000, 0.008, 0, 4096, 2343), 25),
    ((128, 300000, 0.008, 0, 4, 2343), 4),
    ((64, 300000, 0.008, 0, 4096, 4687), 25),
    ((64, 300000, 0.008, 0, 4, 4687), 4),
    ((32, 300000, 0.008, 0, 4096, 9375), 32),     # 8 ms are 75 hops of 32 samples: keep_long
    ((32, 300000, 0.008, 0, 4, 9375), 32),
    ((1024, 2400000, 0.05, 0, 4, 2343), 32),      # keep_long at nperseg 1024 (50 ms = 117 hops)
    ((1024, 2400000, 0.05, 0, 4096, 2343), 32),
    ((100, 300000, 0.008, 0, 4096, 3000), 27),    # a general size: sized as nperseg 256 (its scratch is not used)
    ((256, 300000, 0.008, 13, 4096, 1171), 13),   # forced
    ((8192, 2400000, 0.008, 13, 4, 390), 13),
]


def _chunk(hc, nperseg, fs, min_d, forced, n_streams, n_seg):
    return hc.hc_choose_chunk(nperseg, BLOCK, float(fs), min_d, forced, n_streams, n_seg)


@pytest.mark.parametrize("case,want", CHUNKS)
def test_choose_chunk(hc, case, want):
    assert _chunk(hc, *case) == want


@pytest.mark.parametrize("nperseg,fs,n_streams,n_seg", [
    (256, 300000, 1000, 1171),   # the halving for batches that do not fill the chip
    (1024, 2400000, 256, 2343),  # the "at least eight rounds" cut-off of the nperseg >= 1024 search
])
def test_choose_chunk_depends_on_the_number_of_streams(hc, nperseg, fs, n_streams, n_seg):
    """The chunk length sets the order in which a row's partial sums are added.  It depends on the number of streams in two places,
    so the halves of a batch agree with the whole only if they ask with the whole batch's count -- or are handed its answer as a
    forced length, which is what a laned handle does for its lanes."""
    whole = _chunk(hc, nperseg, fs, 0.008, 0, n_streams, n_seg)
    half = _chunk(hc, nperseg, fs, 0.008, 0, n_streams // 2, n_seg)
    assert half != whole
    assert _chunk(hc, nperseg, fs, 0.008, whole, n_streams // 2, n_seg) == whole
