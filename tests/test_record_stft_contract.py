"""rt_fetch_record_stft without a GPU: the float64 model of a value is SciPy's ``mode='complex'`` spectrogram; the NumPy restatement
of record_stft's summation order stays inside the bound and four planted mistakes leave it (tests/record_stft_cases.py); the
pulse-pair arithmetic of ``fetch_record_fine``; the entries' argument checks through the loaded library; the host work list, the
twiddle table and sqrt(scale) through ``rt_hostcheck`` against NumPy, and the work list as a stand-alone program under
AddressSanitizer and UBSan (tests/c/stft_work.cpp)."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.signal

from oracle import analyze_oracle as oracle
from pyradiotracking_amd import _native, build
from pyradiotracking_amd.analyze import FINE_DTYPE, record_fine
from tests import precision64 as p64
from tests import record_stft_cases as rs
from tests import sequence_cases as sq

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = sq.FS
SIZES = (32, 256, 300, 1024)
WINDOWS = ("hamming", "hann", ("kaiser", 8.0))
DC = 0.4 - 0.3j
N_SEG = 12


def _bins(N):
    return (0, 1, N - 1, N // 2, N - N // 3)  # DC, +-1, Nyquist, a negative-frequency bin


def _input(N, fi, seed, dc=DC):
    """complex64 [N_SEG * N]: noise, a tone 0.3 bins over bin fi's centre, a DC offset"""
    rng = np.random.default_rng([seed, N, fi])
    n = np.arange(N_SEG * N)
    x = (rng.standard_normal(n.size) + 1j * rng.standard_normal(n.size)) * 0.012 + 0.25 * np.exp(2j * np.pi * (fi + 0.3) * n / N) + dc
    return x.astype(np.complex64)


def _setup(window, N):
    return rs.window32(window, N), p64.scale_f32(window, N, FS)


@pytest.mark.parametrize("window", WINDOWS, ids=lambda w: w if isinstance(w, str) else "kaiser8")
@pytest.mark.parametrize("N", SIZES)
def test_the_model_is_scipys_complex_spectrogram(N, window):
    """SciPy's own complex64 result lies inside the bound (its worst ratio over these cases is 0.26); on the same samples in
    complex128 SciPy and the model agree to 1e-12 of the segment's norm; and |value|^2 is the power map's cell."""
    w, scale = _setup(window, N)
    for fi in _bins(N):
        x = _input(N, fi, 1)
        q = rs.model_values(x, fi, w, scale, N)
        _, _, Z = scipy.signal.spectrogram(x, FS, window, N, noverlap=0, return_onesided=False, mode="complex")
        assert Z.dtype == np.complex64
        r = rs.ratios(Z[fi], q, N, rs.SPP["c64"])
        assert r.max() <= 1.0, (N, window, fi, float(r.max()))
        _, _, Z64 = scipy.signal.spectrogram(x.astype(np.complex128), FS, w.astype(np.float64), N, noverlap=0, return_onesided=False, mode="complex",
                                             scaling="density")
        # (float64 SciPy evaluates its own scale from the float64 window: compare up to that factor)
        own = math.sqrt(1.0 / (FS * float((w.astype(np.float64) ** 2).sum())))
        assert np.abs(Z64[fi] / own * q.root - q.values).max() <= 1e-12 * q.root * q.norm.max() * math.sqrt(N)
        # |value|^2 is the power map's cell
        _, _, P = scipy.signal.spectrogram(x, FS, window, N, noverlap=0, return_onesided=False, mode="psd")
        ref = p64.stft_power_f64(x, FS, window, N)
        assert np.allclose(np.abs(q.values) ** 2, ref.P[:, fi], rtol=1e-12, atol=0)
        assert (np.abs(P[fi] - np.abs(q.values) ** 2) <= 2 * p64.cell_bounds(ref, "sub", "direct" if N & (N - 1) == 0 else "bluestein").dP[:, fi]).all()


@pytest.mark.parametrize("kind", rs.KINDS)
@pytest.mark.parametrize("N", SIZES + (4096,))
def test_the_float32_restatement_stays_inside_the_bound(N, kind):
    w, scale = _setup("hamming", N)
    root = float(np.float32(math.sqrt(scale)))
    rng = np.random.default_rng([11, N])
    for fi in _bins(N):
        x, spp = rs.sweep_input(kind, N, fi, 6, rng)
        q = rs.model_values(x, fi, w, scale, N)
        r = rs.ratios(rs.restate(x, fi, w, root, N, spp), q, N, spp)
        assert r.max() <= 0.5, (N, kind, fi, float(r.max()))  # (the sweep's worst is 0.28: the bound is no tighter than that needs)


@pytest.mark.parametrize("N", (32, 256, 300, 1024))
def test_the_float64_restatement_stays_inside_the_float64_bound(N):
    w = oracle.window_coefficients("hamming", N)
    scale = 1.0 / (FS * float((w ** 2).sum()))
    rng = np.random.default_rng([12, N])
    for fi in _bins(N):
        x, _ = rs.sweep_input("tone_dc", N, fi, 6, rng)
        x = x.astype(np.complex128)
        q = rs.model_values(x, fi, w, scale, N, wide=True)
        r = rs.ratios(rs.restate(x, fi, w, math.sqrt(scale), N, rs.SPP["c128"], np.float64), q, N, rs.SPP["c128"], rs.U64)
        assert r.max() <= 0.5, (N, fi, float(r.max()))


@pytest.mark.parametrize("fault", ["conjugate", "no_detrend", "fi_off_by_one", "scale_not_root"])
@pytest.mark.parametrize("N", (32, 256, 300, 1024))
def test_planted_faults_leave_the_bound(N, fault):
    w, scale = _setup("hamming", N)
    root = float(np.float32(math.sqrt(scale)))
    fi = 1 if fault == "no_detrend" else N - N // 3  # (no detrend: bin 1 under a DC offset, where the window's lobe carries it)
    x = _input(N, fi, 3).reshape(-1, N)
    q = rs.model_values(x, fi, w, scale, N)
    ok = rs.ratios(rs.restate(x, fi, w, root, N, 2), q, N, 2)
    bad = rs.ratios(rs.restate(x, fi, w, root, N, 2, fault=fault), q, N, 2)
    assert ok.max() <= 0.5 and bad.min() > 1.0, (N, fault, float(ok.max()), float(bad.min()))


def test_constant_segments_are_exactly_zero_and_nan_stays_nan():
    for N, spp in ((256, 4), (300, 2), (1024, 8)):
        w, scale = _setup("hamming", N)
        x = np.full((3, N), np.complex64(complex(np.float32(0.3), np.float32(-0.7))))  # (a full-mantissa constant)
        x[1] = np.complex64(32767 / 32768 - 1j)
        x[2, 5] = np.nan
        got = rs.restate(x, 3, w, float(np.float32(math.sqrt(scale))), N, spp)
        assert got[0] == 0 and got[1] == 0 and not np.signbit(got[:2].real).any() and np.isnan(got[2].real) and np.isnan(got[2].imag)
        q = rs.model_values(x, 3, w, scale, N)
        assert rs.ratios(got, q, N, spp)[2] == 0 and np.isfinite(rs.ratios(got, q, N, spp)[:2]).all()


# ---- fetch_record_fine's arithmetic ------------------------------------------------------------------------------------------------
def _pulse_values(N, fi, offset_bins, seg0, seg1, T, w):
    """float64 model values of bin fi for T segments holding a tone ``offset_bins`` off its centre, switched on at the border in
    front of segment seg0 and off behind seg1 - 1"""
    n = np.arange(T * N)
    x = np.exp(2j * np.pi * (fi + offset_bins) * n / N)
    x[:seg0 * N] = 0
    x[seg1 * N:] = 0
    k = (fi * np.arange(N)) % N
    return ((x.reshape(T, N) * w) * np.exp(-2j * np.pi * k / N)).sum(axis=1)  # (no detrend: the tone's mean is the model's business)


@pytest.mark.parametrize("offset", [-0.4, -0.1, 0.0, 0.25, 0.45])
def test_fine_recovers_a_pulse_offset(offset):
    N, fi, T = 256, 40, 20
    w = oracle.window_coefficients("hamming", N)
    c = _pulse_values(N, fi, offset, 4, 15, T, w)
    # two records over the same cells: one delivered with a margin of two segments on either side, one without
    values = np.concatenate([c[2:17], c[4:15]])
    out = record_fine([0, 15, 26], [2, 4], values, [4, 4], [15, 15], FS, N)
    assert out.dtype == FINE_DTYPE and out["n_pairs"].tolist() == [10, 10]
    assert np.abs(out["offset_hz"] / (FS / N) - offset).max() <= 1e-9
    assert np.abs(out["coherence"] - 1).max() <= 1e-12


def test_fine_leaves_out_the_boundary_pair_and_short_records():
    N, fi, T = 256, 7, 12
    w = oracle.window_coefficients("hamming", N)
    c = _pulse_values(N, fi, 0.2, 0, T, T, w)
    jump = c.copy()
    jump[3:] *= np.exp(1j * 1.0)  # a phase step between the cells delivered as segments -1 and 0 -- the predecessor's ragged remainder
    # record 0: segments -3 .. 5 (the step lies between -1 and 0); record 1: one cell; record 2: no cell; record 3: two cells, -1 and 0
    values = np.concatenate([jump[0:8], c[0:1], c[0:0], jump[2:4]])
    out = record_fine([0, 8, 9, 9, 11], [-3, 2, 0, -1], values, [-3, 2, 0, -1], [5, 3, 0, 1], FS, N)
    assert out["n_pairs"].tolist() == [6, 0, 0, 0]
    assert abs(out["offset_hz"][0] / (FS / N) - 0.2) <= 1e-9 and abs(out["coherence"][0] - 1) <= 1e-12
    assert np.isnan(out["offset_hz"][1:]).all() and np.isnan(out["coherence"][1:]).all()
    with_pair = np.angle((jump[1:8] * np.conj(jump[0:7])).sum()) / (2 * np.pi)
    assert abs(with_pair - 0.2) > 1e-3  # (the pair across the boundary would have pulled the estimate)
    assert len(record_fine([0], [], np.zeros(0, np.complex64), [], [], FS, N)) == 0


# ---- the entries without a device --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _native.load_library()


def test_the_entries_exist_and_check_their_arguments_first(lib):
    raw = C.CDLL(_native.LIB_PATH)
    n = C.c_size_t(7)
    for name in ("rt_fetch_record_stft", "rt_fetch_record_stft_f64"):
        assert hasattr(raw, name) and name in _native.ABI_SYMBOLS
        fn = getattr(lib, name)
        assert fn(None, None, 0, None, 0, None, 0, C.byref(n)) == _native.RT_E_INVALID  # a null handle
        assert fn(None, None, 0, None, 0, None, 0, None) == _native.RT_E_INVALID         # ... and a null n_cells
    assert lib.rt_abi_version() == 6


# ---- the host-only arithmetic ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hc():
    lib = C.CDLL(build.build_hostcheck())
    vp = C.c_void_p
    lib.hc_stft_work.argtypes = [vp, vp, C.c_longlong, C.c_int, vp, vp]
    lib.hc_stft_work.restype = C.c_longlong
    lib.hc_stft_record_of.argtypes = [vp, C.c_int, C.c_longlong]
    lib.hc_stft_root_f32.argtypes = [C.c_float]
    lib.hc_stft_root_f32.restype = C.c_float
    lib.hc_stft_root_f64.argtypes = [C.c_double]
    lib.hc_stft_root_f64.restype = C.c_double
    lib.hc_stft_twiddles_f32.argtypes = [C.c_int, vp]
    lib.hc_stft_twiddles_f64.argtypes = [C.c_int, vp]
    return lib


def _work(hc, offsets, fi, N):
    offsets = np.ascontiguousarray(offsets, np.int64)
    fi = np.ascontiguousarray(fi, np.int32)
    seg = np.full(len(offsets), -7, np.int64)
    out = np.full(len(fi), -7, np.int32)
    n = hc.hc_stft_work(offsets.ctypes.data, fi.ctypes.data, len(fi), N, seg.ctypes.data, out.ctypes.data)
    return n, seg, out


@pytest.mark.parametrize("N", (8, 32, 256, 300, 1000, 8192))
def test_the_work_list_matches_numpy(hc, N):
    rng = np.random.default_rng(N)
    for trial in range(20):
        n = int(rng.integers(0, 40))
        counts = rng.integers(0, 9, n)  # (records without a delivered segment among them)
        offsets = np.concatenate([[0], np.cumsum(counts)]) * N
        fi = rng.integers(0, N, n)
        cells, seg, out = _work(hc, offsets, fi, N)
        assert cells == counts.sum() and np.array_equal(seg, offsets // N) and np.array_equal(out, fi)
        want = np.repeat(np.arange(n), counts)  # the record of every delivered segment
        got = [hc.hc_stft_record_of(seg.ctypes.data, n, g) for g in range(int(cells))]
        assert got == want.tolist()
        if n:
            bad = offsets.copy()
            bad[-1] += 1
            assert _work(hc, bad, fi, N)[0] == -1
            for wrong in (-1, N):
                bad_fi = fi.copy()
                bad_fi[int(rng.integers(0, n))] = wrong
                assert _work(hc, offsets, bad_fi, N)[0] == -1
            if counts.sum() and n > 1 and counts[-1]:
                back = offsets.copy()
                back[-1] = back[-2] - N
                assert _work(hc, back, fi, N)[0] == -1


@pytest.mark.parametrize("N", (8, 32, 256, 300, 1000, 4096, 16384))
def test_the_twiddle_table_and_the_root(hc, N):
    t32 = np.zeros(2 * N, np.float32)
    t64 = np.zeros(2 * N, np.float64)
    hc.hc_stft_twiddles_f32(N, t32.ctypes.data)
    hc.hc_stft_twiddles_f64(N, t64.ctypes.data)
    c32, s32 = rs.twiddles(N, np.float32)
    assert np.array_equal(t32[0::2], c32) and np.array_equal(t32[1::2], s32)  # float64 evaluation, rounded once: the restatement's table
    ang = -2 * rs.PI_LD * np.arange(N).astype(np.longdouble) / N
    assert np.abs(t64[0::2] - np.cos(ang)).max() <= 2.0 ** -53 and np.abs(t64[1::2] - np.sin(ang)).max() <= 2.0 ** -53
    assert t32[0] == 1 and t64[0] == 1
    for window in ("hamming", ("kaiser", 8.0)):
        scale = p64.scale_f32(window, N, FS)
        assert hc.hc_stft_root_f32(scale) == np.float32(math.sqrt(float(np.float32(scale))))
        assert hc.hc_stft_root_f64(scale) == math.sqrt(scale)


def test_work_list_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "stft_work"
    # (the runtimes linked statically: the program then runs the same whatever else the environment loads into a process)
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(REPO, "pyradiotracking_amd", "csrc"), "-o", str(exe), os.path.join(REPO, "tests", "c", "stft_work.cpp")],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr)
