"""rt_fetch_record_band without a GPU: the header's contract and the binding; the host book through ``rt_hostcheck`` against a NumPy
restatement, and as a stand-alone program under AddressSanitizer and UBSan (tests/c/stft_band_work.cpp); the model of a column is
SciPy's ``mode='complex'`` spectrogram at the column's bin; three planted faults leave the bound on the GPU suite's own inputs; the
twin case of the bit-identity test gives, through the oracle, the records that test needs; ``record_band_spectrum`` against a loop
(tests/record_band_cases.py)."""
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
from pyradiotracking_amd.analyze import band_bins, record_band_spectrum, stft_frame_positions
from tests import precision64 as p64
from tests import record_band_cases as bc
from tests import record_stft_cases as rs
from tests import record_stft_hop_cases as hop
from tests import sequence_cases as sq

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = sq.FS


# ---- header and binding ------------------------------------------------------------------------------------------------------------
def test_the_header_declares_both_entries_and_states_the_contract():
    text = open(os.path.join(REPO, "include", "rt_analyze.h")).read()
    at = text.index("int rt_fetch_record_band(rt_handle *h, int32_t hop_div, int32_t half_width,")
    assert "int rt_fetch_record_band_f64(rt_handle *h, int32_t hop_div, int32_t half_width," in text
    block = " ".join(text[text.rindex("/*", 0, at):at].replace("\n *", " ").split())  # (the comment's line breaks are not part of the contract)
    for words in ("circular", "half_width", "Column order", "column j of a frame belongs", "(fi + d) mod N", "bit identity", "column w (d = 0) is the bytes",
                  "column w + d of the one is the bytes of column w of the other", "exactly 0 + 0i in every column", "non-finite, in every column",
                  "RT_E_CAPACITY", "size query", "RT_E_NOMEM", "the wrong twin is refused too", "k, w and N"):
        assert words in block, words


def test_the_entries_exist_and_check_their_arguments_first():
    build.build_library()
    lib = _native.load_library()
    raw = C.CDLL(_native.LIB_PATH)
    n = C.c_size_t(7)
    for name in ("rt_fetch_record_band", "rt_fetch_record_band_f64"):
        assert hasattr(raw, name) and name in _native.ABI_SYMBOLS
        fn = getattr(lib, name)
        assert fn(None, 4, 2, None, 0, None, 0, None, 0, C.byref(n)) == _native.RT_E_INVALID  # a null handle
        assert fn(None, 4, 2, None, 0, None, 0, None, 0, None) == _native.RT_E_INVALID         # ... and a null n_frames
    assert lib.rt_abi_version() == 6


# ---- the book ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hc():
    lib = C.CDLL(build.build_hostcheck())
    lib.hc_stft_band_ok.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.hc_stft_band_bin.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    lib.hc_stft_band_elems.argtypes = [C.c_longlong, C.c_int]
    lib.hc_stft_band_elems.restype = C.c_longlong
    return lib


def test_the_book_matches_numpy_for_every_size_hop_and_width(hc):
    n_ok = 0
    for N in list(range(8, 65)) + [256, 300, 4096]:
        for k in range(-1, 19):
            for w in range(-2, 11):
                want = bc.band_ok(N, k, w)
                assert bool(hc.hc_stft_band_ok(N, k, w)) == want, (N, k, w)
                n_ok += want
        for w in range(0, 9):
            if 2 * w + 1 > N:
                continue
            for fi in sorted({0, 1, w, N // 2 - 1, N // 2, N - 1 - w, N - 2, N - 1} & set(range(N))):
                got = [hc.hc_stft_band_bin(fi, j, w, N) for j in range(2 * w + 1)]
                assert got == [bc.band_bin(fi, j, w, N) for j in range(2 * w + 1)] == band_bins([fi], w, N)[0].tolist(), (N, w, fi)
                assert got[w] == fi and all(0 <= b < N for b in got)
    assert n_ok > 1000
    # beside bin N - 1 lies bin 0, beside N / 2 - 1 the most negative frequency
    assert band_bins([255, 127], 1, 256).tolist() == [[254, 255, 0], [126, 127, 128]]
    assert np.fft.fftfreq(256)[128] == -0.5


@pytest.mark.parametrize("N,k,w", [(256, 4, -1), (256, 4, 9), (8, 1, 4), (16, 1, 8), (256, 3, 2), (300, 8, 2), (256, 0, 2), (256, 17, 0)])
def test_widths_and_hops_outside_the_contract_are_refused(hc, N, k, w):
    assert not hc.hc_stft_band_ok(N, k, w) and not bc.band_ok(N, k, w)


def test_the_widest_band_that_fits_is_accepted(hc):
    assert hc.hc_stft_band_ok(9, 3, 4) and hc.hc_stft_band_ok(17, 1, 8) and hc.hc_stft_band_ok(8, 8, 3)
    with pytest.raises(ValueError):
        band_bins([0], 4, 8)


def test_the_pool_size_is_a_checked_64_bit_product(hc):
    for frames, w in ((0, 0), (1, 0), (7, 8), (123456789, 2), (2 ** 40, 8)):
        assert hc.hc_stft_band_elems(frames, w) == bc.band_elems(frames, w) == frames * (2 * w + 1)
    for w in range(9):
        most = (2 ** 63 - 1) // 16 // (2 * w + 1)
        assert hc.hc_stft_band_elems(most, w) == most * (2 * w + 1)
        assert hc.hc_stft_band_elems(most + 1, w) == -1 and hc.hc_stft_band_elems(2 ** 63 - 1, w) == -1
    assert hc.hc_stft_band_elems(-1, 2) == -1 and hc.hc_stft_band_elems(5, 9) == -1 and hc.hc_stft_band_elems(5, -1) == -1


def test_the_book_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "stft_band_work"
    # (the runtimes linked statically: the program then runs the same whatever else the environment loads into a process)
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(REPO, "pyradiotracking_amd", "csrc"), "-o", str(exe), os.path.join(REPO, "tests", "c", "stft_band_work.cpp")],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr)


# ---- the model of a column is SciPy's spectrogram at the column's bin ---------------------------------------------------------------
MODEL_HALF = 2


@pytest.mark.parametrize("window", rs.SWEEP_WINDOWS, ids=lambda w: w if isinstance(w, str) else "kaiser8")
@pytest.mark.parametrize("N", rs.SWEEP_SIZES)
def test_the_model_of_a_column_is_scipys_spectrogram_at_that_bin(N, window):
    """float32: SciPy's complex64 result inside ``rs.bound`` (u = 2^-24) of the float64 model; float64: its complex128 result
    inside the bound at u = 2^-53 of the longdouble model.  The sizes, windows and input kinds are ``rs.sweep``'s; the bins are a
    band of half width 2 around a bin next to the circle's seam and one at the sign change."""
    w32, scale32 = rs.window32(window, N), p64.scale_f32(window, N, FS)
    w64 = oracle.window_coefficients(window, N)
    scale64 = float(1.0 / (FS * (w64 ** 2).sum()))
    worst = [0.0, 0.0]
    for kind in rs.KINDS:
        for k in (1, 4):
            h = N // k
            for fi in (N - 1, N // 2 - 1):
                rng = np.random.default_rng([N, rs.KINDS.index(kind), k, fi])
                x, spp = rs.sweep_input(kind, N, fi, 4, rng)
                part = x.reshape(-1)
                n_f = (len(part) // N - 1) * k + 1
                frames = hop.frames_of(part, np.arange(n_f) * h, N)
                _, _, Z = scipy.signal.spectrogram(part, FS, window, N, noverlap=N - h, detrend="constant", return_onesided=False, mode="complex")
                _, _, Z64 = scipy.signal.spectrogram(part.astype(np.complex128), FS, w64, N, noverlap=N - h, detrend="constant", return_onesided=False,
                                                     mode="complex")
                assert Z.dtype == np.complex64 and Z64.dtype == np.complex128 and Z.shape[1] == n_f
                for d in range(-MODEL_HALF, MODEL_HALF + 1):
                    b = (fi + d) % N
                    q = rs.model_values(frames, b, w32, scale32, N)
                    r = rs.ratios(Z[b], q, N, spp)
                    assert r.max() <= 1.0, ("float32", N, window, kind, k, fi, d, float(r.max()))
                    q64 = rs.model_values(frames.astype(np.complex128), b, w64, scale64, N, wide=True)
                    r64 = rs.ratios(Z64[b], q64, N, spp, rs.U64)
                    assert r64.max() <= 1.0, ("float64", N, window, kind, k, fi, d, float(r64.max()))
                    worst = [max(worst[0], float(r.max())), max(worst[1], float(r64.max()))]
    print(f"record_band model nperseg {N} {window}: worst SciPy ratio float32 {worst[0]:.3f} float64 {worst[1]:.3f}")


# ---- planted faults ----------------------------------------------------------------------------------------------------------------
def _gpu_inputs(N):
    """[(frames [n, N] complex64, fi, window, scale, root)]: the planted pulses of the GPU suite's call 1 (hamming: the pulse at
    bin 1 of the stream under a DC offset, the one at a negative-frequency bin) and the twin call's pulse at bin N - 1 (boxcar)"""
    out = []
    w, scale = rs.window32(sq.WINDOW, N), p64.scale_f32(sq.WINDOW, N, FS)
    x = rs.gpu_buffer(N, 1)
    a, e = rs.PLANT_SEGS
    for s, b in ((rs.DC_STREAM, rs.DC_BIN), (rs.NEG_STREAM, rs.neg_bin(N))):
        out.append((x[s, a * N:(a + 4) * N].reshape(-1, N), b, w, scale))
    wb, scale_b = rs.window32(bc.TWIN_WINDOW, N), p64.scale_f32(bc.TWIN_WINDOW, N, FS)
    _, t0, _ = bc.twin_layout(N)
    out.append((bc.twin_buffer(N, N - 1)[bc.TWIN_STREAM, t0 * N:(t0 + 4) * N].reshape(-1, N), N - 1, wb, scale_b))
    return [(f, b, w_, sc, float(np.float32(math.sqrt(sc)))) for f, b, w_, sc in out]


@pytest.mark.parametrize("N", [32, 256, 300])
def test_three_planted_faults_leave_the_bound_on_the_gpu_suites_inputs(N):
    half, spp = 2, rs.SPP["c64"]
    seen = {f: 0.0 for f in bc.FAULTS}
    for frames, fi, w, scale, root in _gpu_inputs(N):
        qs = bc.model_band(frames, fi, half, w, scale, N)
        ok = bc.band_ratios(bc.restate_band(frames, fi, half, w, root, N, spp), qs, N, spp)
        assert ok.max() <= 0.5, (N, fi, float(ok.max()))
        for fault in bc.FAULTS:
            same = bc.column_bins(fi, half, N, fault) == bc.column_bins(fi, half, N)
            bad = bc.band_ratios(bc.restate_band(frames, fi, half, w, root, N, spp, fault=fault), qs, N, spp)
            # every column the fault moves leaves the bound in every frame; the others are untouched
            if (~same).any():
                assert bad[:, ~same].min() > 1.0, (N, fi, fault, float(bad[:, ~same].min()))
                seen[fault] = max(seen[fault], float(bad[:, ~same].min()))
            assert np.array_equal(bad[:, same], ok[:, same])
    print(f"record_band planted faults nperseg {N}: smallest ratio of a moved column {seen}")
    assert all(v > 1.0 for v in seen.values()), seen  # each fault shows on some input (the clamp only at the circle's seam)


# ---- the twins plan ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", bc.TWIN_SIZES)
def test_the_twin_case_gives_records_of_one_span_at_every_bin_of_the_band(N):
    for fi in bc.twin_bins(N):
        rec = bc.twin_oracle_records(N, fi)
        spans = {(a, e) for _, a, e in rec}
        bins = [b for b, _, _ in rec]
        want = {(fi + d) % N for d in range(-bc.MAX_HALF, bc.MAX_HALF + 1)} - {0}
        print(f"record_band twins nperseg {N} fi {fi}: {len(rec)} records, spans {sorted(spans)}")
        assert len(spans) == 1 and len(set(bins)) == len(bins) and want <= set(bins) and 0 not in bins, (N, fi, spans)
        (a, e), = spans
        assert e - a >= bc.twin_need(N)
    if N == 4096:
        assert "signal_max_duration_ms" in bc.twin_settings(N)


# ---- record_band_spectrum ----------------------------------------------------------------------------------------------------------
def test_record_band_spectrum_against_a_direct_loop():
    rng = np.random.default_rng(11)
    for N, k, w in ((256, 4, 2), (300, 3, 1), (32, 1, 8), (256, 2, 0)):
        # records: both parts, all predecessor, all own, no segment, no inside frame
        L = np.array([7, 3, 4, 0, 2, 5])
        first = np.array([-3, -3, 0, -2, 4, 1], np.int32)
        start = np.array([-2, -3, 1, -2, 9, 2])
        end = np.array([3, 0, 4, -2, 9, 2])
        plan = hop.frame_plan(np.concatenate([[0], np.cumsum(L)]) * N, first, N, k)
        off = plan["frame_first"]
        values = (rng.standard_normal((off[-1], 2 * w + 1)) + 1j * rng.standard_normal((off[-1], 2 * w + 1))).astype(np.complex64)
        got = record_band_spectrum(off, first, values, start, end, N, k)
        want = bc.spectrum_loop(off, first, values, start, end, N, k)
        assert got.shape == (6, 2 * w + 1) and got.dtype == np.float64
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.allclose(got, want, rtol=1e-12, atol=0, equal_nan=True)
        assert np.isnan(got[3]).all() and np.isnan(got[4]).all() and np.isnan(got[5]).all() and not np.isnan(got[:3]).any()
        # the inside frames, counted from the positions
        pos = stft_frame_positions(off, first, N, k)
        inside = (pos >= start[plan["record"]] * N) & (pos + N <= end[plan["record"]] * N)
        assert np.array_equal(np.bincount(plan["record"][inside], minlength=6) > 0, ~np.isnan(got[:, 0]))
    assert record_band_spectrum([0], [], np.zeros((0, 5), np.complex64), [], [], 256, 4).shape == (0, 5)
