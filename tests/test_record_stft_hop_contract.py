"""rt_fetch_record_stft_hop without a GPU: the host's frame plan through ``rt_hostcheck`` against a NumPy restatement, and as a
stand-alone program under AddressSanitizer and UBSan (tests/c/stft_hop_work.cpp); the model of a frame is SciPy's overlapped
``mode='complex'`` spectrogram; the kernel's order with groups of 8, 16 and 32 lanes gives the bits of the 64-lane order; the
pulse-pair and edge estimators on model values, what ``hop_div`` adds to them, and three planted faults that leave their bounds
(tests/record_stft_hop_cases.py)."""
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
from pyradiotracking_amd.analyze import record_edges, record_fine, stft_frame_positions
from tests import precision64 as p64
from tests import record_stft_cases as rs
from tests import record_stft_hop_cases as hc_cases
from tests import sequence_cases as sq

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = sq.FS
WINDOWS = ("hamming", "hann", ("kaiser", 8.0))


# ---- the frame plan ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hc():
    lib = C.CDLL(build.build_hostcheck())
    vp = C.c_void_p
    lib.hc_stft_hop_work.argtypes = [vp, vp, vp, C.c_longlong, C.c_int, C.c_int, vp, vp, vp, vp]
    lib.hc_stft_hop_work.restype = C.c_longlong
    lib.hc_stft_hop_frame_at.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_longlong, vp]
    lib.hc_stft_hop_frame_at.restype = None
    return lib


def _plan(hc, offsets, first, fi, N, k):
    offsets = np.ascontiguousarray(offsets, np.int64)
    first = np.ascontiguousarray(first, np.int32)
    fi = np.ascontiguousarray(fi, np.int32)
    n = len(fi)
    frame_first = np.full(n + 1, -7, np.int64)
    pool_seg = np.full(n, -7, np.int64)
    lp = np.full(n, -7, np.int32)
    out = np.full(n, -7, np.int32)
    frames = hc.hc_stft_hop_work(offsets.ctypes.data, first.ctypes.data, fi.ctypes.data, n, N, k, frame_first.ctypes.data, pool_seg.ctypes.data,
                                 lp.ctypes.data, out.ctypes.data)
    return frames, frame_first, pool_seg, lp, out


def _random_records(rng, N):
    """record lists with every shape of record: no segment (L = 0), all in the predecessor part (Lp = L), all its own, both"""
    n = int(rng.integers(0, 30))
    L = rng.integers(0, 7, n)
    first = rng.integers(-5, 12, n)
    if n >= 4:
        L[0], first[0] = 0, -2      # no segment at all
        L[1], first[1] = 3, -3      # Lp = L: the record ends where its own part would begin
        L[2], first[2] = 2, -6      # all predecessor, ends before segment -1
        L[3], first[3] = 4, 0       # all its own
    return np.concatenate([[0], np.cumsum(L)]).astype(np.int64) * N, first.astype(np.int32), rng.integers(0, N, n).astype(np.int32)


@pytest.mark.parametrize("N,k", [(8, 1), (8, 2), (8, 8), (32, 16), (256, 4), (300, 4), (300, 3), (300, 15), (1000, 10), (8192, 16), (9, 3)])
def test_the_frame_plan_matches_numpy(hc, N, k):
    rng = np.random.default_rng([N, k])
    for trial in range(12):
        offsets, first, fi = _random_records(rng, N)
        n = len(fi)
        frames, frame_first, pool_seg, lp, fi_out = _plan(hc, offsets, first, fi, N, k)
        want = hc_cases.frame_plan(offsets, first, N, k)
        assert frames == want["frame_first"][-1] == len(want["record"])
        assert np.array_equal(frame_first, want["frame_first"]) and np.array_equal(pool_seg, want["pool_seg"])
        assert np.array_equal(lp, want["lp"]) and np.array_equal(fi_out, fi)
        got = np.zeros((int(frames), 3), np.int64)
        for g in range(int(frames)):
            hc.hc_stft_hop_frame_at(frame_first.ctypes.data, pool_seg.ctypes.data, lp.ctypes.data, n, N, k, g, got[g].ctypes.data)
        assert np.array_equal(got[:, 0], want["record"]) and np.array_equal(got[:, 1], want["part"]) and np.array_equal(got[:, 2], want["sample"])
        # every frame lies inside its part: none straddles the two, none leaves the record
        if frames:
            part_lo = offsets[:-1][want["record"]] + np.where(want["part"] == 1, want["lp"][want["record"]] * N, 0)
            part_hi = np.where(want["part"] == 1, offsets[1:][want["record"]], offsets[:-1][want["record"]] + want["lp"][want["record"]] * N)
            assert (want["sample"] >= part_lo).all() and (want["sample"] + N <= part_hi).all()
        # the Python side's positions are the plan's
        assert np.array_equal(stft_frame_positions(frame_first, first, N, k), want["position"])
        if k == 1:
            assert np.array_equal(frame_first, offsets // N)
        if n:
            bad = offsets.copy()
            bad[-1] += 1
            assert _plan(hc, bad, first, fi, N, k)[0] == -1
            bad_fi = fi.copy()
            bad_fi[int(rng.integers(0, n))] = N
            assert _plan(hc, offsets, first, bad_fi, N, k)[0] == -1
            if offsets[-1] > offsets[-2]:
                back = offsets.copy()
                back[-1] = back[-2] - N
                assert _plan(hc, back, first, fi, N, k)[0] == -1


@pytest.mark.parametrize("N,k", [(256, 0), (256, -1), (256, 17), (256, 3), (300, 8), (9, 2), (32, 32)])
def test_a_hop_that_does_not_divide_nperseg_is_refused(hc, N, k):
    offsets, first, fi = _random_records(np.random.default_rng(1), N)
    assert _plan(hc, offsets, first, fi, N, k)[0] == -1


def test_frame_plan_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "stft_hop_work"
    # (the runtimes linked statically: the program then runs the same whatever else the environment loads into a process)
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(REPO, "pyradiotracking_amd", "csrc"), "-o", str(exe), os.path.join(REPO, "tests", "c", "stft_hop_work.cpp")],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr)


def test_the_entries_exist_and_check_their_arguments_first():
    build.build_library()
    lib = _native.load_library()
    raw = C.CDLL(_native.LIB_PATH)
    n = C.c_size_t(7)
    for name in ("rt_fetch_record_stft_hop", "rt_fetch_record_stft_hop_f64"):
        assert hasattr(raw, name) and name in _native.ABI_SYMBOLS
        fn = getattr(lib, name)
        assert fn(None, 4, None, 0, None, 0, None, 0, C.byref(n)) == _native.RT_E_INVALID  # a null handle
        assert fn(None, 4, None, 0, None, 0, None, 0, None) == _native.RT_E_INVALID         # ... and a null n_frames
    assert lib.rt_abi_version() == 6


# ---- the model of a frame is SciPy's overlapped spectrogram --------------------------------------------------------------------------
def _input(N, fi, seed, n_seg=6):
    """complex64 [n_seg * N]: noise, a tone 0.3 bins over bin fi's centre, a DC offset"""
    rng = np.random.default_rng([seed, N, fi])
    n = np.arange(n_seg * N)
    x = (rng.standard_normal(n.size) + 1j * rng.standard_normal(n.size)) * 0.012 + 0.25 * np.exp(2j * np.pi * (fi + 0.3) * n / N) + (0.4 - 0.3j)
    return x.astype(np.complex64)


@pytest.mark.parametrize("window", WINDOWS, ids=lambda w: w if isinstance(w, str) else "kaiser8")
@pytest.mark.parametrize("N,k", [(N, k) for N in (32, 256, 300, 1024) for k in (2, 4, 16) if N % k == 0])
def test_the_model_of_a_frame_is_scipys_overlapped_spectrogram(N, k, window):
    """The tolerances of tests/test_record_stft_contract.py for the same comparison at noverlap 0: SciPy's complex64 result inside
    the bound, its complex128 result within 1e-12 of the segment's norm."""
    w, scale = rs.window32(window, N), p64.scale_f32(window, N, FS)
    h = N // k
    for fi in (1, N // 2, N - N // 3):
        x = _input(N, fi, 2)
        n_f = (len(x) // N - 1) * k + 1
        q = rs.model_values(hc_cases.frames_of(x, np.arange(n_f) * h, N), fi, w, scale, N)
        _, _, Z = scipy.signal.spectrogram(x, FS, window, N, noverlap=N - h, detrend="constant", return_onesided=False, mode="complex")
        assert Z.dtype == np.complex64 and Z.shape[1] == n_f
        r = rs.ratios(Z[fi], q, N, rs.SPP["c64"])
        assert r.max() <= 1.0, (N, k, window, fi, float(r.max()))
        _, _, Z64 = scipy.signal.spectrogram(x.astype(np.complex128), FS, w.astype(np.float64), N, noverlap=N - h, detrend="constant",
                                             return_onesided=False, mode="complex", scaling="density")
        own = math.sqrt(1.0 / (FS * float((w.astype(np.float64) ** 2).sum())))
        assert np.abs(Z64[fi] / own * q.root - q.values).max() <= 1e-12 * q.root * q.norm.max() * math.sqrt(N)


# ---- lane groups: the bits of the 64-lane order ---------------------------------------------------------------------------------------
GROUP_CASES = [(256, 8, 32), (32, 2, 16), (32, 4, 8), (32, 8, 8), (9, 2, 8), (9, 4, 8), (9, 8, 8), (64, 8, 8), (64, 4, 16), (300, 8, 64), (256, 4, 64)]


def _group_inputs(N, fi, rng):
    n = np.arange(N)
    noise = ((rng.standard_normal((3, N)) + 1j * rng.standard_normal((3, N))) * 0.012).astype(np.complex64)
    tone = (0.25 * np.exp(2j * np.pi * (fi + 0.3) * n / N) + (0.4 - 0.3j)).astype(np.complex64)[None, :]
    const = np.full((1, N), np.complex64(complex(np.float32(0.3), np.float32(-0.7))))         # a full-mantissa constant
    const2 = np.full((1, N), np.complex64(complex(-np.float32(1) / np.float32(3), np.float32(32767 / 32768))))
    cancel = (np.float32(0.25) * (-1.0) ** n).astype(np.complex64)[None, :]                      # sums that cancel exactly
    cancel2 = (np.float32(-0.5) * (-1.0) ** (n // 2) * (1 + 1j)).astype(np.complex64)[None, :]
    neg = -np.abs(noise[:1].real) - 1j * np.abs(noise[:1].imag)
    return np.concatenate([noise, tone, const, const2, cancel, cancel2, neg.astype(np.complex64)])


@pytest.mark.parametrize("N,spp,G", GROUP_CASES)
def test_a_lane_group_gives_the_bits_of_a_whole_wave(N, spp, G):
    """A frame of at most G pieces on G lanes against ``rs.restate``'s 64 lanes: the same bits, the zeros' signs included, under
    the handle's window and under a boxcar (where the alternating frames cancel exactly, lane by lane and in the butterfly)."""
    assert math.ceil(N / spp) <= G or G == 64
    rng = np.random.default_rng([N, spp, G])
    for window in ("hamming", "boxcar"):
        w = rs.window32(window, N)
        root = float(np.float32(math.sqrt(p64.scale_f32(window, N, FS))))
        for fi in (0, 1, N // 2, N - N // 3):
            x = _group_inputs(N, fi, rng)
            want = rs.restate(x, fi, w, root, N, spp)
            got = hc_cases.restate_groups(x, fi, w, root, N, spp, G)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (N, spp, G, window, fi)
            assert np.array_equal(np.signbit(got.real), np.signbit(want.real)) and np.array_equal(np.signbit(got.imag), np.signbit(want.imag))
            assert got[4] == 0 and got[5] == 0 and not np.signbit(got[4:6].real).any() and not np.signbit(got[4:6].imag).any()
    assert hc_cases.group_of(N, 16 // spp) == (G if math.ceil(N / spp) <= 32 else 64)


def test_a_lane_group_in_float64():
    N, spp, G = 16, 1, 16
    w = oracle.window_coefficients("hamming", N)
    rng = np.random.default_rng(3)
    x = _group_inputs(N, 3, rng).astype(np.complex128)
    want = rs.restate(x, 3, w, 0.37, N, spp, np.float64)
    got = hc_cases.restate_groups(x, 3, w, 0.37, N, spp, G, np.float64)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


# ---- the estimators on model values ---------------------------------------------------------------------------------------------------
TONES = (0.3, 0.7, 1.3, -1.6)


def _tone_setup():
    N, fi = 256, 50
    w = oracle.window_coefficients("hamming", N)
    return N, fi, w, 1.0 / (FS * float((w ** 2).sum()))


def _estimate(delta, k, fi_given=None):
    N, fi, w, scale = _tone_setup()
    off, first, values = hc_cases.tone_record(delta, fi, N, k, w, scale)
    out = record_fine(off, first, values, [0], [12], FS, N, k, [fi if fi_given is None else fi_given])
    assert out["n_pairs"][0] == len(values) - 1 and out["coherence"][0] > 0.99
    return out["offset_hz"][0] / (FS / N)


@pytest.mark.parametrize("delta", TONES)
def test_pulse_pair_at_a_quarter_segment_hop_recovers_offsets_beyond_half_a_bin(delta):
    got = _estimate(delta, 4)
    print(f"record_fine k=4 delta {delta}: {got:.4f}")
    assert abs(got - delta) <= 0.01
    whole = _estimate(delta, 1)
    print(f"record_fine k=1 delta {delta}: {whole:.4f}")
    if abs(delta) > 0.5:  # what the feature adds: at whole-segment hops the estimate is the offset modulo one bin
        assert abs(whole - delta) >= 0.99
    else:
        assert abs(whole - delta) <= 0.01


def test_record_fine_with_a_hop_needs_the_bins_and_keeps_to_one_part():
    N, fi, w, scale = _tone_setup()
    off, first, values = hc_cases.tone_record(0.3, fi, N, 4, w, scale)
    with pytest.raises(ValueError):
        record_fine(off, first, values, [0], [12], FS, N, 4)
    # the same twelve segments delivered as segments -5 .. 6: two parts of 5 and 7 segments, 17 + 25 frames; pairs stay inside a
    # part, and only frames wholly inside [start, end) count
    n = np.arange(12 * N)
    x = np.exp(2j * np.pi * (fi + 0.3) * n / N)
    x[5 * N:] *= np.exp(1j * 2.0)  # (the ragged remainder between the buffers: a phase step between the parts)
    plan = hc_cases.frame_plan([0, 12 * N], [-5], N, 4)
    assert plan["frame_first"].tolist() == [0, 42] and plan["part"].sum() == 25
    values = rs.model_values(hc_cases.frames_of(x, plan["sample"], N), fi, w, scale, N).values
    out = record_fine([0, 42], [-5], values, [-4], [6], FS, N, 4, [fi])
    assert out["n_pairs"][0] == (4 * 3 + 1 - 1) + (6 * 4 - 3 - 1)  # part 0: segments -4 .. -1; part 1: segments 0 .. 5
    assert abs(out["offset_hz"][0] / (FS / N) - 0.3) <= 1e-6 and abs(out["coherence"][0] - 1) <= 1e-9


@pytest.mark.parametrize("window,N", hc_cases.EDGE_ROWS, ids=lambda v: str(v))
def test_record_edges_to_a_quarter_of_a_hop(window, N):
    """The quarter hop is a cap, not a measurement (profiles/record_stft_hop_estimators.txt holds the worst errors: at most 0.083
    of a hop at k >= 2, and exactly 0 under a boxcar, whose |c| is a linear ramp)."""
    trials = 40 if N <= 1024 else 12  # (nperseg 4096: every trial is 10 x 8 frames of 4096 samples through the float64 model)
    for k in (2, 4, 8):
        e = hc_cases.edge_errors(window, N, k, trials)
        print(f"record_edges {window} {N} k={k}: worst rise {e[0] / (N // k):.3f} fall {e[1] / (N // k):.3f} hop")
        assert e.max() <= 0.25 * (N // k), (window, N, k, e)


def test_record_edges_at_whole_segment_hops_is_what_the_feature_improves_on():
    """At k = 1 the worst edge is more than 0.15 nperseg off: 0.199 (hamming 256), 0.20 (hamming 4096), 0.214 (hann 1024).  The
    boxcar row alone stays at 0.0858 nperseg, and that is the rule's own figure, not a fault: under a boxcar |c| is the number of
    samples the pulse has in the frame, a ramp, and the line between a partly filled segment (a of N samples) and the full one
    crosses N / 2 at an error of N (1/2 - a/N)(a/N) / (1 - a/N), at most (3 - 2 sqrt 2) / 2 = 0.0858 N.  So the statement is held
    over the rows together and by every tapered row on its own."""
    worst = {}
    for window, N in hc_cases.EDGE_ROWS:
        worst[(window, N)] = hc_cases.edge_errors(window, N, 1, 40 if N <= 1024 else 12).max() / N
        print(f"record_edges {window} {N} k=1: worst {worst[(window, N)]:.4f} nperseg")
    assert max(worst.values()) > 0.15
    assert all(v > 0.15 for (window, _), v in worst.items() if window != "boxcar")
    assert abs(worst[("boxcar", 256)] - (3 - 2 * math.sqrt(2)) / 2) < 2e-3


def test_record_edges_is_nan_where_the_part_ends_first():
    N, k = 256, 4
    w = oracle.window_coefficients("hamming", N)
    scale = 1.0 / (FS * float((w ** 2).sum()))
    x, rise, fall, start, end = hc_cases.edge_trial(N, np.random.default_rng(4))
    cut = x[start * N:end * N]  # margin 0: only the record's own cells are delivered
    off, first, values = hc_cases.one_part_record(cut, hc_cases.EDGE_BIN, w, scale, N, k, first_segment=start)
    assert np.isnan(record_edges(off, first, values, [start], [end], N, k)).all()
    # a record without a frame inside its own cells; an empty call
    assert np.isnan(record_edges(off, first, values, [start], [start], N, k)).all()
    assert record_edges([0], [], np.zeros(0, np.complex64), [], [], N, k).shape == (0, 2)
    # the buffer's end cuts the fall, the rise is found
    keep = x[:(end) * N]
    off, first, values = hc_cases.one_part_record(keep, hc_cases.EDGE_BIN, w, scale, N, k)
    got = record_edges(off, first, values, [start], [end], N, k)[0]
    assert abs(got[0] - rise) <= 0.25 * (N // k) and np.isnan(got[1])


# ---- planted faults --------------------------------------------------------------------------------------------------------------------
def test_a_frame_start_off_by_one_sample_leaves_the_bound():
    for N, k in ((256, 4), (300, 4), (32, 16)):
        w, scale = rs.window32("hamming", N), p64.scale_f32("hamming", N, FS)
        root = float(np.float32(math.sqrt(scale)))
        fi = N - N // 3
        x = _input(N, fi, 3)
        start = np.arange((len(x) // N - 2) * k + 1) * (N // k)
        q = rs.model_values(hc_cases.frames_of(x, start, N), fi, w, scale, N)
        ok = rs.ratios(hc_cases.restate_groups(hc_cases.frames_of(x, start, N), fi, w, root, N, 2, 64), q, N, 2)
        bad = rs.ratios(hc_cases.restate_groups(hc_cases.frames_of(x, start + 1, N), fi, w, root, N, 2, 64), q, N, 2)
        assert ok.max() <= 0.5 and bad.min() > 1.0, (N, k, float(ok.max()), float(bad.min()))


def test_a_frame_straddling_the_two_parts_leaves_the_bound():
    """A plan that frames a record's two parts as one run of samples delivers, between the last frame of the predecessor part and
    the first of the record's own, k - 1 frames that hold samples of both buffers: none of them is within the bound of any frame
    the contract delivers."""
    N, fi, w, scale = _tone_setup()
    k = 4
    n = np.arange(8 * N)
    x = np.exp(2j * np.pi * (fi + 0.3) * n / N)
    x[4 * N:] *= np.exp(1j * 2.5)  # the predecessor's ragged remainder lies between segments -1 and 0
    x = x.astype(np.complex64)
    plan = hc_cases.frame_plan([0, 8 * N], [-4], N, k)
    assert len(plan["sample"]) == 2 * (3 * k + 1)
    q = rs.model_values(hc_cases.frames_of(x, plan["sample"], N), fi, w, scale, N)
    good = record_fine(plan["frame_first"], [-4], q.values, [-4], [4], FS, N, k, [fi])
    assert abs(good["offset_hz"][0] / (FS / N) - 0.3) <= 0.01
    run = np.arange(7 * k + 1) * (N // k)  # the faulty plan: one part of eight segments
    straddling = np.setdiff1d(run, plan["sample"])
    assert len(straddling) == k - 1
    qs = rs.model_values(hc_cases.frames_of(x, straddling, N), fi, w, scale, N)
    e = rs.bound(q, N, rs.SPP["c64"])
    for v in qs.values:
        assert (np.abs(v - q.values) > e).all()


def test_leaving_out_the_bins_own_rotation_leaves_the_tolerance():
    # bin 50 at k = 4: 50 mod 4 = 2, half a turn a hop -- two bins; a bin that is a multiple of k needs no rotation
    assert abs(_estimate(0.3, 4, fi_given=0) - 0.3) > 0.01
    assert abs(abs(_estimate(0.3, 4, fi_given=0) - 0.3) - 2.0) <= 0.01
    assert abs(_estimate(0.3, 4, fi_given=48) - 0.3) > 0.01 and abs(_estimate(0.3, 4, fi_given=54) - 0.3) <= 0.01
