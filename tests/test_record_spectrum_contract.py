"""rt_fetch_record_spectrum without a GPU: the entry and its argument rule; the kernel's order restated in NumPy
(tests/record_spectrum_cases.py) against ``record_band_rows`` -- and against ``record_band_spectrum`` for the means -- within the
derived bounds, on tones, noise and two-part records; the degenerate plans through ``rt_hostcheck``; non-finite frames; three
planted faults; what the two position estimates say of model tones (recorded, not asserted)."""
import ctypes as C
import os

import numpy as np
import pytest

from pyradiotracking_amd import _native, build
from pyradiotracking_amd.analyze import SPECTRUM_DTYPE, record_band_rows, record_band_spectrum, spectrum_hz
from tests import record_spectrum_cases as sc
from tests import record_stft_hop_cases as hop
from tests import test_record_estimates_contract as est_contract

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORST = {}
#: (N, k) with k a divisor of N, over the sizes and hops the contract test is asked for
SHAPES = [(8, 1), (8, 4), (32, 1), (32, 4), (32, 16), (256, 1), (256, 4), (256, 16), (300, 1), (300, 3), (300, 4)]
WIDTHS = (0, 1, 2, 3, 8)


@pytest.fixture(scope="module")
def hc():
    lib = C.CDLL(build.build_hostcheck())
    vp = C.c_void_p
    lib.hc_estimates_work.argtypes = [vp, vp, vp, vp, vp, C.c_longlong, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]
    lib.hc_estimates_work.restype = C.c_longlong
    lib.hc_spectrum_refusal.argtypes = [C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int]
    lib.hc_stft_hop_refusal.argtypes = [C.c_int, C.c_int, C.c_char_p, C.c_int]
    lib.hc_spectrum_pool_bytes.argtypes = [C.c_longlong, C.c_int]
    lib.hc_spectrum_pool_bytes.restype = C.c_longlong
    return lib


# ---- header, binding, the argument rule --------------------------------------------------------------------------------------------
def test_the_header_declares_the_entry_and_states_the_contract():
    text = open(os.path.join(REPO, "include", "rt_analyze.h")).read()
    at = text.index("typedef struct rt_record_spectrum {")
    assert "int rt_fetch_record_spectrum(rt_handle *h, int32_t hop_div, int32_t half_width, rt_record_spectrum *rows, double *mean, double *peak," in text
    block = " ".join(text[text.rindex("/*", 0, at):at].replace("\n *", " ").split())
    for words in ("partial i mod 64", "folded by halving", "divided by n_inside", "a NaN propagates", "left to right", "lowest j", "peak_col is -1",
                  "k, w and N", "RT_E_CAPACITY", "size query", "RT_E_NOMEM", "copies only", "copies without rebuilding", "rt_set_record_iq must be on",
                  "total == 0"):
        assert words in block, words
    assert SPECTRUM_DTYPE.itemsize == 48 and SPECTRUM_DTYPE is _native.SPECTRUM_DTYPE


def _refusal(hc, N, k, w):
    buf = C.create_string_buffer(512)
    n = hc.hc_spectrum_refusal(N, k, w, buf, 512)
    assert n == len(buf.value)
    return buf.value.decode()


def test_the_entry_exists_and_refuses_bad_arguments_first(hc):
    """(fails without the feature: the library has no such symbol)"""
    build.build_library()
    lib = _native.load_library()
    raw = C.CDLL(_native.LIB_PATH)
    assert hasattr(raw, "rt_fetch_record_spectrum") and "rt_fetch_record_spectrum" in _native.ABI_SYMBOLS
    n = C.c_size_t(7)
    assert lib.rt_fetch_record_spectrum(None, 4, 2, None, None, None, 0, C.byref(n)) == _native.RT_E_INVALID  # a null handle
    assert lib.rt_fetch_record_spectrum(None, 4, 2, None, None, None, 0, None) == _native.RT_E_INVALID         # ... and a null n_out
    assert lib.rt_abi_version() == 6
    # the rule the entry applies before it looks at the handle's calls, and the words it refuses with (csrc/rt_record_stft_book.h:
    # spectrum_refusal): k not dividing N, w = 9, 2 w + 1 > N at N = 8 with w = 4
    for N, k, w in ((256, 3, 2), (256, 4, 9), (8, 1, 4), (256, 0, 2), (256, 17, 2), (256, 4, -1), (300, 8, 0)):
        why = _refusal(hc, N, k, w)
        assert why and f"k = {k}" in why and f"w = {w}" in why and f"N = {N}" in why, (N, k, w, why)
    for N, k, w in ((8, 1, 3), (8, 8, 0), (256, 16, 8), (300, 15, 8), (17, 1, 8), (1, 1, 0)):
        assert _refusal(hc, N, k, w) == "", (N, k, w)
    # the hop and estimates entries' rule has no w (stft_hop_refusal): its words are the front of the band rule's
    for N, k, ok in ((256, 3, False), (256, 0, False), (256, 17, False), (300, 8, False), (256, 16, True), (300, 15, True), (1, 1, True)):
        buf = C.create_string_buffer(512)
        assert hc.hc_stft_hop_refusal(N, k, buf, 512) == len(buf.value)
        assert buf.value.decode() == ("" if ok else f"hop_div k = {k} must be 1 ... 16 and divide nperseg N = {N}"), (N, k)
        assert _refusal(hc, N, k, 9).startswith(f"hop_div k = {k} must be 1 ... 16 and divide nperseg N = {N}, half_width w = 9 must be 0 ... 8")
    for n_rec, w in ((0, 0), (1, 0), (7, 8), (79000, 2)):
        assert hc.hc_spectrum_pool_bytes(n_rec, w) == n_rec * (48 + 16 * (2 * w + 1))


# ---- the kernel's order against the model ------------------------------------------------------------------------------------------
def _held(name, offsets, first, values, start, end, N, k, left_out=0):
    got = sc.restate(offsets, first, values, start, end, N, k)
    want = sc.model(offsets, first, values, start, end, N, k)
    worst, out, bad = sc.compare(got, want)
    assert not bad, (name, bad[:3])
    assert out <= left_out, (name, out)
    # record_band_spectrum's means agree with the new function's within the same bound (two summation orders of the same terms)
    old = record_band_spectrum(offsets, first, values, start, end, N, k)
    n_in = want[0]["n_inside"].astype(np.float64)[:, None]
    assert np.array_equal(np.isnan(old), np.isnan(want[1]))
    fin = np.isfinite(want[1]) & np.isfinite(old)
    assert (np.abs(old[fin] - want[1][fin]) <= ((2 * n_in + 1) * sc.U * want[1])[fin]).all(), name
    w = WORST.setdefault(name, dict.fromkeys(worst, 0.0))
    for f, v in worst.items():
        w[f] = max(w[f], v)
    return got, want


@pytest.mark.parametrize("window", ["hamming", "boxcar"])
def test_tones_within_the_bounds(window):
    seen = 0
    for N, k in SHAPES:
        for w in WIDTHS:
            if 2 * w + 1 > N:
                continue
            fi = N - 1 if w == 1 else 1 if w == 3 else min(5, N - 1)  # (the band wraps at either end of the circle; bin 0 is detrended away)
            for delta in (0.0, 0.3, -0.45):
                off, first, values = sc.tone_band(delta, fi, w, N, k, window, n_seg=6)
                for cast in (np.complex64, np.complex128):
                    (rows, mean, peak), _ = _held(f"tone {window}", off, first, values.astype(cast), [0], [6], N, k, left_out=1)
                    assert rows["n_inside"][0] == len(values) == 5 * k + 1 and (peak >= mean).all()
                    if w >= 1 and N >= 32 and abs(delta) < 0.4:
                        assert rows["peak_col"][0] == w and rows["centre_share"][0] > 0.4
                    if w == 0:
                        assert rows["centre_share"][0] == 1.0 and rows["width"][0] == 0.0 and np.isnan(rows["peak_bins"][0]) and rows["centroid"][0] == 0.0
                    seen += 1
    assert seen > 200


def _noise_band(rng, N, k, w, cast, scale):
    offsets, first, fi, start, end = est_contract._records(rng, N)
    fp = hop.frame_plan(offsets, first, N, k)
    n_f = int(fp["frame_first"][-1])
    B = 2 * w + 1
    shape = rng.uniform(0.2, 1.0, B)  # (columns of unequal power: a peak column with clearance)
    values = (scale * shape * (rng.standard_normal((n_f, B)) + 1j * rng.standard_normal((n_f, B)))).astype(cast)
    return fp["frame_first"], first, values, start, end, fp


@pytest.mark.parametrize("N,k", SHAPES, ids=lambda v: str(v))
def test_noise_and_two_part_records_within_the_bounds(N, k):
    seen = dict(two_parts=0, inside=0, empty=0, records=0)
    for w in WIDTHS:
        if 2 * w + 1 > N:
            continue
        rng = np.random.default_rng([N, k, w, 3])
        for trial in range(4):
            off, first, values, start, end, fp = _noise_band(rng, N, k, w, np.complex64 if trial % 2 else np.complex128, 10.0 ** rng.integers(-6, 3))
            (rows, mean, peak), _ = _held(f"noise N={N} k={k}", off, first, values, start, end, N, k, left_out=len(first))
            rng4 = sc.plan_of(off, first, start, end, N, k)
            seen["two_parts"] += int(((rng4[:, 1] > rng4[:, 0]) & (rng4[:, 3] > rng4[:, 2])).sum())
            seen["inside"] += int(rows["n_inside"].sum())
            seen["empty"] += int((rows["n_inside"] == 0).sum())
            seen["records"] += len(rows)
            empty = rows["n_inside"] == 0
            assert np.isnan(mean[empty]).all() and np.isnan(peak[empty]).all() and (rows["peak_col"][empty] == -1).all()
            assert all(np.isnan(rows[f][empty]).all() for f in sc.SCALARS)
    assert seen["two_parts"] > 0 and seen["empty"] > 0 and seen["inside"] > seen["records"], seen


def test_long_records_take_several_rounds_of_the_partials():
    """1, 2, 3, 63, 64, 65, 127, 128, 129 and 1105 inside frames: the lane count and the one- and two-round limits"""
    rng = np.random.default_rng(21)
    for n_in, N, k in [(c, 32, 1) for c in (1, 2, 3, 63, 64, 65, 127, 128, 129)] + [(1105, 32, 16)]:
        n_f = n_in + 2 * k
        values = rng.standard_normal((n_f, 5)) + 1j * rng.standard_normal((n_f, 5))
        L = (n_f - 1) // k + 1
        assert (L - 1) * k + 1 == n_f
        (rows, mean, peak), _ = _held(f"{n_in} inside", [0, n_f], [0], values, [1], [L - 1], N, k, left_out=1)
        assert rows["n_inside"][0] == n_in
        p = np.abs(values[k:k + n_in]) ** 2
        assert np.allclose(mean[0], p.mean(axis=0), rtol=1e-12) and np.allclose(peak[0], p.max(axis=0), rtol=1e-15)


# ---- degenerate plans ----------------------------------------------------------------------------------------------------------------
def test_degenerate_plans_through_the_hosts_planner(hc):
    N, k, w = 32, 4, 2
    B = 2 * w + 1
    rng = np.random.default_rng(9)
    # records: no inside frame (cells beyond what was delivered); exactly one; wholly in the predecessor part; wholly in its own;
    # both parts; no segment at all
    L = np.array([3, 3, 4, 4, 6, 0])
    first = np.array([2, 2, -4, 1, -3, 0], np.int32)
    start = np.array([9, 3, -4, 2, -2, 0], np.int32)
    end = np.array([9, 4, -1, 4, 2, 0], np.int32)
    fi = np.zeros(6, np.int32)
    offsets = np.concatenate([[0], np.cumsum(L)]) * N
    frames, plan = est_contract._plan(hc, offsets, first, fi, start, end, N, k)
    off = plan["frame_first"]
    assert frames == off[-1] > 0
    assert np.array_equal(sc.plan_of(off, first, start, end, N, k), plan["range"])  # the restatement runs from the host's runs
    values = (rng.standard_normal((frames, B)) + 1j * rng.standard_normal((frames, B))).astype(np.complex64)
    (rows, mean, peak), _ = _held("degenerate plans", off, first, values, start, end, N, k, left_out=6)
    lo0, hi0, lo1, hi1 = plan["range"].T
    assert rows["n_inside"].tolist() == [0, 1, 2 * k + 1, k + 1, k + 1 + k + 1, 0]
    assert (hi0 - lo0).tolist() == [0, 0, 2 * k + 1, 0, k + 1, 0] and (hi1 - lo1).tolist() == [0, 1, 0, k + 1, k + 1, 0]
    for i in (0, 5):
        assert np.isnan(mean[i]).all() and np.isnan(peak[i]).all() and rows["peak_col"][i] == -1 and all(np.isnan(rows[f][i]) for f in sc.SCALARS)
    # one inside frame: the mean is the frame, and so is the peak
    one = values[off[1] + lo1[1]].astype(np.complex128)
    assert np.array_equal(mean[1], one.real ** 2 + one.imag ** 2) and np.array_equal(peak[1], mean[1])
    # an empty call
    rows, mean, peak = sc.restate([0], [], np.zeros((0, B), np.complex64), [], [], N, k)
    assert len(rows) == 0 and mean.shape == peak.shape == (0, B)
    rows, mean, peak = record_band_rows([0], [], np.zeros((0, B), np.complex64), [], [], N, k)
    assert len(rows) == 0 and mean.shape == peak.shape == (0, B) and rows.dtype == SPECTRUM_DTYPE


def test_non_finite_frames_keep_to_the_models_pattern():
    N, k, w = 32, 4, 2
    n_f = 6 * k + 1
    rng = np.random.default_rng(4)
    clean = rng.standard_normal((n_f, 5)) + 1j * rng.standard_normal((n_f, 5))
    ref, _ = _held("clean twin", [0, n_f], [0], clean, [1], [5], N, k)
    nan, inf = np.nan, np.inf
    for kind in (complex(nan, 0.25), complex(0.25, nan), complex(inf, 0.25), complex(0.25, -inf), complex(inf, nan), complex(nan, nan)):
        # inside the record's cells: the column's mean and peak, and with a NaN mean every scalar
        x = clean.copy()
        x[2 * k, 1] = kind
        (rows, mean, peak), (mrows, mmean, mpeak) = _held("a non-finite frame inside", [0, n_f], [0], x, [1], [5], N, k, left_out=1)
        p = kind.real * kind.real + kind.imag * kind.imag
        if np.isnan(p):
            assert np.isnan(mean[0, 1]) and np.isnan(peak[0, 1]) and rows["peak_col"][0] == -1 and all(np.isnan(rows[f][0]) for f in sc.SCALARS)
        else:
            assert mean[0, 1] == inf and peak[0, 1] == inf and rows["total"][0] == inf and rows["peak_col"][0] == 1 and np.isnan(rows["peak_bins"][0])
            assert rows["centre_share"][0] == 0.0 and np.isnan(rows["centroid"][0])
        others = [0, 2, 3, 4]  # the other columns' means and peaks are the clean twin's bytes
        assert mean[:, others].tobytes() == ref[1][:, others].tobytes() and peak[:, others].tobytes() == ref[2][:, others].tobytes()
        # in the margin: nothing reads it
        x = clean.copy()
        x[1, 3] = kind
        got, _ = _held("a non-finite frame in the margin", [0, n_f], [0], x, [1], [5], N, k)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, ref))
    # a +inf and a NaN in one column: the NaN wins in the peak (numpy.max), whichever comes first
    for a, b in ((3 * k, 2 * k), (2 * k, 3 * k)):
        x = clean.copy()
        x[a, 0], x[b, 0] = complex(inf, 0), complex(nan, 0)
        (rows, mean, peak), _ = _held("inf and NaN", [0, n_f], [0], x, [1], [5], N, k)
        assert np.isnan(peak[0, 0]) and np.isnan(mean[0, 0])
    # constant (zero) frames: total == 0 and the divisions give NaN
    (rows, mean, peak), _ = _held("zero frames", [0, n_f], [0], np.zeros((n_f, 5), np.complex64), [1], [5], N, k, left_out=1)
    assert (mean == 0).all() and (peak == 0).all() and rows["total"][0] == 0 and rows["peak_col"][0] == 0
    assert all(np.isnan(rows[f][0]) for f in ("centre_share", "centroid", "width", "peak_bins"))


# ---- planted faults ------------------------------------------------------------------------------------------------------------------
def _two_part_call(seed=6):
    N, k, w = 32, 4, 2
    rng = np.random.default_rng(seed)
    L, first = np.array([9, 30]), np.array([-3, 2], np.int32)
    start, end = np.array([-2, 4], np.int32), np.array([5, 30], np.int32)
    fp = hop.frame_plan(np.concatenate([[0], np.cumsum(L)]) * N, first, N, k)
    off = fp["frame_first"]
    amp = np.where((fp["position"] >= start[fp["record"]] * N) & (fp["position"] + N <= end[fp["record"]] * N), 1.0, 0.05)  # a pulse: the margin is quiet
    values = amp[:, None] * (rng.standard_normal((off[-1], 5)) + 1j * rng.standard_normal((off[-1], 5))) * np.array([0.3, 0.6, 1.0, 0.7, 0.2])
    return off, first, values, start, end, N, k


def test_a_frame_in_the_next_partial_changes_the_bytes():
    off, first, values, start, end, N, k = _two_part_call()
    good = sc.restate(off, first, values, start, end, N, k)
    bad = sc.restate(off, first, values, start, end, N, k, fault="partial_shifted")
    assert not sc.same_bytes(good, good) and "mean" in sc.same_bytes(bad, good)
    assert good[2].tobytes() == bad[2].tobytes()  # (a maximum does not depend on the order)
    assert not sc.compare(bad, sc.model(off, first, values, start, end, N, k))[2]  # (another order of the same sum: inside the bounds)


def test_frames_that_are_not_inside_counted_in_leave_the_bounds():
    off, first, values, start, end, N, k = _two_part_call()
    want = sc.model(off, first, values, start, end, N, k)
    assert not sc.compare(sc.restate(off, first, values, start, end, N, k), want)[2]
    bad = sc.compare(sc.restate(off, first, values, start, end, N, k, fault="outside_counted"), want)[2]
    assert bad and bad[0][0] == "counts"
    # ... and with the count itself put right, every mean leaves its bound
    rows, mean, peak = sc.restate(off, first, values, start, end, N, k, fault="outside_counted")
    rows["n_inside"] = want[0]["n_inside"]
    worst, _, bad = sc.compare((rows, mean, peak), want)
    assert worst["mean"] > 1e6 and any(b[0] == "mean" for b in bad)


def test_the_last_maximum_on_a_planted_tie_changes_peak_col():
    off, first, values, start, end, N, k = _two_part_call()
    values = values.copy()
    values[:, 3] = values[:, 2]  # columns 2 and 3 tie exactly, and are the largest
    values[:, 1] = values[:, 2] * 0.5
    good = sc.restate(off, first, values, start, end, N, k)
    bad = sc.restate(off, first, values, start, end, N, k, fault="last_maximum")
    assert np.array_equal(good[1][:, 2], good[1][:, 3]) and (good[0]["peak_col"] == 2).all() and (bad[0]["peak_col"] == 3).all()
    assert sc.same_bytes(bad, good) == ["peak_col"]
    assert (record_band_rows(off, first, values, start, end, N, k)[0]["peak_col"] == 2).all()  # the definition takes the lowest too


# ---- the helper, the profiles -----------------------------------------------------------------------------------------------------
def test_spectrum_hz_scales_the_three_fields_in_bins():
    off, first, values, start, end, N, k = _two_part_call()
    rows = record_band_rows(off, first, values, start, end, N, k)[0]
    hz = spectrum_hz(rows, 250000.0, N)
    for f in ("centroid", "width", "peak_bins"):
        assert np.array_equal(hz[f], rows[f] * (250000.0 / N), equal_nan=True)
    for f in ("total", "centre_share", "peak_col", "n_inside"):
        assert np.array_equal(hz[f], rows[f])
    assert hz is not rows and hz.dtype == SPECTRUM_DTYPE


def test_zz_write_the_estimators_and_the_worst_ratios():
    """(last in the file) what peak_bins and centroid say of model tones is recorded, not asserted"""
    text = sc.write_estimators(sc.ESTIMATORS if os.environ.get("RT_WRITE_PROFILES") else None)
    print(text)
    assert len(text.splitlines()) == 10 and WORST
    table = sc.format_worst("the NumPy restatement of the kernel's order against record_band_rows (tests/test_record_spectrum_contract.py)", WORST)
    print(table)
    assert max(max(v.values()) for v in WORST.values()) <= 1.0
    if os.environ.get("RT_WRITE_PROFILES"):
        sc.write_worst("cpu", table)
