"""rt_fetch_record_estimates without a GPU: the host's plan through ``rt_hostcheck`` against a NumPy restatement, and as a
stand-alone program under AddressSanitizer and UBSan (tests/c/estimates_work.cpp); the kernel's order restated in NumPy
(tests/record_estimates_cases.py) against ``record_fine`` and ``record_edges`` within the derived bounds, on tones, pulses, noise and
the degenerate records; four planted faults that the bounds reject; the k = 1 frame rule against ``record_fine``'s segment rule; the
record lengths of the GPU suite's size-edge buffers from the oracle."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import analyze_oracle as oracle
from pyradiotracking_amd import _native, build
from pyradiotracking_amd.analyze import record_edges, record_fine
from tests import record_estimates_cases as ec
from tests import record_stft_hop_cases as hop
from tests import sequence_cases as sq
from tests import test_record_stft_hop_contract as hop_contract

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = sq.FS
WORST = {}


@pytest.fixture(scope="module")
def hc():
    lib = C.CDLL(build.build_hostcheck())
    vp = C.c_void_p
    lib.hc_estimates_work.argtypes = [vp, vp, vp, vp, vp, C.c_longlong, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]
    lib.hc_estimates_work.restype = C.c_longlong
    return lib


def _plan(hc, offsets, first, fi, start, end, N, k):
    offsets = np.ascontiguousarray(offsets, np.int64)
    first, fi = np.ascontiguousarray(first, np.int32), np.ascontiguousarray(fi, np.int32)
    start, end = np.ascontiguousarray(start, np.int32), np.ascontiguousarray(end, np.int32)
    n = len(fi)
    out = dict(frame_first=np.full(n + 1, -7, np.int64), lp=np.full(n, -7, np.int32), range=np.full((n, 4), -7, np.int32), base=np.full((n, 2), -7, np.int64),
               fmod=np.full(n, -7, np.int32), turn=np.full((16, 2), -7.0))
    frames = hc.hc_estimates_work(offsets.ctypes.data, first.ctypes.data, fi.ctypes.data, start.ctypes.data, end.ctypes.data, n, N, k,
                                  *(out[name].ctypes.data for name in ("frame_first", "lp", "range", "base", "fmod", "turn")))
    return frames, out


def _records(rng, N):
    """the hop contract test's record lists with cells of every kind: below what was delivered, inside it, beyond it, empty"""
    offsets, first, fi = hop_contract._random_records(rng, N)
    n = len(fi)
    L = np.diff(offsets) // N
    start = first + rng.integers(-3, 4, n)
    end = np.maximum(start, first + L + rng.integers(-3, 4, n))
    if n >= 8:
        L4 = int(L[4])
        start[4], end[4] = first[4] - 2, first[4] + L4          # cells that begin below what was delivered
        start[5], end[5] = max(int(first[5]), 0), max(int(first[5]), 0) + 1  # one segment of the record's own part
        start[6], end[6] = first[6], first[6]                  # no cell at all
        first[7], start[7], end[7] = -int(L[7]), -int(L[7]), 0  # no own part: the record ends where it would begin
    return offsets, first, fi, start.astype(np.int32), end.astype(np.int32)


@pytest.mark.parametrize("N,k", [(8, 1), (8, 2), (8, 8), (32, 16), (256, 4), (300, 4), (300, 3), (300, 15), (1000, 10), (8192, 16), (9, 3), (32, 1)])
def test_the_plan_matches_numpy(hc, N, k):
    rng = np.random.default_rng([N, k, 1])
    kinds = dict(no_own=0, no_pred=0, one=0, below=0)
    for trial in range(12):
        offsets, first, fi, start, end = _records(rng, N)
        n = len(fi)
        frames, got = _plan(hc, offsets, first, fi, start, end, N, k)
        want = ec.work_plan(offsets, first, fi, start, end, N, k)
        assert want is not None and frames == want["frame_first"][-1]
        for name in ("frame_first", "lp", "range", "base", "fmod"):
            assert np.array_equal(got[name], want[name]), name
        assert (np.abs(got["turn"][:k] - ec.turn_table(k)) <= 2.0 ** -52).all() and (got["turn"][k:] == -7.0).all()  # (one ulp of 1: two libms)
        # the runs hold exactly the frames record_fine and record_edges call inside
        fp = hop.frame_plan(offsets, first, N, k)
        assert np.array_equal(fp["frame_first"], want["frame_first"])
        for i in range(n):
            pos = fp["position"][fp["frame_first"][i]:fp["frame_first"][i + 1]]
            inside = np.flatnonzero((pos >= int(start[i]) * N) & (pos + N <= int(end[i]) * N))
            lo0, hi0, lo1, hi1 = want["range"][i]
            assert np.array_equal(inside, np.concatenate([np.arange(lo0, hi0), np.arange(lo1, hi1)]))
            L = (offsets[i + 1] - offsets[i]) // N
            kinds["no_own"] += int(L > 0 and want["lp"][i] == L)
            kinds["no_pred"] += int(L > 0 and want["lp"][i] == 0)
            kinds["one"] += int(L == 1)
            kinds["below"] += int(start[i] < first[i] and len(inside) > 0)
        if n:  # what the plan refuses: nothing is written
            i = int(rng.integers(0, n))
            bad = start.copy()
            bad[i] = end[i] + 1
            f, out = _plan(hc, offsets, first, fi, bad, end, N, k)
            assert f == -1 and ec.work_plan(offsets, first, fi, bad, end, N, k) is None and (out["range"] == -7).all() and (out["frame_first"] == -7).all()
            bad_off = offsets.copy()
            bad_off[-1] += 1
            assert _plan(hc, bad_off, first, fi, start, end, N, k)[0] == -1
            bad_fi = fi.copy()
            bad_fi[i] = N
            assert _plan(hc, offsets, first, bad_fi, start, end, N, k)[0] == -1
            if offsets[-1] > offsets[-2]:
                back = offsets.copy()
                back[-1] = back[-2] - N
                assert _plan(hc, back, first, fi, start, end, N, k)[0] == -1
    assert all(v > 0 for v in kinds.values()), kinds


@pytest.mark.parametrize("N,k", [(256, 0), (256, -1), (256, 17), (256, 3), (300, 8), (9, 2), (32, 32)])
def test_a_hop_that_does_not_divide_nperseg_is_refused(hc, N, k):
    offsets, first, fi, start, end = _records(np.random.default_rng(1), N)
    assert _plan(hc, offsets, first, fi, start, end, N, k)[0] == -1


def test_plan_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "estimates_work"
    # (the runtimes linked statically: the program then runs the same whatever else the environment loads into a process)
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(REPO, "pyradiotracking_amd", "csrc"), "-o", str(exe), os.path.join(REPO, "tests", "c", "estimates_work.cpp")],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr)


def test_the_entry_exists_and_checks_its_arguments_first():
    build.build_library()
    lib = _native.load_library()
    raw = C.CDLL(_native.LIB_PATH)
    n = C.c_size_t(7)
    assert hasattr(raw, "rt_fetch_record_estimates") and "rt_fetch_record_estimates" in _native.ABI_SYMBOLS
    assert lib.rt_fetch_record_estimates(None, 4, None, 0, C.byref(n)) == _native.RT_E_INVALID  # a null handle
    assert lib.rt_fetch_record_estimates(None, 4, None, 0, None) == _native.RT_E_INVALID         # ... and a null n_out
    assert _native.ESTIMATE_DTYPE.itemsize == 72 and lib.rt_abi_version() == 6


# ---- the kernel's order against the model ----------------------------------------------------------------------------------------------
def _held(name, offsets, first, values, start, end, fi, N, k, turn=None, left_out=0):
    got = ec.restate(offsets, first, values, start, end, fi, N, k, turn=turn)
    m = ec.model(offsets, first, values, start, end, fi, N, k)
    worst, out, bad = ec.compare(got, m, N, k)
    print(f"record_estimates restated, {name}: " + " ".join(f"{f} {v:.3f}" for f, v in worst.items()) + f", {out} without clearance")
    assert not bad, (name, bad[:3])
    assert out <= left_out, (name, out)
    w = WORST.setdefault(name, dict.fromkeys(worst, 0.0))
    for f, v in worst.items():
        w[f] = max(w[f], v)
    return got, m


def _tone_setup(N=256):
    w = oracle.window_coefficients("hamming", N)
    return w, 1.0 / (FS * float((w ** 2).sum()))


@pytest.mark.parametrize("k", [1, 2, 4, 16])
def test_tones_within_the_bounds(hc, k):
    N, fi = 256, 50
    w, scale = _tone_setup(N)
    turn = _plan(hc, [0], [], [], [], [], N, k)[1]["turn"][:k]
    for delta in hop_contract.TONES:
        for cast in (np.complex64, np.complex128):
            off, first, values = hop.tone_record(delta, fi, N, k, w, scale)
            got, m = _held(f"tone k={k}", off, first, values.astype(cast), [0], [12], [fi], N, k, turn=turn)
            assert got["n_pairs"][0] == len(values) - 1 and got["coherence"][0] > 0.99 and np.isnan(got["rise"][0]) and np.isnan(got["fall"][0])
            if abs(delta) < k / 2:
                assert abs(got["offset_bins"][0] - delta) <= 0.01


@pytest.mark.parametrize("window,N", [r for r in hop.EDGE_ROWS if r[1] <= 1024], ids=lambda v: str(v))
def test_pulses_within_the_bounds(window, N):
    w = oracle.window_coefficients(window, N)
    scale = 1.0 / (FS * float((w ** 2).sum()))
    for k in (1, 2, 4, 8):
        rng = np.random.default_rng([7, N, k])
        edges = 0
        for _ in range(8):
            x, rise, fall, start, end = hop.edge_trial(N, rng)
            x = x + 1e-3 * (rng.standard_normal(len(x)) + 1j * rng.standard_normal(len(x)))
            off, first, values = hop.one_part_record(x, hop.EDGE_BIN, w, scale, N, k)
            got, m = _held(f"pulse {window} {N}", off, first, values, [start], [end], [hop.EDGE_BIN], N, k)
            edges += int(np.isfinite(got["rise"][0])) + int(np.isfinite(got["fall"][0]))
            if k >= 2:
                assert abs(got["rise"][0] - rise) <= 0.3 * (N // k) and abs(got["fall"][0] - fall) <= 0.3 * (N // k)
        assert edges == 16


def _noise_call(rng, N, k, cast=np.complex128, scale=1.0):
    offsets, first, fi, start, end = _records(rng, N)
    fp = hop.frame_plan(offsets, first, N, k)
    n_f = int(fp["frame_first"][-1])
    values = (scale * (rng.standard_normal(n_f) + 1j * rng.standard_normal(n_f))).astype(cast)
    return fp["frame_first"], first, values, start, end, fi


@pytest.mark.parametrize("N,k", [(256, 4), (32, 16), (9, 3), (32, 1), (1024, 2)])
def test_noise_within_the_bounds(N, k):
    rng = np.random.default_rng([N, k, 2])
    seen = dict(pairs=0, two_parts=0, edges=0)
    for trial in range(10):
        off, first, values, start, end, fi = _noise_call(rng, N, k, np.complex64 if trial % 2 else np.complex128, 10.0 ** rng.integers(-6, 3))
        got, m = _held(f"noise N={N} k={k}", off, first, values, start, end, fi, N, k)
        seen["pairs"] += int(got["n_pairs"].sum())
        seen["edges"] += int(np.isfinite(got["rise"]).sum() + np.isfinite(got["fall"]).sum())
    assert seen["pairs"] > 50 and seen["edges"] > 5, seen


def test_a_long_record_reads_its_frames_again():
    """more than 256 inside frames: the magnitudes beyond the lane's registers, and strides of more than one round"""
    N, k = 32, 16
    rng = np.random.default_rng(11)
    n_f = 69 * k + 1
    values = (rng.standard_normal(n_f) + 1j * rng.standard_normal(n_f)) * np.concatenate([np.full(40, 0.01), np.full(n_f - 80, 1.0), np.full(40, 0.01)])
    got, m = _held("long record", [0, n_f], [3], values, [4], [72], [5], N, k)
    assert got["n_inside"][0] == 67 * k + 1 and got["n_pairs"][0] == 67 * k and np.isfinite(got["rise"][0]) and np.isfinite(got["fall"][0])


def test_degenerate_records():
    N, k, fi = 256, 4, 50
    n_f = 6 * k + 1
    # identical frames: every pair product is the same number, the median is that value, no frame lies below half
    same = np.full(n_f, 0.3 - 0.7j)
    got, m = _held("identical frames", [0, n_f], [0], same, [1], [6], [fi], N, k)
    assert got["level"][0] == np.sqrt(0.3 * 0.3 + 0.7 * 0.7) and np.isnan(got["rise"][0]) and np.isnan(got["fall"][0]) and abs(got["coherence"][0] - 1) < 1e-15
    # all-zero frames: M == 0, coherence 0 / 0, half == 0 and no edge
    got, m = _held("zero frames", [0, n_f], [0], np.zeros(n_f, np.complex64), [1], [6], [fi], N, k)
    assert got["pair_mag"][0] == 0 and got["n_pairs"][0] > 0 and np.isnan(got["coherence"][0]) and got["level"][0] == 0
    assert np.isnan(got["rise"][0]) and np.isnan(got["fall"][0]) and got["offset_bins"][0] == 0
    # a NaN frame inside: R, M, level and the edges are NaN; in the margin only: nothing but an edge walk meets it, and passes it
    rng = np.random.default_rng(5)
    amp = np.concatenate([np.full(k, 0.01), np.full(n_f - 2 * k, 1.0), np.full(k, 0.01)])
    clean = amp * np.exp(2j * np.pi * (0.05 * np.arange(n_f) + 0.01 * rng.standard_normal(n_f)))
    inside = clean.copy()
    inside[3 * k] = complex(np.nan, 1.0)
    got, m = _held("a NaN frame inside", [0, n_f], [0], inside, [1], [5], [fi], N, k)
    assert np.isnan(got["r_re"][0]) and np.isnan(got["pair_mag"][0]) and np.isnan(got["level"][0]) and np.isnan(got["rise"][0]) and got["n_pairs"][0] == 3 * k
    margin = clean.copy()
    margin[1] = complex(np.nan, np.nan)
    ref, _ = _held("clean twin", [0, n_f], [0], clean, [1], [5], [fi], N, k)
    got, m = _held("a NaN frame in the margin", [0, n_f], [0], margin, [1], [5], [fi], N, k)
    assert got.tobytes() == ref.tobytes() and np.isfinite(got["rise"][0]) and np.isfinite(got["fall"][0])
    # ... and where the walk has to pass it: the frames between up0 and the first frame below half
    passed = clean.copy()
    passed[k] = complex(np.nan, 0.0)  # (frame k is the record's first inside frame's predecessor's place: inside starts at frame k)
    got, m = _held("a NaN frame the walk passes", [0, n_f], [0], passed, [2], [5], [fi], N, k)
    assert np.isnan(got["rise"][0]) and np.isfinite(got["fall"][0])  # (the neighbour on the pulse's side is the NaN frame: record_edges gives NaN)
    # records without a frame inside, and an empty call
    got, m = _held("nothing inside", [0, n_f], [0], clean, [3], [3], [fi], N, k)
    assert got["n_inside"][0] == 0 and got["n_pairs"][0] == 0 and all(np.isnan(got[f][0]) for f in ("offset_bins", "coherence", "level", "rise", "fall"))
    assert len(ec.restate([0], [], np.zeros(0, np.complex64), [], [], [], N, k)) == 0


def test_non_finite_frames_keep_to_the_models_pattern():
    """Frames with an infinite component, a NaN in one component only, and both: |c| = inf, level = inf, half = inf,
    (inf - a) / (inf - a) in the edge line, inf * 0 and inf - inf in the pair sums.  The rows have the model's NaN / Inf pattern in
    every field (``ec.compare`` holds infinities to equality), inside the record's cells and in the margin."""
    N, fi = 256, 50
    nan, inf = np.nan, np.inf
    kinds = [complex(inf, 0.25), complex(0.25, -inf), complex(nan, 0.25), complex(0.25, nan), complex(nan, nan), complex(inf, nan), complex(nan, -inf),
             complex(inf, inf), complex(-inf, 0.0)]
    rng = np.random.default_rng(21)
    seen = dict(inf_level=0, nan_level=0, inf_mag=0)
    for k in (1, 4):
        n_f = 8 * k + 1
        amp = np.concatenate([np.full(2 * k, 0.01), np.full(n_f - 4 * k, 1.0), np.full(2 * k, 0.01)])
        clean = amp * np.exp(2j * np.pi * (0.05 * np.arange(n_f) + 0.01 * rng.standard_normal(n_f)))
        for bad in kinds:
            for at in (0, 2 * k - 1, 2 * k, 3 * k, 4 * k + 1, n_f - 2 * k - 1, n_f - 1):  # the margins, the edges' frames, the plateau
                for count in (1, 2, 5):  # (five of nine inside frames: the median itself is the planted magnitude)
                    v = clean.copy()
                    v[at:at + count] = bad
                    for start, end, bin_ in ((2, 6, fi), (2, 7, fi + 1), (0, 8, fi + 2)):
                        got, m = _held("non-finite frames", [0, n_f], [0], v, [start], [end], [bin_], N, k, left_out=0)
                        seen["inf_level"] += int(np.isinf(got["level"][0]))
                        seen["nan_level"] += int(np.isnan(got["level"][0]))
                        seen["inf_mag"] += int(np.isinf(got["pair_mag"][0]))
    assert all(v > 20 for v in seen.values()), seen
    # two parts, the planted frame in the predecessor part
    for bad in kinds[:5]:
        off, first, v, start, end = _two_part_record(N, 4, rng)
        v = v.copy()
        v[5] = bad
        _held("non-finite frames", off, first, v, start, end, [fi], N, 4)


# ---- planted faults ----------------------------------------------------------------------------------------------------------------------
def _two_part_record(N, k, rng, quiet_own_head=False):
    """segments -4 .. 5 delivered, the cells -3 .. 5 the record's own: 13 + 21 frames at k = 4, a phase step between the parts"""
    f0, f1 = 3 * k + 1, 5 * k + 1
    amp0 = np.concatenate([np.full(k // 2 + 1, 0.01), np.full(f0 - k // 2 - 1, 1.0)])
    amp1 = np.concatenate([np.full(f1 - k, 1.0), np.full(k, 0.01)])
    if quiet_own_head:  # the own part never falls below half towards its first frame, the predecessor part does
        amp0 = np.concatenate([np.full(f0 - 2, 1.0), np.full(2, 0.01)])
    ph = 2 * np.pi * 0.3 / k * np.arange(f0 + f1) + 0.01 * rng.standard_normal(f0 + f1)
    ph[f0:] += 2.0
    values = np.concatenate([amp0, amp1]) * np.exp(1j * ph)
    return [0, f0 + f1], [-4], values, [-3 if not quiet_own_head else 0], [5]


def _faulty(fault, off, first, values, start, end, fi, N, k):
    ok = ec.compare(ec.restate(off, first, values, start, end, fi, N, k), ec.model(off, first, values, start, end, fi, N, k), N, k)
    assert not ok[2] and ok[1] == 0, ok
    return ec.compare(ec.restate(off, first, values, start, end, fi, N, k, fault=fault), ec.model(off, first, values, start, end, fi, N, k), N, k)[2]


def test_a_pair_across_the_two_parts_leaves_the_bounds():
    N, k = 256, 4
    rec = _two_part_record(N, k, np.random.default_rng(1))
    bad = _faulty("pair_across_parts", *rec, [48], N, k)
    assert bad and bad[0][0] == "counts"
    # the counts aside: the pair's own product alone moves R beyond its bound
    got = ec.restate(*rec, [48], N, k, fault="pair_across_parts")
    m = ec.model(*rec, [48], N, k)
    allow = ec.C1 * (m["n_pairs"][0] + 4) * ec.U * m["pair_mag"][0]
    assert max(abs(got["r_re"][0] - m["r_re"][0]), abs(got["r_im"][0] - m["r_im"][0])) > 1e6 * allow


def test_a_median_one_rank_off_leaves_the_bounds():
    rng = np.random.default_rng(3)
    for N, k in ((256, 4), (32, 1)):
        hit = 0
        for trial in range(4):
            off, first, values, start, end, fi = _noise_call(rng, N, k)
            bad = _faulty("median_rank_off", off, first, values, start, end, fi, N, k)
            hit += sum(1 for b in bad if b[0] == "level")
        assert hit > 10


def test_the_turn_back_left_out_leaves_the_bounds():
    N, k = 256, 4
    w, scale = _tone_setup(N)
    off, first, values = hop.tone_record(0.3, 50, N, k, w, scale)
    bad = _faulty("no_turn_back", off, first, values, [0], [12], [50], N, k)  # 50 mod 4 = 2: half a turn a hop
    assert {b[0] for b in bad} >= {"r_re", "offset_bins"}
    assert not ec.compare(ec.restate(off, first, values, [0], [12], [48], N, k, fault="no_turn_back"), ec.model(off, first, values, [0], [12], [48], N, k), N, k)[2]


def test_an_edge_walk_into_the_other_part_leaves_the_bounds():
    N, k = 256, 4
    rec = _two_part_record(N, k, np.random.default_rng(2), quiet_own_head=True)
    m = ec.model(*rec, [48], N, k)
    assert np.isnan(m["rise"][0]) and np.isfinite(m["fall"][0])  # the own part begins at full level: its rise is not delivered
    bad = _faulty("walk_crosses_parts", *rec, [48], N, k)
    assert [b[:3] for b in bad] == [("rise", 0, "NaN pattern")]


# ---- k = 1: the frames are the segments ------------------------------------------------------------------------------------------------
def test_the_frame_rule_at_k_1_is_record_fines_segment_rule():
    """``record_fine(hop_div=1)`` pairs segments by number and leaves out (-1, 0); the plan pairs frames by position inside a part.
    ``ec.model`` asserts its frame-rule pair count against ``record_fine``'s; here the sums themselves are compared too."""
    rng = np.random.default_rng(9)
    pairs = back = 0
    for N in (32, 256):
        for trial in range(10):
            off, first, values, start, end, fi = _noise_call(rng, N, 1)
            got, m = _held("k=1 segment rule", off, first, values, start, end, fi, N, 1)
            fine = record_fine(off, first, values, start, end, float(N), N, 1)
            assert np.array_equal(got["n_pairs"], fine["n_pairs"])
            plan = ec.work_plan(off * N, first, fi, start, end, N, 1)
            both = (plan["range"][:, 1] > plan["range"][:, 0]) & (plan["range"][:, 3] > plan["range"][:, 2])
            back += int(both.sum())
            pairs += int(fine["n_pairs"].sum())
    assert pairs > 50 and back > 5, (pairs, back)


def test_record_edges_and_the_restatement_agree_on_nan():
    rng = np.random.default_rng(13)
    for N, k in ((256, 4), (32, 1)):
        off, first, values, start, end, fi = _noise_call(rng, N, k)
        got = ec.restate(off, first, values, start, end, fi, N, k)
        want = record_edges(off, first, values, start, end, N, k)
        assert np.array_equal(np.isnan(got["rise"]), np.isnan(want[:, 0])) and np.array_equal(np.isnan(got["fall"]), np.isnan(want[:, 1]))


def test_the_size_edge_buffers_give_the_record_lengths_the_gpu_suite_counts_on():
    """The oracle on tests/record_estimates_cases.py's size-edge buffers: exactly one record a pulse, of the pulse's cells and the
    cold cell before it.  A pulse that runs to the buffer's end is no record of that call: the reference reports it in the next,
    with a negative start -- so no record of a call is cut by the buffer's end, and a fall is NaN only where margin 0 delivers
    nothing behind the record."""
    calls = ec.edge_oracle_records()
    assert [[(e - s) for _, s, e in per] for per in calls[0]] == [[n] for n in ec.EDGE_INSIDE] + [[ec.EDGE_LONG], []]
    assert all(fi == ec.EDGE_BIN for per in calls[0] + calls[1] for fi, _, _ in per)
    assert calls[0][0] == [(ec.EDGE_BIN, 0, 1)]  # the only record without a cold cell in front
    assert [per for per in calls[1] if per] == [[(ec.EDGE_BIN, 2, 5)], [(ec.EDGE_BIN, -6, 4)]] and calls[1][ec.EDGE_S - 1] == [(ec.EDGE_BIN, -6, 4)]
    assert (ec.EDGE_LONG - 1) * 16 + 1 == 1105


def test_zz_write_the_worst_ratios():
    """(last in the file: the table of what the tests above saw, profiles/record_estimates_worst_ratio.txt's CPU half)"""
    assert WORST
    text = ec.format_worst("the NumPy restatement of the kernel's order (no GPU involved)", WORST)
    print(text)
    if os.environ.get("RT_WRITE_PROFILES"):
        ec.write_worst("cpu", text)
