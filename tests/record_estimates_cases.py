"""Per-record estimates reduced on the device (``rt_fetch_record_estimates``): the NumPy restatement of the host's plan and of
the kernel's order, the model rows (``record_fine`` and ``record_edges``, which define the result), the bounds a row is held to and
the comparison -- shared by tests/test_record_estimates_contract.py (CPU) and tests/test_gpu_record_estimates.py (GPU).

Bounds, u = 2^-53.  Model and kernel start from the same float64 frames c[t] = x + i y.

R, M.  A pair term x1 x0 + y1 y0 is two rounded products and a rounded sum: off by at most 2 u (|x1 x0| + |y1 y0|) <= 2 u |c1||c0|.
Summing n terms in any order adds at most (n - 1) u sum|term| <= (n - 1) u M.  The turn R (cos - i sin) with table entries one u
off costs 3 u |R| <= 3 u M on each side (the model's complex product is the same three roundings).  The model's R is summed exactly
(math.fsum) before the turn.  Together (n + 7) u M.  A term of M is sqrt(s1) sqrt(s0), s = x^2 + y^2 within 2 u, each root within
2 u, the product u: 5 u; its sum (n - 1) u M; the model's terms (hypot within one ulp = 2 u each, the product u) 5 u: (n + 9) u M.
Both are below  C1 (n_pairs + 4) u M  with  C1 = 2  for every n_pairs >= 1.

offset_bins.  The angle of R moves by at most |dR| / |R| with |dR| <= sqrt(2) times the component bound; times k / (2 pi).  atan2
(2 u on the device, u in libm, of at most pi), the division and the product by k on each side and the model's detour through Hz
(two more roundings) are relative errors of at most 10 u on |offset_bins| <= k / 2:  C2 u  with  C2 = 5 k.

coherence.  |R| / M: relative dR / |R| + dM / M, and 4 u for the root and the quotient on both sides.

level.  |c| is +inf on both sides where a component is infinite (hypot's rule, which the kernel follows), and NaN where one is NaN
and none infinite.  (Finite components whose squares overflow are outside the contract, as they are for the frames themselves.)
Otherwise sqrt(x^2 + y^2) is within 2 u of |c| and hypot within one ulp: 2 ulp of the level between them, the figure the contract
names.  The median is one of the inputs or the mean of two, and moves by no more than its inputs do.

An edge.  t = (half - a_q) / (a_p - a_q) with a_q < half <= a_p.  half, a_q and a_p each differ by 4 u relative between the sides,
the differences round once: numerator and denominator are each off by at most 9 u max(a_p, half); t in [0, 1] and the quotient's
rounding on both sides give dt <= (18 max(a_p, half) / |a_p - a_q| + 2) u <= C3 u max(a_p, half) / |a_p - a_q|  with  C3 = 20.
The edge is (pos[q] +- t h) + N / 2: h dt, and u |pos| for the sums' own rounding.  Each side rounds twice, at pos[q] +- t h and
at the edge itself, and where t differs in its last place the two sides' roundings fall independently: up to u times the rounded
magnitude for each of the four roundings.  |pos| is therefore their sum, 2 (|pos[q]| + h) + 2 (|pos[q]| + h + N / 2).  (Reading
|pos| as one magnitude, |pos[q]| + h + N, allows half an ulp of the edge: an MI355X run then shows six rows whose t differs in
the last place and whose edge differs by exactly one ulp, 9.1e-13 at -5120.5, against 8.1e-13 allowed -- ratio 1.12.)  A comparison |c| >= half or |c| < half can fall differently on the two sides only where |c| is within a few u of
half: a record with such a |c| within 1e-12 relative among the frames the rule compares has no clearance and its edges are not
compared (compare() counts them; the tests allow at most one per case).
"""
import math
import os

import numpy as np

from pyradiotracking_amd import _native
from pyradiotracking_amd.analyze import _stft_frames, record_edges, record_fine
from tests import record_stft_hop_cases as hop

U = 2.0 ** -53
C1, C3 = 2.0, 20.0
CLEARANCE = 1e-12
FAULTS = ("pair_across_parts", "median_rank_off", "no_turn_back", "walk_crosses_parts")


def c2(k):
    return 5.0 * k


# ---- the plan --------------------------------------------------------------------------------------------------------------------------
def work_plan(offsets, first_seg, fi, start, end, N, k):
    """estimates_build_work (csrc/rt_record_stft_book.h) in NumPy: ``offsets`` [n + 1] in SAMPLES -> dict of ``frame_first`` [n + 1],
    ``lp`` [n], ``range`` [n, 4] (lo0, hi0, lo1, hi1 as frame indices inside the record), ``base`` [n, 2], ``fmod`` [n]; None where
    the host refuses the lists."""
    offsets = np.asarray(offsets, dtype=np.int64)
    first = np.asarray(first_seg, dtype=np.int64)
    fi = np.asarray(fi, dtype=np.int64)
    start = np.asarray(start, dtype=np.int64)
    end = np.asarray(end, dtype=np.int64)
    n = len(first)
    if not (1 <= k <= 16 and N >= 1 and N % k == 0) or offsets[0] != 0 or (np.diff(offsets) < 0).any() or (offsets % N).any():
        return None
    if ((fi < 0) | (fi >= N)).any() or (start > end).any():
        return None
    L = np.diff(offsets) // N
    lp = np.clip(-first, 0, L)
    fp, fc = hop.part_frames(lp, k), hop.part_frames(L - lp, k)
    rng = np.zeros((n, 4), np.int64)
    base = np.stack([first * N, np.maximum(first, 0) * N], axis=1) if n else np.zeros((0, 2), np.int64)
    for p, (seg0, F) in enumerate(((first, fp), (np.maximum(first, 0), fc))):
        lo = np.clip((start - seg0) * k, 0, F)
        hi = np.maximum(np.clip((end - 1 - seg0) * k + 1, 0, F), lo)
        rng[:, 2 * p], rng[:, 2 * p + 1] = lo + p * fp, hi + p * fp
    return dict(frame_first=np.concatenate([[0], np.cumsum(fp + fc)]).astype(np.int64), lp=lp.astype(np.int32), range=rng.astype(np.int32),
                base=base.astype(np.int64), fmod=(fi % k).astype(np.int32))


def turn_table(k):
    """[k, 2] (cos, sin) of 2 pi m / k as the host builds it (libm through ``math``)"""
    return np.array([[math.cos(2.0 * math.pi * m / k), math.sin(2.0 * math.pi * m / k)] for m in range(k)], np.float64).reshape(k, 2)


# ---- the kernel's order -----------------------------------------------------------------------------------------------------------------
_LANES = np.arange(64)


def _butterfly(v):
    m = 32
    while m >= 1:
        v = v + v[_LANES ^ m]
        m //= 2
    return v[0]


def _select(bits, rank):
    """the pattern of rank ``rank`` among the uint64 ``bits``, found bit by bit from the top as the kernel finds it"""
    res = np.uint64(0)
    for b in range(62, -1, -1):
        cand = res | (np.uint64(1) << np.uint64(b))
        if int((bits < cand).sum()) <= rank:
            res = cand
    return res


def restate(offsets, first_seg, values, start, end, fi, N, k, fault=None, turn=None):
    """record_estimates' arithmetic (csrc/rt_record_estimates.h) on the frames ``values`` of ``fetch_record_stft(hop_div=k)``
    (``offsets`` in FRAMES): ``ESTIMATE_DTYPE`` rows.  ``fault``: one of FAULTS, planted."""
    assert fault is None or fault in FAULTS
    offsets = np.asarray(offsets, dtype=np.int64)
    n = len(offsets) - 1
    h = N // k
    first = np.asarray(first_seg, dtype=np.int64)
    L = np.zeros(n + 1, np.int64)
    # the plan from frame counts: a record's segments follow from its frames and lp
    fr = np.diff(offsets)
    lp_want = np.maximum(-first, 0)
    fp = np.minimum(hop.part_frames(lp_want, k), fr)
    lp = np.where(fp > 0, (fp - 1) // k + 1, 0)
    fc = fr - fp
    seg_total = lp + np.where(fc > 0, (fc - 1) // k + 1, 0)
    L[1:] = np.cumsum(seg_total)
    plan = work_plan(L * N, first, fi, start, end, N, k)
    assert plan is not None and np.array_equal(plan["frame_first"], offsets)
    turn = turn_table(k) if turn is None else np.asarray(turn, np.float64).reshape(-1, 2)
    v = np.asarray(values).astype(np.complex128)
    out = np.zeros(n, _native.ESTIMATE_DTYPE)
    for name in ("offset_bins", "coherence", "level", "rise", "fall"):
        out[name] = np.nan
    with np.errstate(all="ignore"):
        for i in range(n):
            x, y = v[offsets[i]:offsets[i + 1]].real.copy(), v[offsets[i]:offsets[i + 1]].imag.copy()
            a = np.where(np.isinf(x) | np.isinf(y), np.inf, np.sqrt(x * x + y * y))  # (hypot's rule for an infinite component)
            F, Fp = len(x), int(fp[i])
            lo0, hi0, lo1, hi1 = (int(t) for t in plan["range"][i])
            runs = [(lo0, hi0), (lo1, hi1)]
            if fault == "pair_across_parts" and hi0 == Fp and lo1 == Fp and hi0 > lo0 and hi1 > lo1:
                runs = [(lo0, hi1)]
            re, im, mg = np.zeros(64), np.zeros(64), np.zeros(64)
            n_pairs = 0
            for lo, hi in runs:
                n_pairs += max(hi - lo - 1, 0)
                for t0 in range(lo, hi - 1, 64):
                    t = t0 + _LANES
                    ok = t < hi - 1
                    t = np.minimum(t, max(hi - 2, 0))
                    re = np.where(ok, re + (x[t + 1] * x[t] + y[t + 1] * y[t]), re)
                    im = np.where(ok, im + (y[t + 1] * x[t] - x[t + 1] * y[t]), im)
                    mg = np.where(ok, mg + a[t + 1] * a[t], mg)
            re, im, mg = _butterfly(re), _butterfly(im), _butterfly(mg)
            re = re + 0.0 * im  # (record_fine's re + 1j * im)
            if k != 1 and fault != "no_turn_back":
                c, s = turn[int(plan["fmod"][i])]
                re, im = re * c + im * s, im * c - re * s
            inside = np.concatenate([np.arange(lo0, hi0), np.arange(lo1, hi1)])
            n_in = len(inside)
            row = out[i]
            row["r_re"], row["r_im"], row["pair_mag"], row["n_pairs"], row["n_inside"] = re, im, mg, n_pairs, n_in
            if n_pairs:
                row["offset_bins"] = math.atan2(im, re) / (2.0 * 3.141592653589793) * float(k)
                row["coherence"] = np.sqrt(re * re + im * im) / mg
            if n_in == 0 or np.isnan(a[inside]).any():
                continue
            bits = a[inside].view(np.uint64)
            shift = 1 if fault == "median_rank_off" else 0
            upper = _select(bits, min(n_in // 2 + shift, n_in - 1)).view(np.float64)
            level = upper if n_in & 1 else (_select(bits, n_in // 2 - 1 + shift).view(np.float64) + upper) / 2.0
            row["level"] = level
            half = 0.5 * level
            if not half > 0:
                continue
            up = inside[a[inside] >= half]
            if not len(up):
                continue
            pos = lambda q: float(int(plan["base"][i][0 if q < Fp else 1]) + (q - (0 if q < Fp else Fp)) * h)  # noqa: E731
            for name, q0, step in (("rise", int(up[0]), -1), ("fall", int(up[-1]), 1)):
                pb, pe = (0, Fp) if q0 < Fp else (Fp, F)
                if fault == "walk_crosses_parts":
                    pb, pe = 0, F
                q = q0 + step
                while pb <= q < pe and not a[q] < half:
                    q += step
                if not pb <= q < pe:
                    continue
                t = (half - a[q]) / (a[q - step] - a[q])
                row[name] = (pos(q) + t * float(-step * h)) + 0.5 * float(N)
    return out


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
def model(offsets, first_seg, values, start, end, fi, N, k):
    """What defines the rows: ``record_fine`` and ``record_edges`` on the same frames, with the quantities the bounds are made
    of.  ``offsets`` in FRAMES.  dict of arrays [n]: the fields of a row (``offset_bins`` from ``offset_hz`` at sample rate N), and
    per edge ``q_pos``, ``ratio`` = max(a_p, half) / |a_p - a_q| and ``clear`` (False: some compared |c| is within CLEARANCE of half)."""
    offsets = np.asarray(offsets, dtype=np.int64)
    n = len(offsets) - 1
    v = np.asarray(values).astype(np.complex128)
    start = np.asarray(start, dtype=np.int64)
    end = np.asarray(end, dtype=np.int64)
    fi = np.asarray(fi, dtype=np.int64)
    with np.errstate(all="ignore"):
        fine = record_fine(offsets, first_seg, v, start, end, float(N), N, k, fi)
        edges = record_edges(offsets, first_seg, v, start, end, N, k)
        rec, pred, pos = _stft_frames(offsets, first_seg, N, k)
        a = np.abs(v)
    m = dict(offset_bins=fine["offset_hz"].astype(np.float64), coherence=fine["coherence"].astype(np.float64), n_pairs=fine["n_pairs"].astype(np.int64),
             rise=edges[:, 0].copy(), fall=edges[:, 1].copy(), level=np.full(n, np.nan), n_inside=np.zeros(n, np.int64), r_re=np.zeros(n),
             r_im=np.zeros(n), pair_mag=np.zeros(n), q_pos=np.full((n, 2), np.nan), ratio=np.full((n, 2), np.nan), clear=np.ones(n, bool))
    h = N // k
    with np.errstate(all="ignore"):
        for i in range(n):
            lo, hi = int(offsets[i]), int(offsets[i + 1])
            ai, pi, parti, ci = a[lo:hi], pos[lo:hi], pred[lo:hi], v[lo:hi]
            own = (pi >= start[i] * N) & (pi + N <= end[i] * N)
            inside = np.flatnonzero(own)
            m["n_inside"][i] = len(inside)
            pair = own[:-1] & own[1:] & (parti[:-1] == parti[1:]) if hi - lo >= 2 else np.zeros(0, bool)
            assert int(pair.sum()) == m["n_pairs"][i]
            prod = (ci[1:] * np.conj(ci[:-1]))[pair] if hi - lo >= 2 else np.zeros(0, np.complex128)
            if np.isfinite(prod.real).all() and np.isfinite(prod.imag).all():
                R = complex(math.fsum(prod.real), math.fsum(prod.imag))
            else:  # (record_fine's own construction: 1j * inf has a NaN real part)
                R = complex(np.float64(prod.real.sum()) + 1j * np.float64(prod.imag.sum()))
            if k != 1:
                R = complex(np.complex128(R) * np.exp(-2j * np.pi * (fi[i] % k) / k))
            mags = (ai[1:] * ai[:-1])[pair] if hi - lo >= 2 else np.zeros(0)
            m["r_re"][i], m["r_im"][i] = R.real, R.imag
            m["pair_mag"][i] = math.fsum(mags) if np.isfinite(mags).all() else mags.sum()
            if not len(inside):
                continue
            m["level"][i] = float(np.median(ai[inside]))
            half = 0.5 * m["level"][i]
            if not half > 0:
                continue
            near = [ai[inside]]
            up = inside[ai[inside] >= half]
            if not len(up):
                continue
            for col, q, step in ((0, int(up[0]), -1), (1, int(up[-1]), 1)):
                part = parti[q]
                q += step
                while 0 <= q < len(ai) and parti[q] == part and not ai[q] < half:
                    near.append(ai[q:q + 1])
                    q += step
                if not (0 <= q < len(ai)) or parti[q] != part:
                    assert np.isnan(edges[i, col])
                    continue
                near.append(ai[q:q + 1])
                p = q - step
                want = pi[q] + (half - ai[q]) / (ai[p] - ai[q]) * (pi[p] - pi[q]) + 0.5 * N
                assert want == edges[i, col] or (np.isnan(want) and np.isnan(edges[i, col]))  # this walk is record_edges'
                m["q_pos"][i, col] = pi[q]
                m["ratio"][i, col] = max(ai[p], half) / abs(ai[p] - ai[q])
            near = np.concatenate(near)
            near = near[np.isfinite(near)]
            # (an infinite half compares exactly: every finite |c| is below it on both sides)
            m["clear"][i] = not (np.isfinite(half) and (np.abs(near - half) <= CLEARANCE * half).any())
    return m


# ---- the comparison ----------------------------------------------------------------------------------------------------------------------
def compare(got, m, N, k):
    """``got`` (ESTIMATE_DTYPE rows) against ``model``'s dict: counts and NaN patterns must be equal, every finite field within its
    bound.  Returns (worst ratio per field, records left out of the edge comparison for want of clearance, list of failures)."""
    h = N // k
    n = len(got)
    worst = dict(r=0.0, pair_mag=0.0, offset_bins=0.0, coherence=0.0, level=0.0, edge=0.0)
    bad = []
    if not (np.array_equal(got["n_pairs"], m["n_pairs"]) and np.array_equal(got["n_inside"], m["n_inside"])):
        bad.append(("counts", got["n_pairs"].tolist(), m["n_pairs"].tolist(), got["n_inside"].tolist(), m["n_inside"].tolist()))
        return worst, 0, bad
    left_out = 0

    def hold(field, i, g, w, allow):
        if np.isnan(g) != np.isnan(w):
            bad.append((field, i, "NaN pattern", float(g), float(w)))
            return
        if np.isnan(w):
            return
        if np.isinf(w) or np.isinf(g):
            if g != w:
                bad.append((field, i, "infinity", float(g), float(w)))
            return
        key = "edge" if field in ("rise", "fall") else "r" if field in ("r_re", "r_im") else field
        ratio = abs(g - w) / allow if allow > 0 else (0.0 if g == w else np.inf)
        worst[key] = max(worst[key], float(ratio))
        if not ratio <= 1.0:
            bad.append((field, i, float(g), float(w), float(allow), float(ratio)))

    for i in range(n):
        npair, M = int(m["n_pairs"][i]), float(m["pair_mag"][i])
        d_comp = C1 * (npair + 4) * U * M
        hold("r_re", i, got["r_re"][i], m["r_re"][i], d_comp)
        hold("r_im", i, got["r_im"][i], m["r_im"][i], d_comp)
        hold("pair_mag", i, got["pair_mag"][i], M, d_comp)
        absR = math.hypot(m["r_re"][i], m["r_im"][i]) if np.isfinite(m["r_re"][i]) and np.isfinite(m["r_im"][i]) else np.nan
        d_R = math.sqrt(2.0) * d_comp
        if npair and absR > 0 and np.isfinite(M):
            turn = d_R / absR
            if turn < 0.5:
                hold("offset_bins", i, got["offset_bins"][i], m["offset_bins"][i], k / (2.0 * math.pi) * turn + c2(k) * U)
            elif not (np.isfinite(got["offset_bins"][i]) and abs(got["offset_bins"][i]) <= k / 2.0):
                # (R cancels to within its own round-off: the frames do not determine its angle, but an angle it is)
                bad.append(("offset_bins", i, "no angle", float(got["offset_bins"][i]), float(m["offset_bins"][i])))
            hold("coherence", i, got["coherence"][i], m["coherence"][i], abs(m["coherence"][i]) * (turn + d_comp / M + 4 * U))
        else:
            for f in ("offset_bins", "coherence"):
                if np.isnan(got[f][i]) != np.isnan(m[f][i]) and not (f == "offset_bins" and npair and absR == 0):
                    bad.append((f, i, "NaN pattern", float(got[f][i]), float(m[f][i])))
        hold("level", i, got["level"][i], m["level"][i], 2.0 * float(np.spacing(abs(m["level"][i]))) if np.isfinite(m["level"][i]) else 0.0)
        if not m["clear"][i]:
            left_out += 1
            continue
        for col, f in enumerate(("rise", "fall")):
            mass = 2.0 * (abs(m["q_pos"][i, col]) + h) + 2.0 * (abs(m["q_pos"][i, col]) + h + 0.5 * N)  # the four roundings of the sums
            allow = h * C3 * U * m["ratio"][i, col] + U * mass if np.isfinite(m["ratio"][i, col]) else 0.0
            hold(f, i, got[f][i], m[f][i], allow)
    return worst, left_out, bad


PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "record_estimates_worst_ratio.txt")


def format_worst(title, worst):
    """``worst``: {case: {field: worst |got - model| / bound}} -> the lines of one half of the profile"""
    fields = ("r", "pair_mag", "offset_bins", "coherence", "level", "edge")
    lines = [title, f"{'case':<34} " + " ".join(f"{f:>11}" for f in fields)]
    for name in sorted(worst):
        lines.append(f"{name:<34} " + " ".join(f"{worst[name][f]:11.3f}" for f in fields))
    return "\n".join(lines) + "\n"


def write_worst(half, text, path=PROFILE):
    """replace the ``half`` ("cpu" or "gpu") of the profile: the halves are kept apart by marker lines"""
    head = ("record_estimates: worst |row - model| / bound per case and field (tests/record_estimates_cases.py derives the bounds; 1.000 is the\n"
            "limit).  r: the components of R; edge: rise and fall.\n")
    halves = {"cpu": "(not written yet)\n", "gpu": "(not measured yet)\n"}
    if os.path.exists(path):
        parts = open(path).read().split("==== ")
        for part in parts[1:]:
            name, _, body = part.partition(" ====\n")
            if name in halves:
                halves[name] = body
    halves[half] = text
    with open(path, "w") as f:
        f.write(head + "".join(f"==== {name} ====\n{halves[name]}" for name in ("cpu", "gpu")))


# ---- size edges: boxcar, bin-centred tones switched at segment borders (tests/detect_order_cases.py), nperseg 32 --------------------
EDGE_N, EDGE_T, EDGE_BIN, EDGE_CALLS = 32, 200, 5, 2
EDGE_INSIDE = (1, 2, 3, 63, 64, 65, 127, 128, 129)  # inside frames at k = 1: the lane count, one and two rounds, either side
EDGE_LONG = 70                                      # cells of the record read again at k = 16: (70 - 1) * 16 + 1 = 1105 frames
# per stream, per call: (first segment of the pulse, its segments).  A record is the pulse's cells and the cold cell before it, so
# a pulse of r segments makes r + 1 inside frames at k = 1; only a pulse on segment 0 of a first buffer has no cell before it.
EDGE_PULSES = (
    ((0, 1), None),                  # 1 inside frame; margin 0 or not, nothing delivered lies below half: both edges NaN
    ((10, 1), (3, 2)),               # 2
    ((10, 2), None),                 # 3
    ((10, 62), None), ((10, 63), None), ((10, 64), None),
    ((10, 126), None), ((10, 127), None), ((10, 128), None),
    ((10, EDGE_LONG - 1), None),     # the long record
    ((EDGE_T - 5, 5), (0, 4)),       # runs to the buffer's end: the reference reports it in call 2, begun in the previous buffer
)
EDGE_S = len(EDGE_PULSES)


def edge_settings():
    from tests import detect_order_cases as doc

    return dict(sample_rate=doc.FS, fft_nperseg=EDGE_N, fft_window=doc.WINDOW, signal_threshold_dbw=doc.THRESHOLD_DBW, snr_threshold_db=doc.SNR_DB,
                signal_min_duration_ms=0.5 * doc.hop_ms(EDGE_N), signal_max_duration_ms=doc.MAX_HOPS * doc.hop_ms(EDGE_N))


def edge_feed(call):
    """complex64 [EDGE_S, EDGE_T * EDGE_N]: the buffers of ``call``"""
    from tests import detect_order_cases as doc

    rows = []
    for s, pulses in enumerate(EDGE_PULSES):
        p = pulses[call]
        rows.append(doc.plant(EDGE_N, EDGE_T, [(EDGE_BIN, p[0], p[1], doc.TONE_DBW)] if p else [], seed=100 * call + s))
    return np.stack(rows)


def edge_oracle_records():
    """[call][stream] -> [(fi, start, end)] from the oracle, the look-back carried from call to call"""
    from oracle import analyze_oracle as oracle
    from tests import detect_order_cases as doc

    kw = edge_settings()
    p = oracle.ExtractParams(kw["signal_threshold_dbw"], kw["snr_threshold_db"], kw["signal_min_duration_ms"], kw["signal_max_duration_ms"])
    out, last = [], [None] * EDGE_S
    for call in range(EDGE_CALLS):
        x = edge_feed(call)
        per = []
        for s in range(EDGE_S):
            _, times, spec = oracle.stft_power(x[s], doc.FS, doc.WINDOW, EDGE_N)
            per.append([(int(r.fi), int(r.start), int(r.end)) for r in oracle.extract_records(times, spec, last[s], p)])
            last[s] = spec
        out.append(per)
    return out
