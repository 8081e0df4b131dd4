"""Per-record band spectrum reduced on the device (``rt_fetch_record_spectrum``): the NumPy restatement of the kernel's order, the
model (``record_band_rows``, which defines the result), the bounds a row is held to and the comparison -- shared by
tests/test_record_spectrum_contract.py (CPU) and tests/test_gpu_record_spectrum.py (GPU).

Bounds, u = 2^-53.  Model and kernel start from the same frames, and p = re * re + im * im is two rounded products and a rounded
sum on both sides (NumPy's ``** 2`` is a product): the same bits.  So ``peak`` is held to equality.

mean.  A sum of n non-negative terms in any order is within (n - 1) u of itself relative, the division adds u: n u a side, 2 n u
between the sides; one more u covers the second order (n u)^2 for every n below 2^26.  EM = (2 n + 1) u, relative.

total.  The B = 2 w + 1 means carry EM each, and each side adds them with B - 1 roundings: ET = EM + 2 (B - 1) u, relative.

centre_share.  m_w / total: EM + ET, and u for each side's division: share (EM + ET + 2 u).

centroid.  S1 = sum m_j d_j: a term carries EM and one rounding a side for the product, the sums B - 1 roundings a side, all of
them relative to A1 = sum m_j |d_j|: dS1 = A1 (EM + 2 B u).  S1 / total: dC = dS1 / total + |centroid| (ET + 2 u).

width.  t_j = d_j - centroid differs by dC and a rounding a side: dt = dC + 2 u |t_j|.  t_j t_j and the product by m_j round once
a side each.  A term m_j t_j^2 is therefore off by m_j t_j^2 (EM + 8 u) + 2 m_j |t_j| dC, and the sums add 2 (B - 1) u S2:
dS2 = S2 (EM + (2 B + 6) u) + 2 dC sum m_j |t_j|.  var = S2 / total: dV = dS2 / total + var (ET + 2 u).  For the root,
|sqrt(a) - sqrt(b)| = |a - b| / (sqrt(a) + sqrt(b)) <= min(|a - b| / sqrt(b), sqrt(|a - b|)), and each side's root rounds once:
dW = min(dV / width, sqrt(dV)) + 2 u width.

peak_col.  The two sides can name different columns only where another mean lies within 2 EM of the largest: such a row has no
clearance, its peak_col and peak_bins are not compared and compare() counts it.

peak_bins.  a, b, c are logarithms of means that carry EM (the derivative of log is 1 / m: EM absolute), from a log that is within
1 ulp on the device (the ROCm device library's documented error for the double-precision log) and within 1 ulp in libm; an ulp is
at most 2 u relative: dL = EM + 4 u max(|a|, |b|, |c|).  num = a - c: dN = 2 dL + 2 u |num|.  den = (a - 2 b) + c, 2 b exact:
dD = 4 dL + 2 u (|a - 2 b| + |den|).  q = num / den: dQ = (dN + |q| dD) / (|den| - dD) + 2 u |q|, and nothing is claimed where
dD >= |den| / 2 (a top as flat as its own round-off: counted with the rows without clearance).  peak_bins = d_p + 0.5 q, the
half exact, the sum rounded once a side: dP = 0.5 dQ + 2 u (|d_p| + 0.5 |q|).
"""
import math
import os

import numpy as np

from pyradiotracking_amd import _native
from pyradiotracking_amd.analyze import record_band_rows
from tests import record_estimates_cases as ec
from tests import record_stft_hop_cases as hop

U = 2.0 ** -53
FAULTS = ("partial_shifted", "outside_counted", "last_maximum")
FAULT_FRAME = 5  # "partial_shifted": the inside frame that is added into partial (i + 1) mod 64 (moving every frame only turns the
#                  partials round, and the fold by halving gives a turned set the same bits)
FIELDS = ("mean", "total", "centre_share", "centroid", "width", "peak_bins")
SCALARS = ("total", "centre_share", "centroid", "width", "peak_bins")
EXACT = ("total", "peak_col", "n_inside")  # with mean and peak: the bytes of the restatement

_LANES = np.arange(64)


def plan_of(offsets, first_seg, start, end, N, k):
    """the inside runs [n, 4] (lo0, hi0, lo1, hi1) from the frame prefix ``offsets``: ``ec.work_plan`` on the segments the frames
    imply, as ``ec.restate`` derives them"""
    offsets = np.asarray(offsets, dtype=np.int64)
    first = np.asarray(first_seg, dtype=np.int64)
    n = len(offsets) - 1
    fr = np.diff(offsets)
    fp = np.minimum(hop.part_frames(np.maximum(-first, 0), k), fr)
    lp = np.where(fp > 0, (fp - 1) // k + 1, 0)
    fc = fr - fp
    L = np.zeros(n + 1, np.int64)
    L[1:] = np.cumsum(lp + np.where(fc > 0, (fc - 1) // k + 1, 0))
    plan = ec.work_plan(L * N, first, np.zeros(n, np.int64), start, end, N, k)
    assert plan is not None and np.array_equal(plan["frame_first"], offsets)
    return plan["range"].astype(np.int64)


def scalars(m, w, n_in, fault=None):
    """the kernel's scalars from one row of means, left to right: (total, centre_share, centroid, width, peak_bins, peak_col)"""
    nan = float("nan")
    B = 2 * w + 1
    m = [float(x) for x in m]
    if n_in == 0 or any(x != x for x in m):
        return nan, nan, nan, nan, nan, -1
    with np.errstate(all="ignore"):
        total, moment, best, col = np.float64(0.0), np.float64(0.0), np.float64(m[0]), 0
        for c in range(B):
            total = total + np.float64(m[c])
            moment = moment + np.float64(m[c]) * np.float64(c - w)
            if c > 0 and (m[c] >= best if fault == "last_maximum" else m[c] > best):
                best, col = np.float64(m[c]), c
        centroid = moment / total
        spread = np.float64(0.0)
        for c in range(B):
            t = np.float64(c - w) - centroid
            spread = spread + np.float64(m[c]) * (t * t)
        share, width = np.float64(m[w]) / total, np.sqrt(spread / total)
        peak_bins = nan
        if 0 < col < 2 * w and all(0.0 < m[j] < math.inf for j in (col - 1, col, col + 1)):
            la, lb, lc = (np.float64(math.log(m[j])) for j in (col - 1, col, col + 1))
            peak_bins = np.float64(col - w) + np.float64(0.5) * (la - lc) / ((la - np.float64(2.0) * lb) + lc)
    return float(total), float(share), float(centroid), float(width), float(peak_bins), col


def restate(offsets, first_seg, values, start, end, N, k, fault=None):
    """record_spectrum's arithmetic (csrc/rt_record_spectrum.h) on the frames ``values`` [n_frames, B] of ``fetch_record_band(k, w)``
    (``offsets`` in FRAMES): ``(rows, mean, peak)``.  ``fault``: one of FAULTS, planted."""
    assert fault is None or fault in FAULTS
    offsets = np.asarray(offsets, dtype=np.int64)
    v = np.asarray(values)
    n, B = len(offsets) - 1, v.shape[1]
    w = B // 2
    rng = plan_of(offsets, first_seg, start, end, N, k)
    rows = np.zeros(n, _native.SPECTRUM_DTYPE)
    mean, peak = np.full((n, B), np.nan), np.full((n, B), np.nan)
    with np.errstate(all="ignore"):
        re, im = v.real.astype(np.float64), v.imag.astype(np.float64)
        p = re * re + im * im
        for i in range(n):
            lo0, hi0, lo1, hi1 = (int(t) for t in rng[i])
            inside = np.concatenate([np.arange(lo0, hi0), np.arange(lo1, hi1)])
            if fault == "outside_counted":
                inside = np.arange(int(offsets[i + 1] - offsets[i]))
            n_in = len(inside)
            mine = p[offsets[i]:offsets[i + 1]]
            part, top = np.zeros((64, B)), np.full((64, B), -np.inf)
            for t0 in range(0, n_in, 64):  # inside frame i into partial i mod 64, in increasing i
                idx = inside[t0:t0 + 64]
                at = np.arange(len(idx))
                if fault == "partial_shifted" and t0 == 0 and n_in > FAULT_FRAME + 1:  # one frame lands in its neighbour's partial
                    part[FAULT_FRAME + 1] = part[FAULT_FRAME + 1] + mine[idx[FAULT_FRAME]]
                    top[FAULT_FRAME + 1] = np.maximum(top[FAULT_FRAME + 1], mine[idx[FAULT_FRAME]])
                    idx, at = np.delete(idx, FAULT_FRAME), np.delete(at, FAULT_FRAME)
                part[at] = part[at] + mine[idx]
                top[at] = np.maximum(top[at], mine[idx])
            m = 32
            while m >= 1:  # the fold by halving
                part = part + part[_LANES ^ m]
                top = np.maximum(top, top[_LANES ^ m])
                m //= 2
            if n_in:
                mean[i] = part[0] / np.float64(n_in)
                peak[i] = top[0]
            row = rows[i]
            row["total"], row["centre_share"], row["centroid"], row["width"], row["peak_bins"], row["peak_col"] = scalars(mean[i], w, n_in, fault)
            row["n_inside"] = n_in
    return rows, mean, peak


# ---- the model and its bounds -----------------------------------------------------------------------------------------------------------
def model(offsets, first_seg, values, start, end, N, k):
    """``record_band_rows`` on the same frames: (rows, mean, peak)"""
    return record_band_rows(offsets, first_seg, values, start, end, N, k)


def bounds(row, m):
    """the allowed |got - model| per field of one model row with the means ``m``; None for a field nothing is claimed of.  Also
    ``clear``: whether peak_col (and with it peak_bins) can be compared."""
    B = len(m)
    w = B // 2
    n = int(row["n_inside"])
    out = dict(mean=None, total=None, centre_share=None, centroid=None, width=None, peak_bins=None, clear=False)
    if n == 0 or np.isnan(m).any() or not np.isfinite(m).all():
        return out
    EM = (2 * n + 1) * U
    ET = EM + 2 * (B - 1) * U
    out["mean"] = EM * m
    total = float(row["total"])
    out["total"] = ET * total
    if not total > 0:
        return out
    d = np.arange(-w, w + 1, dtype=np.float64)
    out["centre_share"] = abs(float(row["centre_share"])) * (EM + ET + 2 * U)
    A1 = float((m * np.abs(d)).sum())
    cen = float(row["centroid"])
    dC = A1 * (EM + 2 * B * U) / total + abs(cen) * (ET + 2 * U)
    out["centroid"] = dC
    t = d - cen
    S2 = float((m * t * t).sum())
    dS2 = S2 * (EM + (2 * B + 6) * U) + 2 * dC * float((m * np.abs(t)).sum())
    dV = dS2 / total + S2 / total * (ET + 2 * U)
    width = float(row["width"])
    out["width"] = (min(dV / width, math.sqrt(dV)) if width > 0 else math.sqrt(dV)) + 2 * U * width
    col = int(row["peak_col"])
    others = np.delete(m, col)
    out["clear"] = not (len(others) and (np.abs(others - m[col]) <= 2 * EM * m[col]).any())
    if out["clear"] and np.isfinite(row["peak_bins"]):
        a, b, c = (math.log(float(m[j])) for j in (col - 1, col, col + 1))
        dL = EM + 4 * U * max(abs(a), abs(b), abs(c))
        num, den = a - c, (a - 2 * b) + c
        dN = 2 * dL + 2 * U * abs(num)
        dD = 4 * dL + 2 * U * (abs(a - 2 * b) + abs(den))
        if dD >= abs(den) / 2:
            out["clear"] = False
        else:
            q = num / den
            dQ = (dN + abs(q) * dD) / (abs(den) - dD) + 2 * U * abs(q)
            out["peak_bins"] = 0.5 * dQ + 2 * U * (abs(d[col]) + 0.5 * abs(q))
    return out


def compare(got, want):
    """``got`` = (rows, mean, peak) against the model's triple: counts and NaN patterns equal, ``peak`` equal, every other finite
    field within its bound.  Returns (worst ratio per field, rows whose peak_col and peak_bins were left out for want of clearance,
    list of failures)."""
    rows, mean, peak = got
    mrows, mmean, mpeak = want
    worst = dict.fromkeys(FIELDS, 0.0)
    bad = []
    if rows.shape != mrows.shape or mean.shape != mmean.shape or peak.shape != mpeak.shape or not np.array_equal(rows["n_inside"], mrows["n_inside"]):
        bad.append(("counts", rows["n_inside"].tolist(), mrows["n_inside"].tolist()))
        return worst, 0, bad
    left_out = 0

    def hold(field, i, g, w, allow):
        g, w = np.atleast_1d(np.asarray(g, np.float64)), np.atleast_1d(np.asarray(w, np.float64))
        if not np.array_equal(np.isnan(g), np.isnan(w)):
            bad.append((field, i, "NaN pattern", g.tolist(), w.tolist()))
            return
        fin = np.isfinite(w)
        if not np.array_equal(g[~fin & ~np.isnan(w)], w[~fin & ~np.isnan(w)]):
            bad.append((field, i, "infinity", g.tolist(), w.tolist()))
            return
        if allow is None:  # nothing derived (non-finite means): the patterns above are all that is held
            return
        allow = np.broadcast_to(np.asarray(allow, np.float64), w.shape)
        with np.errstate(all="ignore"):
            diff = np.abs(g[fin] - w[fin])
            ratio = np.where(allow[fin] > 0, diff / allow[fin], np.where(diff == 0, 0.0, np.inf))
        if len(ratio):
            worst[field] = max(worst[field], float(ratio.max()))
            if not ratio.max() <= 1.0:
                bad.append((field, i, g.tolist(), w.tolist(), allow.tolist(), float(ratio.max())))

    for i in range(len(rows)):
        b = bounds(mrows[i], mmean[i])
        hold("mean", i, mean[i], mmean[i], b["mean"])
        same_peak = np.array_equal(np.isnan(peak[i]), np.isnan(mpeak[i])) and np.array_equal(peak[i][~np.isnan(peak[i])], mpeak[i][~np.isnan(mpeak[i])])
        if not same_peak:
            bad.append(("peak", i, peak[i].tolist(), mpeak[i].tolist()))
        for f in ("total", "centre_share", "centroid", "width"):
            hold(f, i, rows[f][i], mrows[f][i], b[f])
        if np.isnan(mmean[i]).any():
            if rows["peak_col"][i] != -1 or mrows["peak_col"][i] != -1:
                bad.append(("peak_col", i, int(rows["peak_col"][i]), int(mrows["peak_col"][i])))
            hold("peak_bins", i, rows["peak_bins"][i], mrows["peak_bins"][i], None)
        elif b["clear"]:
            if rows["peak_col"][i] != mrows["peak_col"][i]:
                bad.append(("peak_col", i, int(rows["peak_col"][i]), int(mrows["peak_col"][i])))
            hold("peak_bins", i, rows["peak_bins"][i], mrows["peak_bins"][i], b["peak_bins"])
        else:
            left_out += 1
    return worst, left_out, bad


def same_bytes(got, want, fields=EXACT):
    """(rows, mean, peak) twice: the failures of "``mean``, ``peak`` and the ``fields`` of the rows are the same bytes" -- a NaN
    equals a NaN, whatever its payload (the kernel stores one quiet NaN, NumPy's arithmetic another)"""
    bad = []

    def eq(a, b):
        a, b = np.asarray(a), np.asarray(b)
        if a.shape != b.shape:
            return False
        if a.dtype.kind != "f":
            return np.array_equal(a, b)
        na, nb = np.isnan(a), np.isnan(b)
        return np.array_equal(na, nb) and a[~na].tobytes() == b[~nb].tobytes()

    for name, a, b in (("mean", got[1], want[1]), ("peak", got[2], want[2])) + tuple((f, got[0][f], want[0][f]) for f in fields):
        if not eq(a, b):
            bad.append(name)
    return bad


# ---- synthetic bands ---------------------------------------------------------------------------------------------------------------------
def band_of(x, fi, half, w, scale, N, k, first_segment=0):
    """``hop.one_part_record`` at every bin of the band: ``(offsets, first_segment, values [n_frames, 2 half + 1])``"""
    cols = [hop.one_part_record(x, (fi + j - half) % N, w, scale, N, k, first_segment) for j in range(2 * half + 1)]
    return cols[0][0], cols[0][1], np.stack([c[2] for c in cols], axis=1)


def tone_band(delta_bins, fi, half, N, k, window, n_seg=12, noise_db=-60.0, seed=0):
    """a tone ``delta_bins`` off bin ``fi`` over ``n_seg`` segments under noise: one record, all of one part"""
    from oracle import analyze_oracle as oracle

    w = oracle.window_coefficients(window, N)
    scale = 1.0 / (250000.0 * float((w ** 2).sum()))
    rng = np.random.default_rng([seed, int(round(delta_bins * 1000)) % 100003, k, N])
    n = np.arange(n_seg * N)
    sigma = 10.0 ** (noise_db / 20.0) / math.sqrt(2.0)
    x = np.exp(2j * np.pi * (fi + delta_bins) * n / N) + sigma * (rng.standard_normal(n.size) + 1j * rng.standard_normal(n.size))
    return band_of(x, fi, half, w, scale, N, k)


# ---- a small case at any nperseg: boxcar, bin-centred tones switched at segment borders (tests/detect_order_cases.py) ----------------
SMALL_T = 60


def small_settings(N):
    from tests import detect_order_cases as doc

    return dict(sample_rate=doc.FS, fft_nperseg=N, fft_window=doc.WINDOW, signal_threshold_dbw=doc.THRESHOLD_DBW, snr_threshold_db=doc.SNR_DB,
                signal_min_duration_ms=0.5 * doc.hop_ms(N), signal_max_duration_ms=doc.MAX_HOPS * doc.hop_ms(N))


def small_feed(N, pulses, seed=0):
    """complex64 [len(pulses), SMALL_T * N]: stream s holds the tone ``pulses[s]`` = (bin, first segment, segments)"""
    from tests import detect_order_cases as doc

    return np.stack([doc.plant(N, SMALL_T, [(b, t0, r, doc.TONE_DBW)], seed=1000 * seed + s) for s, (b, t0, r) in enumerate(pulses)])


# ---- the profiles ------------------------------------------------------------------------------------------------------------------------
_PROFILES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles")
PROFILE = os.path.join(_PROFILES, "record_spectrum_worst_ratio.txt")
ESTIMATORS = os.path.join(_PROFILES, "record_spectrum_estimators.txt")


def format_worst(title, worst):
    """``worst``: {case: {field: worst |got - model| / bound}} -> the lines of one half of the profile"""
    lines = [title, f"{'case':<40} " + " ".join(f"{f:>12}" for f in FIELDS)]
    for name in sorted(worst):
        lines.append(f"{name:<40} " + " ".join(f"{worst[name][f]:12.3f}" for f in FIELDS))
    return "\n".join(lines) + "\n"


def write_worst(half, text, path=PROFILE):
    """replace the ``half`` ("cpu" or "gpu") of the profile: the halves are kept apart by marker lines"""
    head = ("record_spectrum: worst |row - model| / bound per case and field (tests/record_spectrum_cases.py derives the bounds; 1.000 is the\n"
            "limit).  peak is held to equality and not listed.\n")
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


def write_estimators(path=None):
    """the error of peak_bins and centroid on model tones, as text and into ``path``: recorded, not asserted"""
    N, fi, k, half = 256, 50, 4, 2
    lines = ["record_spectrum: what peak_bins and centroid say of a model tone delta bins off bin 50's centre (nperseg 256, k = 4, w = 2, 12",
             "segments, noise 60 dB below the tone; tests/record_spectrum_cases.py: tone_band).  Errors in bins; recorded, not asserted.", "",
             f"{'window':<8} {'delta':>6} {'peak_bins':>10} {'error':>9} {'centroid':>10} {'error':>9} {'width':>7} {'share':>6}"]
    for window in ("hamming", "boxcar"):
        for delta in (0.0, 0.3, -0.45):
            off, first, values = tone_band(delta, fi, half, N, k, window)
            rows, _, _ = restate(off, first, values, [0], [12], N, k)
            r = rows[0]
            lines.append(f"{window:<8} {delta:6.2f} {r['peak_bins']:10.4f} {r['peak_bins'] - delta:9.4f} {r['centroid']:10.4f} {r['centroid'] - delta:9.4f} "
                         f"{r['width']:7.4f} {r['centre_share']:6.3f}")
    text = "\n".join(lines) + "\n"
    if path:
        with open(path, "w") as f:
            f.write(text)
    return text
