"""Float64 reference of the STFT power map and a float32 round-off model for it -- test infrastructure.

The oracle (``oracle/analyze_oracle.py``) restates SciPy's float32 arithmetic; comparing a kernel with it can only use
tolerances wide enough for two independent float32 round-offs.  This module computes the same operation in float64 on the
exact inputs the float32 arithmetic sees, and bounds what an honest float32 implementation may differ from it, cell by cell
and record field by record field.  ``tests/test_precision_model.py`` holds the model against SciPy's own float32 transform
(and float32 restatements of the kernels' other forms) and shows that it rejects results that are subtly wrong;
``tests/test_gpu_float64.py`` holds the HIP kernels to it.

Inputs of the reference operation (``stft_power_f64``)
------------------------------------------------------
* the complex64 samples; for the uint8 wire format the kernel's own conversion (``synth.u8_to_complex64_like_kernel``);
* the window cast to float32, as SciPy casts it to the input dtype (``_spectral_py.py:2083``);
* ``scale = 1 / (fs * sum(w*w))`` as SciPy evaluates it in float32 (the value ``rt_config.scale`` carries);
* the exact mean of each segment subtracted before windowing (``detrend='constant'``).

Cell model (amplitude of bin k of segment t)
--------------------------------------------
    e(t, k) = u * ( C_FFT * G * ||w y_t||_2  +  C_DC * mu_t * |W_k| )

u = 2**-24 (float32 unit round-off), W = DFT(w) (exact), mu_t = mean_n |x_t[n]| (a float32 sum's error is relative to the sum
of the magnitudes, so this, not |m_t|, bounds the rounding of the segment mean m_t), and ``y_t`` what the form transforms:

* ``"sub"`` -- subtract-first (SciPy's order; the kernels' ``subtract_first`` form, uint8 input, windows that are not
  cosine sums of order <= 1, ``stft_wg``, the general transforms): y_t = x_t - m_t.
* ``"lin"`` -- detrend by linearity (the fused scans' default for hamming / hann / boxcar on complex64):
  X = FFT(w x) - m W, so the transform sees the undetrended segment, y_t = x_t.  The C_DC term is the same in both forms: the
  rounding of the float32 mean leaks into the window's main lobe (all of W for ``lin``, whose W is confined to bins 0, +-1).

G is the depth of the transform.  The normwise error of an M-point float32 FFT, sum_k |dX_k|^2 <= (c u log2 M)^2 M ||w y||^2,
spread evenly over the M bins gives u log2(M) ||w y|| per bin; the worst bin of a map lies further out than that, and the
more so the longer the transform (cells 80 - 100 dB under a strong tone, Nyquist bins of an undetrended offset): over the
model tests' sweep SciPy's worst bin grows as M^(1/4) times the even share, from 8 to 16 384 points.  Hence
G = log2(M) M^(1/4) for a direct transform of length M = nperseg and, for Bluestein's algorithm (``"bluestein"``: two
transforms of the padded length M = gen_m, the next power of two >= 2 nperseg - 1, with chirp multiplies before, between and
after them), G = (2 log2(M) + C_CHIRP) M^(1/4).

Power: dP = scale * (2 |X| e + e^2) + C_POW * u * P (the square, the multiply by scale and the final rounding).

Record bounds (propagated from the cell bounds)
-----------------------------------------------
* ``max_p``  : max of dP over the plateau's cells (|max(a + d) - max(a)| <= max |d|).
* ``mean_p`` : mean of dP + (n + 2) u mean(P) for a float32 sum of the n cells and the division.
* ``row_mean``: K_RSS sqrt(sum_t dP_fft^2) / T for the independent per-segment transform errors, plus the systematic
  part C_POW u mean(P), plus the summation term (L + G_PART + 2) u mean(P).  That term is the scheme the kernels
  document: float32 partial rows of at most ``L = segs_per_chunk`` cells per lane group, combined over at most G_PART = 16
  lane groups of a workgroup in float32, the partial rows added in float64 and rounded once (``row_sum_from_partials``,
  ``row_sums_dense``); SciPy's pairwise ``np.mean`` is inside it.  A sequential float32 sum over the whole row is not.
* ``std_db`` : population std is 1-Lipschitz in the RMS of its arguments, so
  |d std| <= rms_i (10 / ln 10) * -ln(1 - dP_i / P_i) + C_STD * u * max_i |dB_i|; a plateau holding a cell whose bound
  reaches its value (round-off far under a strong tone) gets an infinite bound on its own.
* Records with ``start < 0`` take those cells (and their bounds) from the previous buffer's map.
* NaN (tests/nonfinite_cases.py): a field that is NaN in float64 must be NaN, a finite one finite.  A record whose cells hold a
  NaN has NaN max, mean and std; a record of a row that holds a NaN elsewhere keeps its bounds on those and has a NaN ``row_mean``.

The constants were fixed from float32 arithmetic only (SciPy's pocketfft and the NumPy restatements in
``test_precision_model.py``), about 4x over the worst ratio those reach over the model tests' sweep.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np

from oracle import analyze_oracle as oracle

U = 2.0 ** -24  # float32 unit round-off

C_FFT = 4.0  # per-bin transform round-off, in units of u * G * ||w y||
C_DC = 16.0  # segment-mean rounding leaking through W_k, in units of u * mean|x_t| * |W_k|
C_CHIRP = 8.0  # Bluestein: the chirp multiplies, in units of log2 stages
C_POW = 4.0  # |X|^2, * scale, rounding to float32
K_RSS = 4.0  # independent per-segment errors in a row sum: this many standard deviations of their RSS
G_PART = 16  # lane groups combined in float32 into one partial row (the fused scans' workgroups)
C_STD = 8.0  # float32 log10 and np.std on dB values of magnitude |dB|

DB = 10.0 / math.log(10.0)


def window_f32(window, nperseg: int) -> np.ndarray:
    """The coefficients SciPy multiplies with (cast to the complex64 input's dtype), as float64."""
    return oracle.window_coefficients(window, nperseg).astype(np.complex64).real.astype(np.float64)


def scale_f32(window, nperseg: int, fs) -> float:
    """``1 / (fs * sum(w*w))`` evaluated as SciPy does for complex64 input (float32)."""
    win = oracle.window_coefficients(window, nperseg).astype(np.complex64)
    return float(np.float32((1.0 / (fs * (win * win).sum())).real))


def bluestein_m(nperseg: int) -> int:
    m = 1
    while m < 2 * nperseg - 1:
        m <<= 1
    return m


@dataclass
class Ref64:
    """Float64 power map of one stream and what the bound needs; maps are [T, F] (segment-major, like the kernels')."""

    P: np.ndarray  # power, float64
    absX: np.ndarray  # |X| of the detrended transform
    norm_sub: np.ndarray  # [T] ||w (x_t - m_t)||_2
    norm_lin: np.ndarray  # [T] ||w x_t||_2
    abs_m: np.ndarray  # [T] mean_n |x_t[n]| (what bounds the float32 mean's rounding)
    absW: np.ndarray  # [F] |DFT(w)|
    scale: float
    nperseg: int


def stft_power_f64(x, fs, window, nperseg: int) -> Ref64:
    """The reference operation (``oracle.stft_power``) in float64 on the inputs its float32 arithmetic sees; ``x`` is the
    complex64 stream (for uint8 input: ``synth.u8_to_complex64_like_kernel`` of the bytes)."""
    x = np.asarray(x)
    assert x.dtype == np.complex64, x.dtype
    w = window_f32(window, nperseg)
    scale = scale_f32(window, nperseg, fs)
    T = x.shape[-1] // nperseg
    seg = x[: T * nperseg].astype(np.complex128).reshape(T, nperseg)
    m = seg.mean(axis=1)
    y = seg - m[:, None]
    X = np.fft.fft(w * y, axis=1)
    P = (X.real ** 2 + X.imag ** 2) * scale
    norm_sub = np.sqrt(((np.abs(y) * w) ** 2).sum(axis=1))
    norm_lin = np.sqrt(((np.abs(seg) * w) ** 2).sum(axis=1))
    return Ref64(P, np.abs(X), norm_sub, norm_lin, np.abs(seg).mean(axis=1), np.abs(np.fft.fft(w)), scale, nperseg)


def depth(nperseg: int, transform: str = "direct") -> float:
    if transform == "direct":
        return math.log2(nperseg) * nperseg ** 0.25
    if transform == "bluestein":
        m = bluestein_m(nperseg)
        return (2.0 * math.log2(m) + C_CHIRP) * m ** 0.25
    raise ValueError(transform)


def transform_of(nperseg: int) -> str:
    """What the kernels run at this size: Bluestein's algorithm for every size that is not a power of two."""
    return "direct" if nperseg & (nperseg - 1) == 0 else "bluestein"


@dataclass
class Bounds:
    dP: np.ndarray  # [T, F] total cell bound
    dP_fft: np.ndarray  # [T, F] its independent (per-segment) part


def cell_bounds(ref: Ref64, form: str = "sub", transform: Optional[str] = None) -> Bounds:
    transform = transform or transform_of(ref.nperseg)
    norm = {"sub": ref.norm_sub, "lin": ref.norm_lin}[form]
    g = depth(ref.nperseg, transform)
    e = U * (C_FFT * g * norm[:, None] + C_DC * ref.abs_m[:, None] * ref.absW[None, :])
    dP_fft = ref.scale * (2.0 * ref.absX * e + e * e)
    return Bounds(dP_fft + C_POW * U * ref.P, dP_fft)


def cell_ratios(got: np.ndarray, ref: Ref64, b: Bounds) -> np.ndarray:
    """|got - P| / dP per cell (> 1: outside the model)."""
    return np.abs(np.asarray(got, dtype=np.float64) - ref.P) / b.dP


def row_mean_bound(ref: Ref64, b: Bounds, L: int) -> np.ndarray:
    """[F] bound on the row mean of every bin for partial rows of ``L`` segments per lane group."""
    T = ref.P.shape[0]
    mean = ref.P.mean(axis=0)
    return K_RSS * np.sqrt((b.dP_fft ** 2).sum(axis=0)) / T + (C_POW + L + G_PART + 2) * U * mean


# ----------------------------------------------------------------------------------------------------------------------
# records
# ----------------------------------------------------------------------------------------------------------------------
def _cells(a_cur: np.ndarray, a_prev: Optional[np.ndarray], fi: int, start: int, end: int) -> np.ndarray:
    if start < 0:
        return np.concatenate((a_prev[start:, fi], a_cur[:end, fi]))
    return a_cur[start:end, fi]


def oracle_record_fields(records, spec: np.ndarray, spec_prev: Optional[np.ndarray]) -> np.ndarray:
    """The linear fields of the oracle's records (``OracleRecord``), as its float32 arithmetic forms them
    (analyze.py:442-447 via ``extract_records``), from the oracle's map ``spec`` [F, T]."""
    out = np.zeros(len(records), dtype=[("fi", "<i4"), ("start", "<i4"), ("end", "<i4"), ("max_p", "<f4"), ("mean_p", "<f4"),
                                        ("std_db", "<f4"), ("row_mean", "<f4")])
    for i, r in enumerate(records):
        row = spec[r.fi]
        cells = np.concatenate((spec_prev[r.fi][r.start:], row[: r.end])) if r.start < 0 else row[r.start : r.end]
        out[i] = (r.fi, r.start, r.end, np.max(cells), np.mean(cells), np.std(oracle.to_db(cells)), np.mean(row))
    return out


@dataclass
class FieldCheck:
    worst: Dict[str, float]  # field -> worst |got - ref| / bound
    failures: list


def record_bounds(rec, ref: Ref64, b: Bounds, L: int, ref_prev: Optional[Ref64] = None, b_prev: Optional[Bounds] = None):
    """Per record: (want, bound) of max_p, mean_p, row_mean, std_db in float64."""
    rm = ref.P.mean(axis=0)
    rmb = row_mean_bound(ref, b, L)
    out = []
    for r in rec:
        fi, s, e = int(r["fi"]), int(r["start"]), int(r["end"])
        P = _cells(ref.P, ref_prev.P if ref_prev is not None else None, fi, s, e)
        dP = _cells(b.dP, b_prev.dP if b_prev is not None else None, fi, s, e)
        n = len(P)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(P > 0, dP / P, np.inf)
            ddb = np.where(q < 1, -DB * np.log1p(-np.minimum(q, 1 - 1e-16)), np.inf)
            dbs = DB * np.log(P)
            std = float(np.std(dbs)) if np.all(P > 0) else float("nan")
        std_b = float(np.sqrt(np.mean(ddb ** 2))) + C_STD * U * float(np.max(np.abs(dbs))) if np.all(P > 0) else float("inf")
        if np.isnan(P).any():
            # a NaN cell (a non-finite sample's column), in this buffer or in the look-back: max, mean and std are NaN in the
            # reference (np.max propagates it) and must be NaN here -- the std too, which a zero cell would leave unbounded
            std, std_b = float("nan"), 0.0
        out.append({
            "max_p": (float(P.max()), float(dP.max())),
            "mean_p": (float(P.mean()), float(dP.mean()) + (n + 2) * U * float(P.mean())),
            "row_mean": (float(rm[fi]), float(rmb[fi])),
            "std_db": (std, std_b),
        })
    return out


def check_records(rec, ref: Ref64, b: Bounds, L: int, ref_prev: Optional[Ref64] = None, b_prev: Optional[Bounds] = None,
                  what: str = "") -> FieldCheck:
    """Every record's float fields against float64 within the model; ``rec`` has the fields of ``rt_record``."""
    worst = {k: 0.0 for k in ("max_p", "mean_p", "row_mean", "std_db")}
    failures = []
    for r, bd in zip(rec, record_bounds(rec, ref, b, L, ref_prev, b_prev)):
        for k, (want, bound) in bd.items():
            got = float(r[k])
            if k == "std_db" and not np.isfinite(bound):
                continue
            if np.isnan(want) or np.isnan(got):
                ratio = 0.0 if (np.isnan(want) and np.isnan(got)) else np.inf
            else:
                ratio = abs(got - want) / bound if bound > 0 else (0.0 if got == want else np.inf)
            worst[k] = max(worst[k], ratio)
            if ratio > 1.0:
                failures.append(f"{what} fi={int(r['fi'])} [{int(r['start'])},{int(r['end'])}) {k}: {got!r} vs {want!r} "
                                f"(|d| {abs(got - want):.3e}, bound {bound:.3e})")
    return FieldCheck(worst, failures)
