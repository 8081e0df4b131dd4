"""Helpers of the record-cells tests (RT_FLAG_RECORD_CELLS): a NumPy restatement of ``rt::run_stats`` (csrc/rt_core.h) and the
reference's decision predicate, in the precision of the cells they are given."""
import numpy as np


def _fold64(x):
    """64 interleaved partials (element k to partial k mod 64, in k order), folded by halving: p[l] += p[l + off], off = 32 .. 1."""
    x = np.asarray(x, dtype=np.float64)
    pad = (-len(x)) % 64
    p = np.cumsum(np.concatenate((x, np.zeros(pad))).reshape(-1, 64), axis=0)[-1].copy()  # (cumsum: sequential, as the partials are)
    off = 32
    while off:
        p[:off] += p[off:2 * off]
        off //= 2
    return p[0]


def run_stats(cells):
    """(max_p, mean_p, std_db) of one record's cells as ``rt::run_stats`` computes them; max_p and mean_p bit for bit (float64
    sums of the cells, one rounding to the cells' type), std_db up to the platform's log10."""
    c = np.asarray(cells)
    P = c.dtype.type
    n = len(c)
    mx = P(np.nan) if np.isnan(c).any() else c.max()
    mean = P(_fold64(c) / np.float64(n))
    with np.errstate(divide="ignore", invalid="ignore"):
        d = (P(10) * np.log10(c)).astype(np.float64)
        mean_db = _fold64(d) / np.float64(n)
        std = P(np.sqrt(_fold64((d - mean_db) ** 2) / np.float64(n)))
    return mx, mean, std


def cell_above(c, row_mean, thr, snr):
    """``rt::cell_above``: ``!(c < thr) && !(c / row_mean < snr)`` in the type of ``c`` (analyze.py:370, 378)."""
    P = np.asarray(c).dtype.type
    with np.errstate(divide="ignore", invalid="ignore"):
        return ~(c < P(thr)) & ~(c / P(row_mean) < P(snr))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)
