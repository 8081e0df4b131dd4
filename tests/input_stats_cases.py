"""rt_fetch_input_stats: the NumPy model and the case table the CPU and the GPU suite share.

A ROW of a case is the raw component array of one stream, interleaved I, Q, in the wire dtype of its format: uint8, int8, int16,
float32 (complex64) or float64 (complex128).  ``model_row`` restates the header's contract (include/rt_analyze.h) with nothing of the
kernels' order in it: the integer formats' sums are Python integers (exact at any length) converted to float once, the float
formats' are ``math.fsum`` over the finite components -- the correctly rounded sum, which every summation order of m terms
approaches within ``(m - 1) u sum|terms|`` (u = 2^-53); the tests allow ``(m + 1) u``, the two extra covering the rounded square of
a complex128 component (float32 squares are exact in float64) and fsum's own rounding.
"""
import math

import numpy as np

from pyradiotracking_amd import _native

FORMATS = ("c64", "u8", "i16", "i8", "c128")  # in the order of the kernels' format numbers 0 ... 4
FMT_CODE = {f: i for i, f in enumerate(FORMATS)}
PUBLIC_FORMAT = {"c64": 0, "u8": 1, "i16": 2, "i8": 3, "c128": 0}
UNIT = {"c64": 1, "u8": 255, "i16": 32768, "i8": 128, "c128": 1}
DTYPE = {"c64": np.float32, "u8": np.uint8, "i16": np.int16, "i8": np.int8, "c128": np.float64}
RAILS = {"u8": (0, 255), "i8": (-128, 127), "i16": (-32768, 32767)}
SAMPLE_BYTES = {f: 2 * np.dtype(DTYPE[f]).itemsize for f in FORMATS}
U = 2.0 ** -53


def is_float(fmt):
    return fmt in ("c64", "c128")


def raw_int(fmt, comps):
    """the raw components of an integer row as int64: uint8 2 b - 255, int8 and int16 the integer"""
    c = np.asarray(comps).astype(np.int64)
    return 2 * c - 255 if fmt == "u8" else c


def model_row(fmt, comps):
    """-> dict of the fields of rt_input_stats for one stream's row; the float formats' entry ``abs_terms`` holds fsum(|terms|) of
    the three sums for the bound"""
    comps = np.asarray(comps, dtype=DTYPE[fmt])
    assert comps.ndim == 1 and comps.size % 2 == 0
    n = comps.size // 2
    out = dict(n_samples=n, format=PUBLIC_FORMAT[fmt], unit=UNIT[fmt])
    if not is_float(fmt):
        lo, hi = RAILS[fmt]
        raw = raw_int(fmt, comps)  # int64: |raw| <= 2^15, so a sum of 2^32 squares stays below 2^63 -- exact
        assert comps.size < 2 ** 32
        total = [int(np.sum(x, dtype=np.int64)) for x in (raw[0::2], raw[1::2], raw * raw)]  # Python integers, converted once
        out.update(n_rail=int(np.count_nonzero((comps == lo) | (comps == hi))), n_nonfinite=0,
                   sum_i=float(total[0]), sum_q=float(total[1]), sum_sq=float(total[2]), peak=float(np.max(np.abs(raw), initial=0)))
        return out
    c = comps.astype(np.float64)
    fin = np.isfinite(c)
    ci, cq = c[0::2][fin[0::2]], c[1::2][fin[1::2]]
    both = c[fin]
    sq = both * both  # (exact for float32 values; one rounding each for float64 values: the bound's extra term)
    out.update(n_rail=int(np.count_nonzero(np.abs(both) >= 1.0)), n_nonfinite=int(np.count_nonzero(~fin)),
               sum_i=math.fsum(ci), sum_q=math.fsum(cq), sum_sq=math.fsum(sq), peak=float(np.max(np.abs(both), initial=0.0)),
               abs_terms=dict(sum_i=math.fsum(np.abs(ci)), sum_q=math.fsum(np.abs(cq)), sum_sq=math.fsum(sq)))
    return out


def float_bounds(fmt, model):
    """|got - fsum| allowed for the three sums of a float row: (m + 1) u fsum(|terms|), m the number of terms"""
    n = model["n_samples"]
    return {name: (m + 1) * U * model["abs_terms"][name] for name, m in (("sum_i", n), ("sum_q", n), ("sum_sq", 2 * n))}


def compare(fmt, got, model, what=""):
    """``got``: one INPUT_STATS_DTYPE row.  Integer formats: every field equal.  Float formats: counts, peak, format and unit
    equal, the sums within ``float_bounds``.  Returns the worst |got - model| / bound of the sums (0.0 for an integer row)."""
    for name in ("n_samples", "n_rail", "n_nonfinite", "format", "unit"):
        assert int(got[name]) == model[name], (what, fmt, name, int(got[name]), model[name])
    assert float(got["peak"]) == model["peak"], (what, fmt, "peak", float(got["peak"]), model["peak"])
    if not is_float(fmt):
        for name in ("sum_i", "sum_q", "sum_sq"):
            assert float(got[name]) == model[name], (what, fmt, name, float(got[name]), model[name])
        return 0.0
    worst = 0.0
    for name, bound in float_bounds(fmt, model).items():
        err = abs(float(got[name]) - model[name])
        assert err <= bound, (what, fmt, name, float(got[name]), model[name], err, bound)
        if bound > 0.0:
            worst = max(worst, err / bound)
    return worst


# ---- rows ----
SPECIALS = (1.0, -1.0, 1.5, -0.0, 5e-324, np.nan, np.inf, -np.inf)  # planted into float rows (the denormal: float64's smallest;
                                                                    # a complex64 row gets float32's, 1.4e-45)


def random_row(fmt, n, seed, chunk, specials=True):
    """``n`` samples of random full-range values (float: 0.3 * Gaussian) with rails planted at samples 0, chunk - 1, chunk and
    n - 1 -- I at one rail, Q at the other -- and, float rows with ``specials``, the SPECIALS spread over the row."""
    rng = np.random.default_rng([seed, FMT_CODE[fmt], n])
    if is_float(fmt):
        c = (0.3 * rng.standard_normal(2 * n)).astype(DTYPE[fmt])
        lo, hi = -1.0, 1.0
    else:
        lo, hi = RAILS[fmt]
        c = rng.integers(lo, hi + 1, 2 * n).astype(DTYPE[fmt])
    for j in (0, chunk - 1, chunk, n - 1):
        if 0 <= j < n:
            c[2 * j], c[2 * j + 1] = lo, hi
    if is_float(fmt) and specials and n >= 64:
        tiny = np.float32(1.4e-45) if fmt == "c64" else 5e-324
        spots = rng.choice(np.arange(2, 2 * n - 2), size=len(SPECIALS), replace=False)
        for k, v in zip(spots, SPECIALS):
            c[k] = tiny if v == 5e-324 else v
    return c


def constant_row(fmt, n, value):
    return np.full(2 * n, value, dtype=DTYPE[fmt])


def sizes(chunk):
    """n_samples of the size cases: nothing, one sample, less than a segment of 256, around the chunk length, several chunks and a
    ragged end"""
    return (0, 1, 255, chunk - 1, chunk, chunk + 1, 3 * chunk + 17)


def table(chunk):
    """The case table: (name, fmt, row).  Random rows of every format at every size, the accumulator-width rows (every component
    at a rail, or zero) over 3 chunks + 17, and float rows with every special value."""
    out = []
    for fmt in FORMATS:
        for n in sizes(chunk):
            out.append((f"{fmt} random n={n}", fmt, random_row(fmt, n, 1, chunk)))
    big = 3 * chunk + 17
    for fmt, value in (("i16", -32768), ("i16", 32767), ("u8", 255), ("u8", 0), ("i8", -128), ("i8", 127), ("u8", 128), ("i16", 0), ("i8", 0)):
        out.append((f"{fmt} all {value}", fmt, constant_row(fmt, big, value)))
    for fmt in ("c64", "c128"):
        out.append((f"{fmt} all 1.0", fmt, constant_row(fmt, big, 1.0)))
        out.append((f"{fmt} all NaN", fmt, constant_row(fmt, 300, np.nan)))
        out.append((f"{fmt} all -0.0", fmt, constant_row(fmt, 300, -0.0)))
    return out


def stats_array(rows):
    """model dicts -> an INPUT_STATS_DTYPE array (for input_levels)"""
    out = np.zeros(len(rows), dtype=_native.INPUT_STATS_DTYPE)
    for i, m in enumerate(rows):
        for name in out.dtype.names:
            out[name][i] = m[name]
    return out


# ---- a NumPy restatement that takes planted faults (tests/test_input_stats_contract.py) ----
FAULTS = ("square32", "low_rail", "ragged", "nan_added", "u8_minus_128")


def restated_row(fmt, comps, fault=None, nperseg=256):
    """The contract again, vectorised, with one of FAULTS planted:
    ``square32``     the squares accumulate in 32 bits (wrapping)
    ``low_rail``     -128 / -32768 (and uint8 0) do not count as a rail
    ``ragged``       the samples past the last whole segment of ``nperseg`` are left out
    ``nan_added``    non-finite components are counted AND added
    ``u8_minus_128`` uint8 raw taken as b - 128
    """
    comps = np.asarray(comps, dtype=DTYPE[fmt])
    n = comps.size // 2
    if fault == "ragged":
        n = n // nperseg * nperseg
        comps = comps[:2 * n]
    out = dict(n_samples=n, format=PUBLIC_FORMAT[fmt], unit=UNIT[fmt])
    if not is_float(fmt):
        lo, hi = RAILS[fmt]
        raw = comps.astype(np.int64) - 128 if (fmt == "u8" and fault == "u8_minus_128") else raw_int(fmt, comps)
        rail = (comps == hi) if fault == "low_rail" else (comps == lo) | (comps == hi)
        sq = raw * raw
        if fault == "square32":
            with np.errstate(over="ignore"):
                total_sq = int(np.sum(sq.astype(np.uint32), dtype=np.uint32))
        else:
            total_sq = int(np.sum(sq, dtype=np.int64))
        out.update(n_rail=int(np.count_nonzero(rail)), n_nonfinite=0, sum_i=float(int(np.sum(raw[0::2], dtype=np.int64))),
                   sum_q=float(int(np.sum(raw[1::2], dtype=np.int64))), sum_sq=float(total_sq), peak=float(np.max(np.abs(raw), initial=0)))
        return out
    c = comps.astype(np.float64)
    fin = np.isfinite(c)
    use = np.ones_like(fin) if fault == "nan_added" else fin
    with np.errstate(invalid="ignore", over="ignore"):
        both = c[fin]
        out.update(n_rail=int(np.count_nonzero(np.abs(both) >= 1.0)), n_nonfinite=int(np.count_nonzero(~fin)),
                   sum_i=float(np.sum(c[0::2][use[0::2]])), sum_q=float(np.sum(c[1::2][use[1::2]])), sum_sq=float(np.sum(c[use] * c[use])),
                   peak=float(np.max(np.abs(both), initial=0.0)))
    return out


def rejects(fmt, got, model):
    """does ``compare`` refuse the row ``got`` (a dict)?"""
    row = stats_array([dict(got)])[0] if not any(isinstance(v, float) and math.isnan(v) for v in got.values()) else None
    if row is None:
        return True  # (a NaN sum: no bound holds it)
    try:
        compare(fmt, row, model)
    except AssertionError:
        return True
    return False
