"""What tests/test_gpu_constant.py relies on, shown with the oracle alone (no GPU): tests/constant_cases.py.

* a constant complex64 segment made of int16 (hence int8) components cancels exactly under NumPy's mean, for every component value
  and every segment length of the table -- the contract "a segment whose samples are all one value is an all-zero column" is the
  reference's own behaviour, not an accident of the rails;
* every case holds the record it was built for: the constant segment's column is 0.0 in every bin, the record starts ON it, its
  ``std`` is NaN and its other four figures are finite; the full-mantissa control's column is NOT zero and its ``std`` finite;
* every decision is clear of its thresholds by the margin of tests/test_combo_contract.py (float64_cases.margin_ok);
* the detrend guard (rt_kernels.h: StftParams::dc_flag) is at least a factor 100 short of marking the target stream in every
  single-segment case and beyond it by more than that on the stream pinned to a rail: the linearity form is what analyses the
  former, the subtract-first kernels the latter;
* the table covers what it was asked to cover, by brute force."""
import itertools
import warnings

import numpy as np
import pytest

from oracle import analyze_oracle as oracle
from tests import constant_cases as cc
from tests import float64_cases as fc

SIZES = sorted({c.nperseg for c in cc.CASES})
NAMES = [c.name for c in cc.CASES]


# ---- cancellation -------------------------------------------------------------------------------------------------------------
def _cancels(values_re, values_im, nperseg, rows=2048):
    """x - mean(x) == 0 in every sample of every constant segment re + 1j im (float32 pairs), as oracle.stft_power forms it"""
    for a in range(0, len(values_re), rows):
        c = (values_re[a: a + rows] + 1j * values_im[a: a + rows]).astype(np.complex64)
        seg = np.repeat(c[:, None], nperseg, axis=1)
        d = seg - np.mean(seg, axis=-1, keepdims=True)
        if d.real.any() or d.imag.any():
            return False
    return True


@pytest.mark.parametrize("nperseg", SIZES)
def test_constant_int16_segments_cancel_exactly(nperseg):
    """All 65 536 int16 component values (value / 32768; in the real part ascending and in the imaginary part descending, so that
    both components see every value) at every size of the table, none left out.  int8 components (value / 128) are the multiples
    of 256 among them."""
    v = np.arange(-32768, 32768)
    f = (v.astype(np.float32) * np.float32(2.0 ** -15))
    assert _cancels(f, f[::-1].copy(), nperseg)


def test_the_rails_of_uint8_cancel_and_most_other_bytes_do_not():
    """fma(byte, float32(1 / 127.5), -1) has a full mantissa (byte 255 gives 1.0000001): constant segments of bytes 0 and 255 cancel
    at nperseg 256, most of the others leave a residue in the reference -- which is why the table uses the rails only."""
    from pyradiotracking_amd import synth
    b = np.arange(256, dtype=np.uint8)
    f = synth.u8_to_complex64_like_kernel(np.repeat(b, 2)).real.astype(np.float32)
    assert f[0] == -1.0 and abs(f[255] - 1.0) < 2e-7
    ok = [_cancels(f[i: i + 1], f[i: i + 1], 256) for i in range(256)]
    assert ok[0] and ok[255] and ok.count(False) > 100, ok.count(False)


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def _column(ref, k, t):
    """column t of buffer k's map (t < 0: of the previous buffer's, as the reference's walk reads it)"""
    return ref[k].spec[:, t] if t >= 0 else ref[k - 1].spec[:, t]


@pytest.mark.parametrize("name", NAMES)
def test_record_shape(name):
    c = cc.BY_NAME[name]
    ref = [row[cc.TARGET] for row in cc.reference(name)]
    lengths, consts, pulses, expect = cc.layout(c)
    fi = cc.tone_bin(c)
    full = c.fmt == "c64full"
    for k, t in consts:
        col = ref[k].spec[:, t]
        if full:
            assert col[fi] > 0.0, "the full-mantissa constant cancels in the reference after all"
        else:
            assert (col == 0.0).all(), (k, t, np.flatnonzero(col)[:4])
    for k, start, end in expect:
        mine = [r for r in ref[k].records if (r.fi, r.start, r.end) == (fi, start, end)]
        assert len(mine) == 1, (k, [(r.fi, r.start, r.end) for r in ref[k].records])
        r = mine[0]
        head = _column(ref, k, start)
        assert ((k, start) in consts) or ((k - 1, c.T - 1) in consts and start == -1)  # the head cell is the constant segment's
        if full:
            assert head[fi] > 0.0 and np.isfinite(r.std_db)
        else:
            assert head[fi] == 0.0 and np.isnan(r.std_db)
        assert all(np.isfinite(getattr(r, f)) for f in ("max_dbw", "avg_dbw", "noise_dbw", "snr_db"))
    # controls
    if c.placement in ("e_zero", "e_rail"):
        for k in range(len(ref)):
            assert ref[k].records == [] and (ref[k].spec == 0.0).all()
            with np.errstate(divide="ignore"):
                assert np.isneginf(oracle.to_db(ref[k].spec.mean(axis=1))).all()
    if c.placement == "e_lone":
        assert all(r.records == [] for r in ref)
    if c.placement == "d":
        assert lengths[0] % c.nperseg == c.nperseg // 2 and ref[0].spec.shape[1] == c.T  # the constant half segment is not analysed
        r = [r for r in ref[1].records if (r.fi, r.start, r.end) == (fi, -1, cc.tone_segs(c))]
        assert len(r) == 1 and np.isfinite(r[0].std_db)
    # the other streams hold records with a finite std, so that no comparison passes on NaN alone
    plain = [r for row in cc.reference(name) for r in row[cc.PLAIN].records]
    assert plain and all(np.isfinite(r.std_db) for r in plain)
    if c.placement in ("a", "a_x"):
        (k, t), = consts
        same_chunk = t // c.spc == (t + 1) // c.spc
        assert same_chunk == (c.placement == "a")


@pytest.mark.parametrize("name", NAMES)
def test_decision_margins(name):
    """float64_cases.margin_ok at the margin tests/test_combo_contract.py uses, on the rows that hold a cell not clearly under the
    absolute threshold (the others are clear of it by that and their SNR figures decide nothing), and the same for the previous
    map's last column against this map's row means (the only look-back cells a walk of these cases reaches)."""
    c = cc.BY_NAME[name]
    kw = cc.settings(c)
    p = oracle.ExtractParams(kw["signal_threshold_dbw"], 5.0, kw["signal_min_duration_ms"], 40, 0.0)
    rel = cc.MARGIN_REL
    for s in range(cc.S):
        before = None
        for row in cc.reference(name):
            spec = np.asarray(row[s].spec, dtype=np.float64)
            rows = ~(spec < p.signal_threshold * (1.0 - rel)).all(axis=1)
            if rows.any():
                assert fc.margin_ok(spec[rows], p.signal_threshold, p.snr_threshold, rel=rel), (name, s)
                if before is not None:
                    tail = before[rows][:, -2:]
                    ratio = tail / spec[rows].mean(axis=1, keepdims=True) / p.snr_threshold
                    near = (np.abs(ratio - 1.0) < rel) | (np.abs(tail / p.signal_threshold - 1.0) < rel)
                    assert not near.any(), (name, s)
            before = spec


# ---- the guard of the detrend by linearity ---------------------------------------------------------------------------------------
def lin_form(c):
    """the case is analysed by a LIN instantiation (rt_analyze.hip: launch_stft; rt_tables.h: fit_cosine_window)"""
    return (c.fmt != "u8" and c.precision == "float32" and c.window in ("hamming", "hann", "boxcar") and 32 <= c.nperseg <= 4096
            and c.nperseg & (c.nperseg - 1) == 0 and not dict(c.extra).get("subtract_first"))


def guard_ratios(c, x):
    """The guard's two inequalities on one buffer of one stream (complex128 [n]), evaluated as the kernels do (rt_kernels.h:
    stft_scan's epilogue; rt_scan64.h) but on the float64 map: a wave holds 64 / LG consecutive chunks of ``segs_per_chunk``
    segments up to nperseg 512 (LG = lanes per segment: 2, 4, 8 at 32, 64, 128, else nperseg / 16) and one chunk from 1024 on; with
    D = sum over its segments of |sum of the samples|^2, mn = the smallest row sum of a chunk (bins 0 and +-1 aside), tot = all its
    row sums, it marks the stream when  D > 1e6 N^2 fs mn chunks  and  D > 100 N fs tot.  (From nperseg 2048 on a wave holds a part
    of the bins: the smallest over all bins is no larger than its own, and the first inequality alone is what is asked for below.)
    Returns the (D / first limit, D / second limit) of the wave that comes closest to marking: both > 1 marks."""
    N = c.nperseg
    T = len(x) // N
    seg = x[: T * N].reshape(T, N)
    _, _, spec = oracle.stft_power(x, cc.FS, c.window, N)
    lg = {32: 2, 64: 4, 128: 8}.get(N, N // 16)
    per_wave = max(1, 64 // lg)
    d_seg = np.abs(seg.sum(axis=1)) ** 2
    n_chunks = (T + c.spc - 1) // c.spc
    keep = np.ones(N, dtype=bool)
    keep[[0, 1, N - 1]] = False
    best = None
    for w0 in range(0, n_chunks, per_wave):
        chunks = range(w0, min(w0 + per_wave, n_chunks))
        rows = np.stack([spec[:, ch * c.spc: (ch + 1) * c.spc].sum(axis=1) for ch in chunks])
        d = float(sum(d_seg[ch * c.spc: (ch + 1) * c.spc].sum() for ch in chunks))
        lim1 = 1e6 * N * N * cc.FS * float(rows[:, keep].min()) * len(chunks)
        lim2 = 100.0 * N * cc.FS * float(rows.sum())
        r = tuple((d / lim) if lim > 0 else (np.inf if d > 0 else 0.0) for lim in (lim1, lim2))
        if best is None or min(r) > min(best):
            best = r
    return best


@pytest.mark.parametrize("name", [c.name for c in cc.CASES if lin_form(c)])
def test_guard_distance(name):
    c = cc.BY_NAME[name]
    worst = [guard_ratios(c, cc.as_complex(c, buf)[cc.TARGET].astype(np.complex128)) for buf in cc.wire(name)]
    if c.placement == "e_rail":
        assert all(min(r) >= 100.0 for r in worst), worst       # marked: the subtract-first kernels analyse it
    elif c.placement == "e_zero":
        assert all(r == (0.0, 0.0) for r in worst), worst       # D = 0: nothing to mark
    else:
        assert all(r[0] <= 0.01 for r in worst), worst          # the first inequality alone is a factor 100 short


def test_both_sides_of_the_guard_have_a_witness():
    names = [c.name for c in cc.CASES if lin_form(c)]
    assert sum(cc.BY_NAME[n].placement == "e_rail" for n in names) >= 2
    assert sum(cc.BY_NAME[n].placement in ("a", "a_x", "b", "c") for n in names) >= 30


# ---- coverage, by brute force ------------------------------------------------------------------------------------------------------
def test_coverage():
    cases = cc.CASES
    fams = {(c.nperseg, c.window) for c in cases if c.fmt == "i16" and c.placement in ("a", "a_x", "b", "c")}
    want = {(n, "hamming") for n in (16, 32, 64, 128, 256, 300, 512, 1024, 2048, 4096, 8192)} | {(256, "boxcar"), (256, "hann"), (256, "blackman")}
    assert want <= fams, want - fams
    at256 = [c for c in cases if c.nperseg == 256 and c.window == "hamming" and c.precision == "float32"]
    pairs = {(c.fmt, "a" if c.placement == "a_x" else c.placement) for c in at256}
    for fmt in ("i16", "i8", "u8", "c64"):
        for pl in ("a", "b", "c", "d", "e_rail", "e_lone"):
            assert (fmt, pl) in pairs, (fmt, pl)
    assert ("i16", "e_zero") in pairs and {("c64full", "a"), ("c64full", "b")} <= pairs
    consts = {(c.fmt, tuple(np.ravel(c.const))) for c in cases}
    for fmt, v in (("i16", cc.RAIL16), ("i16", cc.NEG16), ("i16", cc.MID16), ("i8", cc.RAIL8), ("i8", cc.MID8), ("u8", cc.RAILU), ("u8", cc.ZEROU),
                   ("c64", cc.RAIL16)):
        assert (fmt, v) in consts, (fmt, v)
    assert {tuple(np.ravel(c.const)) for c in cases if c.fmt == "u8"} <= {cc.RAILU, cc.ZEROU}
    assert {c.mode for c in at256} >= {"sparse", "dense", "auto", "runfilter", "prefilter"}
    feats = set(itertools.chain.from_iterable(dict(c.extra) for c in at256))
    assert feats >= {"group_detect", "lanes", "in_flight", "record_cells", "row_means", "subtract_first"}, feats
    f64 = [c for c in cases if c.precision == "float64"]
    assert {(c.nperseg, bool(dict(c.extra).get("f64_sparse"))) for c in f64} >= {(256, False), (1024, False), (256, True), (1024, True)}
    assert {c.fmt for c in f64} == {"i16", "i8", "u8"}
    # the rescue: map-free with RT_FLAG_F64_RESCUE at both sizes, and the target stream -- it alone -- holds more cells at or over the
    # threshold than the case's hot_capacity in every buffer, so that it is the stream the fetch analyses again
    rescue = [c for c in f64 if dict(c.extra).get("f64_rescue")]
    assert {c.nperseg for c in rescue} == {256, 1024} and all(dict(c.extra).get("f64_sparse") for c in rescue)
    for c in rescue:
        cap = dict(c.extra)["hot_capacity"]
        thr = oracle.db_to_linear(cc.threshold_dbw(c))
        for row in cc.reference(c.name):
            hot = [int((r.spec >= thr).sum()) for r in row]
            assert hot[cc.TARGET] > cap and all(h < cap // 8 for s, h in enumerate(hot) if s != cc.TARGET), (c.name, hot)
        assert len(cc.nan_records(c.name)) >= 3
    assert all(3 <= cc.n_buffers(c) <= 6 and 24 <= c.T <= 40 for c in cases) and len(cases) <= 70
    # at least two NaN-std oracle records per placement kind, each with its own (fi, start, end)
    for kind in ("a", "b", "c"):
        n = sum(len(cc.nan_records(c.name)) for c in cases if c.placement == kind and c.fmt != "c64full")
        assert n >= 2, (kind, n)
    # the look-back placements put the constant segment at the end of buffers 0 and 2: calls 2 and 4 read it from the tail
    for c in cases:
        if c.placement in ("b", "c") and c.fmt != "c64full":
            assert {k for k, s, fi, a, b in cc.nan_records(c.name) if s == cc.TARGET and a == -1} == {1, 3}, c.name


def test_the_oracle_warns_and_nothing_else_is_hidden():
    """np.std over a plateau with a -inf cell raises RuntimeWarnings in the reference too; constant_cases.reference silences them,
    and only them: the NaN is there."""
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ref = cc.reference("i16_a")
    assert any(np.isnan(r.std_db) for r in ref[1][cc.TARGET].records)
