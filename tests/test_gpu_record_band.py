"""The bins beside each record's bin (rt_fetch_record_band) on the GPU.  Every column of every frame is held to the float64 model
(longdouble for float64 handles) at the column's bin, on the samples the same handle delivers through ``fetch_record_iq``, within
the bound of tests/record_stft_cases.py; the centre column to the bytes of ``fetch_record_stft(hop_div=k)``; a column d bins off to
the bytes of the centre column of the record d bins away (the twin case of tests/record_band_cases.py); the bytes to themselves
across handle kinds, fetches and orders of calls.

Worst |value - model| / bound per (nperseg, format, column) as seen on an MI355X (profiles/record_band_worst_ratio.txt holds the
table; ``RT_WRITE_PROFILES=1`` rewrites it): 0.04 - 0.33 per column on float32 handles, 0.17 - 0.50 on float64 ones with three columns
at 0.74 (complex128 at nperseg 256, d = -6 ... -4)."""
import ctypes as C
import datetime
import os

import numpy as np
import pytest

from pyradiotracking_amd import _native
from pyradiotracking_amd.analyze import BatchSignalAnalyzer, SignalAnalyzer, band_bins, record_band_spectrum, stft_constants, stft_constants_f64
from tests import record_band_cases as bc
from tests import record_iq_cases as riq
from tests import record_stft_cases as rs
from tests import record_stft_hop_cases as hop
from tests import sequence_cases as sq

pytestmark = pytest.mark.gpu

SCHED = rs.GPU_SCHEDULE
S = rs.GPU_S
N_CALLS = len(SCHED.T)
WORST = {}  # (nperseg, format, d) -> the worst ratio the model test saw
PROFILE = os.path.join(os.path.dirname(rs.PROFILE), "record_band_worst_ratio.txt")


@pytest.fixture(autouse=True)
def _need_gpu():
    if _native.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")


def _handle(nperseg, fmt, margin, n_streams=S, **extra):
    if fmt.endswith("f64") or fmt == "c128":
        extra["precision"] = "float64"
    kw = sq.case_settings(nperseg, fmt)
    kw.update(extra)
    if margin is not None:
        kw.update(record_iq=True, record_iq_margin=margin)
    return BatchSignalAnalyzer([str(i) for i in range(n_streams)], sdr_callback_length=sq.max_samples(SCHED, nperseg), **kw)


def _constants(window, nperseg, f64):
    if f64:
        return stft_constants_f64(window, nperseg, sq.FS)
    w, scale = stft_constants(window, nperseg, sq.FS)
    return w, float(scale)


def _run(nperseg, fmt, margin, after, feed=None, calls=N_CALLS, **extra):
    b = _handle(nperseg, fmt, margin, **extra)
    try:
        for c in range(calls):
            sq.enqueue(b, rs.gpu_feed(nperseg, c, fmt) if feed is None else feed(c), fmt)
            after(b, c, b.fetch_records())
    finally:
        b.close()


def _kind(values):
    return np.uint64 if values.dtype == np.complex128 else np.uint32


def _frames(b, fmt, nperseg, k):
    """(plan, frames [n, N] as the kernels convert them) of the call fetched last, from what ``fetch_record_iq`` delivers"""
    off_iq, first_iq, samples = b.fetch_record_iq()
    plan = hop.frame_plan(off_iq, first_iq, nperseg, k)
    x = rs.converted(samples, riq.base_format(fmt), b.precision == "float64")
    return plan, hop.frames_of(x, plan["sample"], nperseg)


def _band(b, k, w, n_rec):
    """``fetch_record_band`` held to ``fetch_record_stft(hop_div=k)``: the offsets, the first segments, the centre column"""
    off, first, values = b.fetch_record_band(k, w)
    off1, first1, centre = b.fetch_record_stft(hop_div=k)
    assert np.array_equal(off, off1) and np.array_equal(first, first1) and len(off) == n_rec + 1
    assert values.dtype == centre.dtype and values.shape == (len(centre), 2 * w + 1) and values.flags["C_CONTIGUOUS"]
    assert np.ascontiguousarray(values[:, w]).view(_kind(values)).tobytes() == centre.view(_kind(values)).tobytes()
    return off, first, values


# ---- 1 - 3: the offsets, the centre column, every column against the model ----------------------------------------------------------
@pytest.mark.parametrize("nperseg,fmt,k,w", [(N, f, k, w) for N, f in bc.GPU_SHAPES for k, w in bc.gpu_pairs(N)], ids=lambda v: str(v))
def test_every_column_of_every_frame_against_the_model_at_its_bin(nperseg, fmt, k, w):
    f64 = fmt == "c128"
    base = riq.base_format(fmt)
    win, scale = _constants(sq.WINDOW, nperseg, f64)
    seen = dict(frames=0, back=0, cells=0)
    worst = np.zeros(2 * w + 1)

    def after(b, c, rec):
        off, first, values = _band(b, k, w, len(rec))
        if w == 0:  # the whole output is the hop entry's
            assert values.view(_kind(values)).tobytes() == b.fetch_record_stft(hop_div=k)[2].view(_kind(values)).tobytes()
        plan, frames = _frames(b, fmt, nperseg, k)
        assert np.array_equal(off, plan["frame_first"]) and len(values) == len(plan["sample"])
        if not len(values):
            return
        bins = band_bins(rec["fi"], w, nperseg)[plan["record"]]
        # the model once per (stream, position, bin): the records a tone makes at neighbouring bins deliver the same samples, and
        # their bands overlap -- frames at one position of one stream are first held to be the same samples
        where = rec["stream"].astype(np.int64)[plan["record"]] * (1 << 40) + (plan["position"] + (1 << 30))
        _, first_at, same_as = np.unique(where, return_index=True, return_inverse=True)
        assert np.array_equal(frames.view(_kind(frames)), frames[first_at[same_as]].view(_kind(frames)))
        cell = (same_as[:, None] * nperseg + bins).reshape(-1)
        _, one, inv = np.unique(cell, return_index=True, return_inverse=True)
        q1 = rs.model_values(frames[one // (2 * w + 1)], bins.reshape(-1)[one], win, scale, nperseg, wide=f64)
        q = rs.Quantities(q1.values[inv], q1.norm[inv], q1.abs_m[inv], q1.absW[inv], q1.root)
        r = rs.ratios(values.reshape(-1), q, nperseg, rs.SPP[base], rs.U64 if f64 else rs.U32).reshape(values.shape)
        np.maximum(worst, r.max(axis=0), out=worst)
        assert r.max() <= 1.0, (c, int(r.argmax()) // (2 * w + 1), int(r.argmax()) % (2 * w + 1) - w, float(r.max()))
        seen["cells"] += len(one)
        seen["frames"] += len(values)
        seen["back"] += int((plan["lp"] > 0).sum())

    # (nperseg 4096: the model of a cell is 4096 sines and cosines; the first two calls hold both parts of a record)
    _run(nperseg, fmt, 0, after, calls=N_CALLS if nperseg < 4096 else 2)
    print(f"record_band nperseg {nperseg} {fmt} k {k} w {w}: {seen['frames']} frames, {seen['cells']} modelled cells, worst ratio per column " + " ".join(f"{v:.3f}" for v in worst))
    for j, v in enumerate(worst):
        WORST[(nperseg, fmt, j - w)] = max(WORST.get((nperseg, fmt, j - w), 0.0), float(v))
    assert seen["frames"] > 50 and seen["back"] > 0, seen  # records with a predecessor part occur


# ---- 4: twins ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nperseg,fmt", bc.TWIN_RUNS, ids=lambda v: str(v))
def test_a_column_is_the_centre_column_of_the_record_that_many_bins_away(nperseg, fmt):
    N = nperseg
    f64 = fmt == "c128"
    T, _, _ = bc.twin_layout(N)
    kw = dict(bc.twin_settings(N), record_iq=True, record_iq_margin=1)
    if f64:
        kw["precision"] = "float64"
    win, scale = _constants(bc.TWIN_WINDOW, N, f64)
    for fi in bc.twin_bins(N):
        b = BatchSignalAnalyzer([str(i) for i in range(S)], sdr_callback_length=T * N, **kw)
        try:
            sq.enqueue(b, bc.twin_feed(N, fi, fmt), fmt)
            rec = b.fetch_records()
            mine = np.flatnonzero(rec["stream"] == bc.TWIN_STREAM)
            spans = {(int(r["start"]), int(r["end"])) for r in rec[mine]}
            assert len(spans) == 1 and len(mine) >= 2 * bc.MAX_HALF, (N, fi, spans, len(mine))
            if fmt == "c64":
                assert sorted(sq.rec_key(rec[mine])) == sorted(bc.twin_oracle_records(N, fi))
            at = {int(rec["fi"][i]): i for i in mine}
            for k, w in ((4, 8), (1, 2), (2, 1)):
                off, first, values = _band(b, k, w, len(rec))
                assert len({int(first[i]) for i in mine}) == 1 and len({int(off[i + 1] - off[i]) for i in mine}) == 1
                seen, seen_centre = set(), set()
                for fa, ia in at.items():
                    for d in range(-w, w + 1):
                        ib = at.get((fa + d) % N)
                        if ib is None:
                            continue
                        one, other = values[off[ia]:off[ia + 1]], values[off[ib]:off[ib + 1]]
                        assert len(one) == len(other) > 0
                        assert np.ascontiguousarray(one[:, w + d]).view(_kind(values)).tobytes() == np.ascontiguousarray(other[:, w]).view(_kind(values)).tobytes(), \
                            (N, fmt, fi, k, w, fa, d)
                        seen.add(d)
                        if fa == fi:
                            seen_centre.add(d)
                assert seen == set(range(-w, w + 1)), (N, fi, k, w, seen)
                # around the tone's own bin every column has a twin but the one that lands on bin 0
                assert seen_centre == {d for d in range(-w, w + 1) if (fi + d) % N != 0}, (N, fi, k, w, seen_centre)
                # ... and that column, like every other, is held by the model
                plan, frames = _frames(b, fmt, N, k)
                i = at[fi]
                sl = slice(int(off[i]), int(off[i + 1]))
                for j in range(2 * w + 1):
                    q = rs.model_values(frames[sl], (fi + j - w) % N, win, scale, N, wide=f64)
                    r = rs.ratios(values[sl, j], q, N, rs.SPP[riq.base_format(fmt)], rs.U64 if f64 else rs.U32)
                    assert r.max() <= 1.0, (N, fmt, fi, k, w, j - w, float(r.max()))
        finally:
            b.close()


# ---- 5: a segment of one value -------------------------------------------------------------------------------------------------------
CONST_VALUE = np.complex64(complex(np.float32(0.3), np.float32(-0.7)))  # a full-mantissa constant


def _const_feed(nperseg, fmt):
    """the GPU suite's buffers with two segments of every stream made one value: call 1's last whole segment -- the records of call 2
    that start at its segment 0 deliver it as segment -1 -- and segment 7 of call 2, behind the pulses that end at segments 6 and 7"""
    def feed(c):
        x = rs.gpu_feed(nperseg, c, fmt).copy()
        if c == 1:
            x[:, (SCHED.T[1] - 1) * nperseg:SCHED.T[1] * nperseg] = CONST_VALUE
        if c == 2:
            x[:, 7 * nperseg:8 * nperseg] = CONST_VALUE
        return x
    return feed


def test_a_segment_of_one_value_is_exactly_zero_in_every_column_and_no_other_frame_is():
    nperseg, fmt, k, w = 256, "c64", 4, 8
    hit = [0, 0]

    def after(b, c, rec):
        off, first, values = _band(b, k, w, len(rec))
        plan, frames = _frames(b, fmt, nperseg, k)
        if not len(values):
            return
        constant = (frames == frames[:, :1]).all(axis=1)
        zero = (values.real == 0) & (values.imag == 0) & ~np.signbit(values.real) & ~np.signbit(values.imag)
        assert np.array_equal(zero.all(axis=1), constant) and np.array_equal(zero.any(axis=1), constant)
        for part in (0, 1):
            hit[part] += int((constant & (plan["part"] == part)).sum())

    _run(nperseg, fmt, 2, after, feed=_const_feed(nperseg, fmt))
    assert hit[0] >= 1 and hit[1] >= 1, hit


# ---- 6: a NaN sample -----------------------------------------------------------------------------------------------------------------
def test_a_nan_sample_makes_exactly_the_frames_that_cover_it_nan_in_every_column():
    nperseg, fmt, margin, k, w = 256, "c64", 2, 4, 2
    t_nan = SCHED.T[1] - 1  # call 1's last segment: the records of call 2 that start at its segment 0 deliver it as segment -1
    seen = dict(nan=0, clean=0, same=0)
    sides = {}
    for dirty in (False, True):
        got = []

        def feed(c, dirty=dirty):
            x = rs.gpu_feed(nperseg, c, fmt).copy()
            if dirty and c == 1:
                x[rs.NEG_STREAM, t_nan * nperseg + 5] = np.nan
            return x

        def after(b, c, rec, got=got):
            off, first, values = _band(b, k, w, len(rec))
            plan, frames = _frames(b, fmt, nperseg, k)
            holds = np.isnan(frames).any(axis=1)
            nan = np.isnan(values.real) & np.isnan(values.imag)
            assert np.array_equal(nan.all(axis=1), holds) and np.array_equal((np.isnan(values.real) | np.isnan(values.imag)).any(axis=1), holds)
            got.append({(int(r["stream"]), int(r["fi"]), int(r["start"]), int(r["end"]), int(first[i])): (values[off[i]:off[i + 1]], holds[off[i]:off[i + 1]])
                        for i, r in enumerate(rec)})

        _run(nperseg, fmt, margin, after, feed=feed)
        sides[dirty] = got
    for c in range(N_CALLS):
        for key, (v, holds) in sides[True][c].items():
            seen["nan"] += int(holds.sum())
            seen["clean"] += int((~holds).sum()) if holds.any() else 0
            if key in sides[False][c]:  # no other value of the call changes against the clean twin
                assert v[~holds].tobytes() == sides[False][c][key][0][~holds].tobytes(), (c, key)
                seen["same"] += 1
    assert seen["nan"] >= 2 and seen["clean"] >= 1 and seen["same"] > 20, seen


# ---- 7: handle kinds and orders of calls ---------------------------------------------------------------------------------------------
def _by_record(b, rec, k, w):
    off, first, values = b.fetch_record_band(k, w)
    again = b.fetch_record_band(k, w)
    assert values.tobytes() == again[2].tobytes() and np.array_equal(off, again[0])  # a second fetch of the same call copies
    return {(int(r["stream"]), int(r["fi"]), int(r["start"]), int(r["end"]), int(first[i])): values[off[i]:off[i + 1]].tobytes() for i, r in enumerate(rec)}


def _hold_common(runs, plain):
    for name in runs:
        if name == plain:
            continue
        common = 0
        for c in range(N_CALLS):
            for key, v in runs[plain][c].items():
                if key in runs[name][c]:
                    assert runs[name][c][key] == v, (name, c, key)
                    common += 1
        assert common >= 0.9 * sum(len(c) for c in runs[plain]) > 20, (name, common)


def test_the_same_samples_give_the_same_bytes_on_every_handle_kind():
    nperseg, margin, k, w = 256, 2, 4, 2
    runs = {}
    for name, extra in (("plain", dict(mode="sparse")), ("dense", dict(mode="dense")), ("lanes", dict(mode="sparse", lanes=2))):
        got = []
        _run(nperseg, "c64", margin, lambda b, c, rec, got=got: got.append(_by_record(b, rec, k, w)), **extra)
        runs[name] = got
    _hold_common(runs, "plain")
    runs = {}
    for name, extra in (("dense64", dict()), ("mapfree64", dict(f64_sparse=True))):
        got = []
        _run(nperseg, "c128", margin, lambda b, c, rec, got=got: got.append(_by_record(b, rec, k, w)), **extra)
        runs[name] = got
    _hold_common(runs, "dense64")


def test_a_chained_handle_gives_the_bytes_of_sequential_calls():
    """One recording of four buffers: through a ``chain=4`` handle in one call, and through a plain handle in four."""
    nperseg, margin, links, T, k, w = 256, 2, 4, 24, 4, 2
    half = T // 2 * nperseg
    bufs = []
    for c in range(links):
        x = rs.gpu_buffer(nperseg, c)[rs.NEG_STREAM][:SCHED.T[c] * nperseg]
        bufs.append(np.ascontiguousarray(np.concatenate([x[:half], x[len(x) - half:]])))
    kw = dict(sq.settings(nperseg), mode="sparse", record_iq=True, record_iq_margin=margin)
    seq = {}
    b = BatchSignalAnalyzer(["0"], sdr_callback_length=T * nperseg, **kw)
    try:
        for c, x in enumerate(bufs):
            b.enqueue(x[None, :])
            for key, v in _by_record(b, b.fetch_records(), k, w).items():
                seq[(c,) + key[1:]] = v
    finally:
        b.close()
    ch = BatchSignalAnalyzer(["0"], sdr_callback_length=T * nperseg, chain=links, **kw)
    try:
        ch.enqueue(np.concatenate(bufs)[None, :], links=links)
        chained = _by_record(ch, ch.fetch_records(), k, w)
    finally:
        ch.close()
    common = [key for key in chained if key in seq]
    assert len(common) >= 0.9 * len(seq) > 8 and any(key[4] < 0 for key in common), (len(common), len(seq))
    for key in common:
        assert chained[key] == seq[key], key


def test_the_order_of_calls_does_not_change_the_bytes():
    nperseg, fmt, margin = 256, "c64", 2
    first_run, n = [], [0]

    def early(b, c, rec):  # the band in front of every other record entry
        first_run.append(b.fetch_record_band(4, 2)[2].tobytes())

    def late(b, c, rec):  # ... and behind them, twice, and after another pair and back
        b.fetch_record_stft()
        b.fetch_record_stft(hop_div=4)
        b.fetch_record_estimates(hop_div=4)
        a = b.fetch_record_band(4, 2)[2]
        assert a.tobytes() == first_run[c] == b.fetch_record_band(4, 2)[2].tobytes()
        wide = b.fetch_record_band(4, 8)[2]
        other = b.fetch_record_band(2, 1)[2]
        assert b.fetch_record_band(4, 2)[2].tobytes() == first_run[c]
        # the columns the pairs share are the same bytes
        assert np.ascontiguousarray(wide[:, 6:11]).tobytes() == a.tobytes()
        plan4 = hop.frame_plan(b.fetch_record_iq()[0], b.fetch_record_iq()[1], nperseg, 4)
        both = plan4["sample"] % (nperseg // 2) == 0
        assert both.sum() == len(other) and np.ascontiguousarray(a[both][:, 1:4]).tobytes() == other.tobytes()
        n[0] += len(a)

    _run(nperseg, fmt, margin, early)
    _run(nperseg, fmt, margin, late)
    assert n[0] > 100


# ---- 8: refusals, the size query ---------------------------------------------------------------------------------------------------
def _fetch_band(b, k, w, n_rec, cap=None, f64=None, n_off=None):
    lib, h = b.native._lib, b.native._handle
    f64 = (b.precision == "float64") if f64 is None else f64
    fn = lib.rt_fetch_record_band_f64 if f64 else lib.rt_fetch_record_band
    off = np.zeros((n_rec if n_off is None else n_off) + 1, np.int64)
    first = np.zeros(n_rec, np.int32)
    n = C.c_size_t(0)
    rc = fn(h, k, w, off.ctypes.data, off.size, first.ctypes.data, first.size, None, 0, C.byref(n))
    if rc != _native.RT_OK or cap is None:
        return rc, n.value, None
    buf = np.full(2 * max(cap, 1) * (2 * w + 1), 7.5, np.float64 if f64 else np.float32)
    rc = fn(h, k, w, off.ctypes.data, off.size, first.ctypes.data, first.size, buf.ctypes.data, cap, C.byref(n))
    return rc, n.value, buf


def _err(b):
    return b.native._lib.rt_last_error(b.native._handle).decode()


def test_refusals_and_the_size_query():
    nperseg, fmt, k, w = 256, "c64", 4, 2
    B = 2 * w + 1
    name = "rt_fetch_record_band"
    feeds = [rs.gpu_feed(nperseg, c, fmt) for c in range(N_CALLS)]
    off_handle = _handle(nperseg, fmt, None)
    b = _handle(nperseg, fmt, 0)
    twin = _handle(nperseg, fmt, 0)
    d64 = _handle(nperseg, "c128", 0)
    small = BatchSignalAnalyzer(["0"], sdr_callback_length=40 * 16, record_iq=True, **sq.settings(16))
    lib = b.native._lib

    def both(x):
        b.enqueue(x)
        twin.enqueue(x)

    def same():
        rec, want = b.fetch_records(), twin.fetch_records()
        assert rec.tobytes() == want.tobytes()  # after every refusal the handle analyses on as its twin does
        return rec

    def good(n_rec):
        """the next valid call returns the bytes it would have returned: the twin's, which was never refused"""
        got, want = b.fetch_record_band(k, w), twin.fetch_record_band(k, w)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, want)) and len(got[0]) == n_rec + 1

    try:
        # feature off
        off_handle.enqueue(feeds[0])
        off_handle.fetch_records()
        with pytest.raises(_native.NativeError) as ei:
            off_handle.fetch_record_band(k, w)
        assert ei.value.code == _native.RT_E_INVALID and name + ": rt_set_record_iq" in str(ei.value)
        # no delivered call yet
        assert _fetch_band(b, k, w, 0)[0] == _native.RT_E_INVALID and _err(b).startswith(name + ": no samples")
        both(feeds[0])
        same()
        both(feeds[1])
        rec = same()
        n_rec = len(rec)
        assert n_rec > 0
        # a null n_frames; the wrong twin, both ways
        h = b.native._handle
        assert lib.rt_fetch_record_band(h, k, w, None, 0, None, 0, None, 0, None) == _native.RT_E_INVALID
        good(n_rec)
        assert _fetch_band(b, k, w, n_rec, f64=True)[0] == _native.RT_E_INVALID and "float32 handle" in _err(b) and name + "_f64" in _err(b)
        good(n_rec)
        d64.enqueue(feeds[1].astype(np.complex128))
        n64 = len(d64.fetch_records())
        assert _fetch_band(d64, k, w, n64, f64=False)[0] == _native.RT_E_INVALID and "float64 handle" in _err(d64)
        assert _fetch_band(d64, k, w, n64)[0] == _native.RT_OK
        # k no divisor of nperseg in 1 .. 16, w outside 0 .. 8: refused, the message names k, w and N, nothing written
        for bad_k, bad_w in ((0, 2), (17, 2), (3, 2), (-4, 2), (4, -1), (4, 9), (1, 100)):
            rc, _, _ = _fetch_band(b, bad_k, bad_w, n_rec)
            e = _err(b)
            assert rc == _native.RT_E_INVALID and f"k = {bad_k}" in e and f"w = {bad_w}" in e and f"N = {nperseg}" in e and e.startswith(name + ":"), e
            with pytest.raises(_native.NativeError):
                b.fetch_record_band(bad_k, bad_w)
            good(n_rec)
        assert _fetch_band(d64, 3, 2, n64)[0] == _native.RT_E_INVALID and _err(d64).startswith(name + "_f64:")
        # 2 w + 1 > nperseg
        small.enqueue(np.zeros((1, 40 * 16), np.complex64))
        assert len(small.fetch_records()) == 0
        assert _fetch_band(small, 1, 8, 0)[0] == _native.RT_E_INVALID and "w = 8" in _err(small) and "N = 16" in _err(small)
        assert _fetch_band(small, 1, 7, 0)[:2] == (_native.RT_OK, 0)
        # size query, then fetch; cap one short; wrong counts
        rc, n_frames, _ = _fetch_band(b, k, w, n_rec)
        assert rc == _native.RT_OK and n_frames > 0
        rc, _, buf = _fetch_band(b, k, w, n_rec, n_frames - 1)
        assert rc == _native.RT_E_CAPACITY and np.all(buf == 7.5)
        good(n_rec)
        assert _fetch_band(b, k, w, n_rec + 1)[0] == _native.RT_E_INVALID and _fetch_band(b, k, w, n_rec, n_off=n_rec + 1)[0] == _native.RT_E_INVALID
        good(n_rec)
        rc, n2, buf = _fetch_band(b, k, w, n_rec, n_frames + 3)
        assert rc == _native.RT_OK and n2 == n_frames
        assert buf[:2 * n_frames * B].view(np.complex64).tobytes() == b.fetch_record_band(k, w)[2].tobytes() and np.all(buf[2 * n_frames * B:] == 7.5)
        # after the next enqueue; with two in flight: process c, process c + 1, fetch c, then the values of c
        both(feeds[2])
        assert _fetch_band(b, k, w, n_rec)[0] == _native.RT_E_INVALID
        both(feeds[3])
        rec = same()
        assert _fetch_band(b, k, w, len(rec))[0] == _native.RT_OK
        good(len(rec))
        # a truncated delivery
        n = C.c_size_t(0)
        out = np.zeros(2, _native.RECORD_DTYPE)
        lib.rt_fetch(h, out.ctypes.data, 2, C.byref(n))
        assert n.value > 2
        assert _fetch_band(b, k, w, 2)[0] == _native.RT_E_INVALID and _err(b) == name + ": the call fetched last was delivered truncated"
        twin.fetch_records()
        # a call without records
        both(np.zeros((S, 4 * nperseg), np.complex64))
        assert len(same()) == 0
        rc, n_frames, _ = _fetch_band(b, k, w, 0)
        assert rc == _native.RT_OK and n_frames == 0
        assert b.fetch_record_band(k, w)[2].shape == (0, B)
        # the feature turned off again
        b.native.set_record_iq(-1)
        twin.native.set_record_iq(-1)
        both(feeds[0])
        same()
        assert _fetch_band(b, k, w, 0)[0] == _native.RT_E_INVALID and "rt_set_record_iq" in _err(b)
        for c in (1, 2):
            both(feeds[c])
            same()
    finally:
        for x in (b, twin, d64, off_handle, small):
            x.close()


# ---- 9: the entry changes nothing else -------------------------------------------------------------------------------------------
def test_the_entry_changes_nothing_else():
    """With the entry never called and with it called after every fetch, in front of and between everything else: the records, the
    record IQ, the segments' STFT values, the hop values and the estimate rows are the same bytes."""
    nperseg, fmt, margin = 256, "c64", 2
    sides = {}
    for use in (False, True):
        got = []

        def after(b, c, rec, use=use, got=got):
            row = [rec.tobytes()]
            for fetch in (b.fetch_record_iq, b.fetch_record_stft, lambda: b.fetch_record_stft(hop_div=4), lambda: (b.fetch_record_estimates(hop_div=4),)):
                if use:
                    b.fetch_record_band(4, 2)
                    b.fetch_record_band(2, 8)
                row += [np.asarray(a).tobytes() for a in fetch()]
            got.append(row)

        _run(nperseg, fmt, margin, after)
        sides[use] = got
    assert sides[False] == sides[True] and len(sides[True]) == N_CALLS


# ---- 10: the Python layers ---------------------------------------------------------------------------------------------------------
def test_signal_analyzer_and_replay_leave_the_band_beside_the_values():
    nperseg, margin, k, w = 256, 2, 4, 2
    sched = sq.SCHEDULES["B"]
    n_buf = 5
    B = sched.T[0] * nperseg
    x = np.concatenate([sq.buffer(sched, nperseg, c, 1)[0] for c in range(n_buf)])
    kw = sq.settings(nperseg)
    with pytest.raises(ValueError):
        SignalAnalyzer("0", sdr_callback_length=B, record_band=w, **kw)
    a = SignalAnalyzer("0", sdr_callback_length=B, record_iq=True, record_iq_margin=margin, record_band=w, stft_hop_div=k, **kw)
    plain = BatchSignalAnalyzer(["0"], sdr_callback_length=B, record_iq=True, record_iq_margin=margin, **kw)
    ts0 = datetime.datetime(2024, 1, 1)
    bands = []
    try:
        for c in range(n_buf):
            buf = x[c * B:(c + 1) * B]
            got = a.analyze_buffer(buf, ts0 + datetime.timedelta(seconds=c * B / sq.FS))
            assert len(a.signal_band) == len(a.signal_stft) == len(got)
            # the arrays fetch_record_band gives for the same buffers
            plain.enqueue(buf[None, :])
            rec = plain.fetch_records()
            off, first, values = plain.fetch_record_band(k, w)
            want = [values[off[i]:off[i + 1]] for i in np.flatnonzero(rec["shadowed"] == 0)]
            assert len(want) == len(a.signal_band)
            for band, centre, ref in zip(a.signal_band, a.signal_stft, want):
                assert band.shape == (len(centre), 2 * w + 1) and band.tobytes() == ref.tobytes()
                assert np.ascontiguousarray(band[:, w]).tobytes() == centre.tobytes()
            spec = record_band_spectrum(off, first, values, rec["start"], rec["end"], nperseg, k)
            assert spec.shape == (len(rec), 2 * w + 1) and (np.nanargmax(spec[rec["shadowed"] == 0], axis=1) == w).all()  # bin-centred tones
            bands.extend(a.signal_band)
        with pytest.raises(ValueError):
            a.replay(x, ts0, chain=2, record_band=w)
        out, out_iq, out_band = a.replay(x, ts0, chain=2, record_iq=True, stft_hop_div=k, record_band=w)
        out5 = a.replay(x, ts0, chain=2, record_iq=True, record_stft=True, stft_hop_div=k, record_estimates=True, record_band=w)
    finally:
        plain.close()
        a._batch.close()
        if a._replay_batch is not None:
            a._replay_batch.close()
    assert len(out) == len(out_iq) == len(out_band) == len(bands) > 3 and len(out5) == 5 and len(out5[4]) == len(out)
    for got, want in zip(out_band, bands):
        assert got.tobytes() == want.tobytes()
    for got, centre in zip(out5[4], out5[2]):
        assert np.ascontiguousarray(got[:, w]).tobytes() == centre.tobytes()


def test_zz_write_the_worst_ratios():
    """(last in the file: the table of what the model test above saw on this GPU)"""
    assert WORST
    lines = ["rt_fetch_record_band on the GPU: worst |value - model| / bound per (nperseg, format, column d = j - w) over the (k, w) of",
             "tests/record_band_cases.py: GPU_PAIRS, every frame of the four calls of tests/record_stft_cases.py: GPU_SCHEDULE (nperseg 4096: of the first two), margin 0.", "",
             f"{'nperseg':>8} {'format':>7} " + " ".join(f"{d:>6}" for d in range(-bc.MAX_HALF, bc.MAX_HALF + 1))]
    for N, fmt in bc.GPU_SHAPES:
        lines.append(f"{N:>8} {fmt:>7} " + " ".join(f"{WORST[(N, fmt, d)]:6.3f}" if (N, fmt, d) in WORST else f"{'-':>6}" for d in range(-bc.MAX_HALF, bc.MAX_HALF + 1)))
    lines.append(f"worst of all: {max(WORST.values()):.3f}")
    text = "\n".join(lines) + "\n"
    print(text)
    if os.environ.get("RT_WRITE_PROFILES"):
        with open(PROFILE, "w") as f:
            f.write(text)
