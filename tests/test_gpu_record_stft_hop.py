"""Record STFT at a sub-segment hop (rt_fetch_record_stft_hop) on the GPU.  Every frame is held to the float64 model (longdouble for
float64 handles) of the samples the same handle delivers through ``fetch_record_iq``, within the bound of
tests/record_stft_cases.py -- a frame is a segment that starts elsewhere, the summation depth is the same; the frames on the segment
grid to the bytes of ``fetch_record_stft()``; the bytes to themselves across handle kinds, fetches and orders of calls.

Worst |value - model| / bound seen on an MI355X (profiles/record_stft_hop_worst_ratio.txt holds the table): 0.14 - 0.32 per case, one
value at 0.49 (complex64 at nperseg 300, margin 2, as for the segments' values)."""
import ctypes as C

import numpy as np
import pytest

from pyradiotracking_amd import _native
from pyradiotracking_amd.analyze import BatchSignalAnalyzer, record_edges, record_fine, stft_constants, stft_constants_f64, stft_frame_positions
from tests import constant_cases as cst
from tests import record_iq_cases as riq
from tests import record_stft_cases as rs
from tests import record_stft_hop_cases as hop
from tests import sequence_cases as sq

pytestmark = pytest.mark.gpu

SCHED = rs.GPU_SCHEDULE
S = rs.GPU_S
N_CALLS = len(SCHED.T)


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


def _constants(nperseg, f64):
    if f64:
        return stft_constants_f64(sq.WINDOW, nperseg, sq.FS)
    w, scale = stft_constants(sq.WINDOW, nperseg, sq.FS)
    return w, float(scale)


def _frames(b, rec, fmt, nperseg, k):
    """(plan, offsets, first, values, frames [n, N] as the kernels convert them) of the call fetched last; the counts and the
    offsets are held to the plan of what ``fetch_record_iq`` delivers"""
    f64 = b.precision == "float64"
    off_iq, first_iq, samples = b.fetch_record_iq()
    off, first, values = b.fetch_record_stft(hop_div=k)
    plan = hop.frame_plan(off_iq, first_iq, nperseg, k)
    assert np.array_equal(off, plan["frame_first"]) and np.array_equal(first, first_iq) and len(off) == len(rec) + 1
    assert values.dtype == (np.complex128 if f64 else np.complex64) and len(values) == off[-1] == len(plan["sample"])
    assert np.array_equal(stft_frame_positions(off, first, nperseg, k), plan["position"])
    x = rs.converted(samples, riq.base_format(fmt), f64)
    return plan, off, first, values, hop.frames_of(x, plan["sample"], nperseg)


def _model(b, rec, fmt, nperseg, k):
    f64 = b.precision == "float64"
    plan, off, first, values, frames = _frames(b, rec, fmt, nperseg, k)
    if not len(values):
        return plan, off, first, values, None, np.zeros(0)
    w, scale = _constants(nperseg, f64)
    q = rs.model_values(frames, rec["fi"].astype(np.int64)[plan["record"]], w, scale, nperseg, wide=f64)
    return plan, off, first, values, q, rs.ratios(values, q, nperseg, rs.SPP[riq.base_format(fmt)], rs.U64 if f64 else rs.U32)


def _run(nperseg, fmt, margin, after, **extra):
    b = _handle(nperseg, fmt, margin, **extra)
    try:
        for k in range(N_CALLS):
            sq.enqueue(b, rs.gpu_feed(nperseg, k, fmt), fmt)
            after(b, k, b.fetch_records())
    finally:
        b.close()


# (nperseg, format, k): the smallest shapes at which each path can go wrong
MODEL_CASES = [(256, "c64", 4),        # the baseline
               (32, "c64", 16),        # 16 pieces, groups of 16 lanes, a hop of 2 samples
               (1024, "c64", 2),
               (4096, "c64", 8),       # frames longer than the registers hold: the re-read path
               (300, "c64", 4),        # frames at byte offsets 600 j: 8-byte loads
               (300, "u8", 4),         # ... 150 j: 2-byte loads
               (256, "u8", 4),         # 32 pieces, groups of 32 lanes
               (256, "u8", 16),        # ... at byte offsets 32 j
               (32, "u8", 2),          # 4 pieces, groups of 8 lanes
               (256, "i8", 4),
               (256, "i16", 4),        # 64 pieces: a whole wave
               (9, "c64", 3),          # frames of 72 bytes at 24-byte hops
               (9, "i16", 3),          # frames of 36 bytes at 12-byte hops
               (9, "u8", 3),           # frames of 18 bytes at 6-byte hops
               (256, "c128", 4), (256, "u8f64", 4), (256, "c128-sparse", 4)]


@pytest.mark.parametrize("margin", [0, 2])
@pytest.mark.parametrize("nperseg,fmt,k", MODEL_CASES, ids=lambda v: str(v))
def test_every_frame_against_the_model_and_the_grid_frames_against_the_segments(nperseg, fmt, k, margin):
    extra = {}
    if fmt.endswith("-sparse"):
        fmt, extra = fmt[:-7], dict(f64_sparse=True)
    seen = dict(frames=0, back=0, worst=0.0, grid=0)

    def after(b, c, rec):
        plan, off, first, values, q, r = _model(b, rec, fmt, nperseg, k)
        if len(r):
            print(f"record_stft_hop nperseg {nperseg} {fmt} k {k} margin {margin} call {c}: {len(r)} frames, worst ratio {r.max():.3f}")
            seen["worst"] = max(seen["worst"], float(r.max()))
            assert r.max() <= 1.0, (c, int(r.argmax()), float(r.max()))
        # the frames on the segment grid are the bytes of fetch_record_stft(), and hop_div = 1 is that entry whole
        off1, first1, seg_values = b.fetch_record_stft()
        grid = plan["sample"] % nperseg == 0
        assert grid.sum() == len(seg_values) == off1[-1]
        kind = np.uint64 if values.dtype == np.complex128 else np.uint32
        assert np.array_equal(values[grid].view(kind), seg_values[plan["sample"][grid] // nperseg].view(kind))
        # (the Python method routes hop_div = 1 to today's entry: ask the new one itself)
        rc, n1, buf = _fetch_hop(b, 1, len(rec), cap=len(seg_values))
        assert rc == _native.RT_OK and n1 == len(seg_values) and buf[:2 * n1].view(kind).tobytes() == seg_values.view(kind).tobytes()
        seen["frames"] += len(values)
        seen["grid"] += int(grid.sum())
        seen["back"] += int((plan["lp"] > 0).sum())

    _run(nperseg, fmt, margin, after, **extra)
    assert seen["frames"] > seen["grid"] > 0, seen
    if nperseg >= 32:
        assert seen["frames"] > 100 and seen["back"] > 0, seen  # records with a predecessor part occur


def _values_by_record(b, rec, k):
    off, first, values = b.fetch_record_stft(hop_div=k)
    again = b.fetch_record_stft(hop_div=k)
    assert values.tobytes() == again[2].tobytes() and np.array_equal(off, again[0])  # a second fetch of the same call
    return {(int(r["stream"]), int(r["fi"]), int(r["start"]), int(r["end"]), int(first[i])): values[off[i]:off[i + 1]].tobytes()
            for i, r in enumerate(rec)}


def test_the_same_samples_give_the_same_bytes_on_every_handle_kind():
    nperseg, fmt, margin, k = 256, "c64", 2, 4
    runs = {}
    for name, extra in (("plain", dict(mode="sparse")), ("dense", dict(mode="dense")), ("lanes", dict(mode="sparse", lanes=3))):
        got = []
        _run(nperseg, fmt, margin, lambda b, c, rec: got.append(_values_by_record(b, rec, k)), **extra)
        runs[name] = got
    for name in ("dense", "lanes"):
        common = 0
        for c in range(N_CALLS):
            for key, v in runs["plain"][c].items():
                if key in runs[name][c]:
                    assert runs[name][c][key] == v, (name, c, key)
                    common += 1
        assert common >= 0.9 * sum(len(c) for c in runs["plain"]) > 20, (name, common)


def test_a_chained_handle_gives_the_bytes_of_sequential_calls():
    """One recording of four buffers: through a ``chain=4`` handle in one call, and through a plain handle in four."""
    nperseg, margin, links, T, k = 256, 2, 4, 24, 4
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
            for key, v in _values_by_record(b, b.fetch_records(), k).items():
                seq[(c,) + key[1:]] = v
    finally:
        b.close()
    ch = BatchSignalAnalyzer(["0"], sdr_callback_length=T * nperseg, chain=links, **kw)
    try:
        ch.enqueue(np.concatenate(bufs)[None, :], links=links)
        chained = _values_by_record(ch, ch.fetch_records(), k)
    finally:
        ch.close()
    common = [key for key in chained if key in seq]
    assert len(common) >= 0.9 * len(seq) > 8 and any(key[4] < 0 for key in common), (len(common), len(seq))
    for key in common:
        assert chained[key] == seq[key], key


def test_frames_inside_a_constant_run_are_exactly_zero_and_no_other():
    """tests/constant_cases.py, int16 rails at nperseg 256: the frames of the target stream's records whose samples are all one
    value are exactly 0 + 0j; every frame that covers a sample outside the run is not."""
    c = cst.BY_NAME["fam256box"]
    assert c.fmt == "i16" and c.nperseg == 256 and c.const == cst.RAIL16
    lengths, consts, _, want = cst.layout(c)
    (k_const, t_const), = consts
    b = BatchSignalAnalyzer([str(i) for i in range(cst.S)], sdr_callback_length=max(lengths), mode=c.mode, segs_per_chunk=c.spc, record_iq=True,
                            record_iq_margin=1, **cst.settings(c))
    hit = part = 0
    try:
        for k, buf in enumerate(cst.wire(c.name)):
            b.enqueue_int16(np.array(buf))
            rec = b.fetch_records()
            plan, off, first, values, frames = _frames(b, rec, "i16", c.nperseg, 4)
            if k != k_const or not len(values):
                continue
            constant = (frames == frames[:, :1]).all(axis=1)
            zero = (values.real == 0) & (values.imag == 0)
            assert np.array_equal(zero, constant)
            hit += int(constant.sum())
            # frames that hold some of the run and a sample outside it
            pos, N = plan["position"], c.nperseg
            part += int(((pos + N > t_const * N) & (pos < (t_const + 1) * N) & ~constant & (rec["stream"][plan["record"]] == cst.TARGET)).sum())
    finally:
        b.close()
    assert hit >= 1 and part >= 1, (hit, part)


def test_a_nan_sample_makes_exactly_the_frames_that_cover_it_nan():
    nperseg, fmt, margin, k = 256, "c64", 2, 4
    t_nan = SCHED.T[1] - 1  # call 1's last segment: the records of call 2 that start at its segment 0 deliver it as segment -1
    seen = dict(nan=0, clean=0, same=0)
    sides = {}
    for dirty in (False, True):
        got = []

        def after(b, c, rec, got=got):
            plan, off, first, values, frames = _frames(b, rec, fmt, nperseg, k)
            holds = np.isnan(frames).any(axis=1)
            assert np.array_equal(np.isnan(values.real) & np.isnan(values.imag), holds) and np.array_equal(np.isnan(values.real) | np.isnan(values.imag), holds)
            got.append({(int(r["stream"]), int(r["fi"]), int(r["start"]), int(r["end"]), int(first[i])): (values[off[i]:off[i + 1]], holds[off[i]:off[i + 1]])
                        for i, r in enumerate(rec)})

        b = _handle(nperseg, fmt, margin)
        try:
            for c in range(N_CALLS):
                x = rs.gpu_feed(nperseg, c, fmt).copy()
                if dirty and c == 1:
                    x[rs.NEG_STREAM, t_nan * nperseg + 5] = np.nan
                b.enqueue(x)
                after(b, c, b.fetch_records())
        finally:
            b.close()
        sides[dirty] = got
    for c in range(N_CALLS):
        for key, (v, holds) in sides[True][c].items():
            seen["nan"] += int(holds.sum())
            seen["clean"] += int((~holds).sum()) if holds.any() else 0
            if key in sides[False][c]:  # no other value of the call changes against the clean twin
                assert v[~holds].tobytes() == sides[False][c][key][0][~holds].tobytes(), (c, key)
                seen["same"] += 1
    assert seen["nan"] >= 2 and seen["clean"] >= 1 and seen["same"] > 20, seen


# ---- order of calls, refusals, queries, side effects -------------------------------------------------------------------------------
def _fetch_hop(b, k, n_rec, cap=None, f64=None, n_off=None):
    lib, h = b.native._lib, b.native._handle
    f64 = (b.precision == "float64") if f64 is None else f64
    fn = lib.rt_fetch_record_stft_hop_f64 if f64 else lib.rt_fetch_record_stft_hop
    off = np.zeros((n_rec if n_off is None else n_off) + 1, np.int64)
    first = np.zeros(n_rec, np.int32)
    n = C.c_size_t(0)
    rc = fn(h, k, off.ctypes.data, off.size, first.ctypes.data, first.size, None, 0, C.byref(n))
    if rc != _native.RT_OK or cap is None:
        return rc, n.value, None
    buf = np.full(2 * max(cap, 1), 7.5, np.float64 if f64 else np.float32)
    rc = fn(h, k, off.ctypes.data, off.size, first.ctypes.data, first.size, buf.ctypes.data, cap, C.byref(n))
    return rc, n.value, buf


def _err(b):
    return b.native._lib.rt_last_error(b.native._handle).decode()


def test_the_order_of_calls_does_not_change_the_bytes():
    nperseg, fmt, margin = 256, "c64", 2
    n = [0]

    def after(b, c, rec):
        a4 = b.fetch_record_stft(hop_div=4)
        seg = b.fetch_record_stft()
        a2 = b.fetch_record_stft(hop_div=2)
        b4 = b.fetch_record_stft(hop_div=4)
        assert a4[2].tobytes() == b4[2].tobytes() and np.array_equal(a4[0], b4[0])
        assert seg[2].tobytes() == b.fetch_record_stft()[2].tobytes()
        plan2, plan4 = hop.frame_plan(seg[0] * nperseg, seg[1], nperseg, 2), hop.frame_plan(seg[0] * nperseg, seg[1], nperseg, 4)
        # the frames k = 2 and k = 4 share
        both4 = plan4["sample"] % (nperseg // 2) == 0
        assert both4.sum() == len(a2[2]) and a2[2].tobytes() == a4[2][both4].tobytes()
        assert np.array_equal(a2[0], plan2["frame_first"])
        n[0] += len(a4[2])

    _run(nperseg, fmt, margin, after)
    assert n[0] > 100


def test_refusals_and_the_size_query():
    nperseg, fmt, k = 256, "c64", 4
    name = "rt_fetch_record_stft_hop"
    feeds = [rs.gpu_feed(nperseg, c, fmt) for c in range(N_CALLS)]
    off_handle = _handle(nperseg, fmt, None)
    b = _handle(nperseg, fmt, 0)
    twin = _handle(nperseg, fmt, 0)
    d64 = _handle(nperseg, "c128", 0)
    lib = b.native._lib

    def both(x):
        b.enqueue(x)
        twin.enqueue(x)

    def same():
        rec, want = b.fetch_records(), twin.fetch_records()
        assert rec.tobytes() == want.tobytes()  # after every refusal the handle analyses on as its twin does
        return rec

    try:
        # feature off
        off_handle.enqueue(feeds[0])
        off_handle.fetch_records()
        with pytest.raises(_native.NativeError) as ei:
            off_handle.fetch_record_stft(hop_div=k)
        assert ei.value.code == _native.RT_E_INVALID and name + ": rt_set_record_iq" in str(ei.value)
        # no delivered call yet
        assert _fetch_hop(b, k, 0)[0] == _native.RT_E_INVALID and _err(b).startswith(name + ": no samples")
        both(feeds[0])
        same()
        both(feeds[1])
        rec = same()
        n_rec = len(rec)
        assert n_rec > 0
        # a null n_frames; the wrong twin, both ways
        h = b.native._handle
        assert lib.rt_fetch_record_stft_hop(h, k, None, 0, None, 0, None, 0, None) == _native.RT_E_INVALID
        assert _fetch_hop(b, k, n_rec, f64=True)[0] == _native.RT_E_INVALID and "float32 handle" in _err(b) and name + "_f64" in _err(b)
        d64.enqueue(feeds[1].astype(np.complex128))
        n64 = len(d64.fetch_records())
        assert _fetch_hop(d64, k, n64, f64=False)[0] == _native.RT_E_INVALID and "float64 handle" in _err(d64)
        assert _fetch_hop(d64, k, n64)[0] == _native.RT_OK
        # a hop that is no divisor of nperseg in 1 .. 16: refused, the message names k and N, nothing written
        for bad in (0, 17, 3, -4):
            rc, _, _ = _fetch_hop(b, bad, n_rec)
            assert rc == _native.RT_E_INVALID and f"k = {bad}" in _err(b) and f"N = {nperseg}" in _err(b) and _err(b).startswith(name + ":"), _err(b)
            with pytest.raises(_native.NativeError):
                b.fetch_record_stft(hop_div=bad)
        assert _fetch_hop(d64, 3, n64)[0] == _native.RT_E_INVALID and _err(d64).startswith(name + "_f64:")
        # size query, then fetch; cap one short; wrong counts
        rc, n_frames, _ = _fetch_hop(b, k, n_rec)
        assert rc == _native.RT_OK and n_frames > 0
        rc, _, buf = _fetch_hop(b, k, n_rec, n_frames - 1)
        assert rc == _native.RT_E_CAPACITY and np.all(buf == 7.5)
        assert _fetch_hop(b, k, n_rec + 1)[0] == _native.RT_E_INVALID and _fetch_hop(b, k, n_rec, n_off=n_rec + 1)[0] == _native.RT_E_INVALID
        rc, n2, buf = _fetch_hop(b, k, n_rec, n_frames)
        assert rc == _native.RT_OK and n2 == n_frames
        assert buf[:2 * n_frames].view(np.complex64).tobytes() == b.fetch_record_stft(hop_div=k)[2].tobytes() and np.all(buf[2 * n_frames:] == 7.5)
        # after the next enqueue; with two in flight: process c, process c + 1, fetch c, then the values of c
        both(feeds[2])
        assert _fetch_hop(b, k, n_rec)[0] == _native.RT_E_INVALID
        both(feeds[3])
        rec = same()
        assert _fetch_hop(b, k, len(rec))[0] == _native.RT_OK
        # a truncated delivery
        n = C.c_size_t(0)
        out = np.zeros(2, _native.RECORD_DTYPE)
        lib.rt_fetch(h, out.ctypes.data, 2, C.byref(n))
        assert n.value > 2
        assert _fetch_hop(b, k, 2)[0] == _native.RT_E_INVALID and _err(b) == name + ": the call fetched last was delivered truncated"
        twin.fetch_records()
        # after rt_extract (on both handles: it moves the look-back)
        spec = np.zeros((S, 4, nperseg), np.float32)
        d = _native.DeviceBuffer(0, spec.nbytes)
        d.upload(spec)
        for x in (b, twin):
            x.native.extract_device(d.ptr, 4, nperseg, None, 0)
            x.fetch_records()
        assert _fetch_hop(b, k, 0)[0] == _native.RT_E_INVALID and "rt_extract" in _err(b)
        d.free()
        # a call without records
        both(np.zeros((S, 4 * nperseg), np.complex64))
        assert len(same()) == 0
        rc, n_frames, _ = _fetch_hop(b, k, 0)
        assert rc == _native.RT_OK and n_frames == 0
        # the feature turned off again
        b.native.set_record_iq(-1)
        twin.native.set_record_iq(-1)
        both(feeds[0])
        same()
        assert _fetch_hop(b, k, 0)[0] == _native.RT_E_INVALID and "rt_set_record_iq" in _err(b)
        for c in (1, 2):
            both(feeds[c])
            same()
    finally:
        for x in (b, twin, d64, off_handle):
            x.close()


def test_the_entry_changes_nothing_else():
    """With the entry never called and with it called after every fetch, in front of everything else: the records, row means,
    record cells, record IQ and the segments' STFT values are the same bytes."""
    nperseg, fmt, margin = 256, "c64", 2
    sides = {}
    for use in (False, True):
        got = []

        def after(b, c, rec, use=use, got=got):
            if use:
                b.fetch_record_stft(hop_div=4)
                b.fetch_record_edges()
            got.append([rec.tobytes(), b.fetch_row_means().tobytes()] + [a.tobytes() for a in b.fetch_record_cells()] + [a.tobytes() for a in b.fetch_record_iq()]
                       + [a.tobytes() for a in b.fetch_record_stft()])

        _run(nperseg, fmt, margin, after, row_means=True, record_cells=True)
        sides[use] = got
    assert sides[False] == sides[True] and len(sides[True]) == N_CALLS


# ---- the estimators ----------------------------------------------------------------------------------------------------------------
def test_the_estimators_against_the_same_estimators_on_the_models_values():
    """``fetch_record_fine(hop_div=4)``: within k (1 / 2 pi) sum_pairs(|c_t| e_{t+1} + |c_{t+1}| e_t + e_t e_{t+1}) / |R_model| bins of
    ``record_fine`` on the model's values, for the records whose model coherence exceeds 0.9 -- the two planted pulses, 0.2 bins
    over their bins' centres, among them.  ``fetch_record_edges(hop_div=4)``: the same NaN pattern as ``record_edges`` on the
    model's values, and each edge within h (e_half + 2 e_q + e_p) / (|a_p - a_q| - e_p - e_q) of it -- q, p the two frames the
    half-level crossing lies between, e their bounds, e_half half the largest bound of a frame inside the record's own cells
    (the median moves by no more than its largest input does)."""
    nperseg, fmt, margin, k = 256, "c64", 2, 4
    h = nperseg // k
    seen = dict(n=0, planted=0, edges=0)

    def after(b, c, rec):
        plan, off, first, values, q, _ = _model(b, rec, fmt, nperseg, k)
        got = b.fetch_record_fine(hop_div=k)
        got_edges = b.fetch_record_edges(hop_div=k)
        assert len(got) == len(rec) and got_edges.shape == (len(rec), 2)
        if q is None:
            return
        want = record_fine(off, first, q.values, rec["start"], rec["end"], sq.FS, nperseg, k, rec["fi"])
        want_edges = record_edges(off, first, q.values, rec["start"], rec["end"], nperseg, k)
        e = rs.bound(q, nperseg, rs.SPP[fmt])
        a = np.abs(q.values).astype(np.float64)
        pos, part, rid = plan["position"], plan["part"], plan["record"]
        own = (pos >= rec["start"].astype(np.int64)[rid] * nperseg) & (pos + nperseg <= rec["end"].astype(np.int64)[rid] * nperseg)
        assert np.array_equal(got["n_pairs"], want["n_pairs"])
        assert np.array_equal(np.isnan(got_edges), np.isnan(want_edges))
        for i, r in enumerate(rec):
            sl = slice(int(off[i]), int(off[i + 1]))
            for col in (0, 1):
                if np.isnan(want_edges[i, col]):
                    continue
                # (a record's positions rise through both parts: the crossing lies between frame j and its successor)
                j = min(int(np.flatnonzero(pos[sl] <= want_edges[i, col] - nperseg / 2)[-1]), sl.stop - sl.start - 2)
                eq, ep = e[sl][j], e[sl][j + 1]
                e_half = 0.5 * e[sl][own[sl]].max()
                da = abs(a[sl][j + 1] - a[sl][j]) - eq - ep
                assert da > 0
                allow = h * (e_half + 2 * max(eq, ep) + max(eq, ep)) / da
                assert abs(got_edges[i, col] - want_edges[i, col]) <= allow, (c, r, col, got_edges[i, col], want_edges[i, col], allow)
                seen["edges"] += 1
            if want["n_pairs"][i] < 1:
                assert np.isnan(got["offset_hz"][i]) and np.isnan(got["coherence"][i])
                continue
            if not want["coherence"][i] > 0.9:
                continue
            pair = own[sl][:-1] & own[sl][1:] & (part[sl][:-1] == part[sl][1:])
            cc, ee, aa = q.values[sl], e[sl], a[sl]
            R = np.abs((cc[1:] * np.conj(cc[:-1]))[pair].sum())
            allow = k * float(((aa[:-1] * ee[1:] + aa[1:] * ee[:-1] + ee[:-1] * ee[1:])[pair]).sum() / R / (2 * np.pi))
            d = abs(got["offset_hz"][i] - want["offset_hz"][i]) / (sq.FS / nperseg)
            assert d <= allow, (c, r, d, allow)
            seen["n"] += 1
            if (r["stream"], r["fi"]) in ((rs.DC_STREAM, rs.DC_BIN), (rs.NEG_STREAM, rs.neg_bin(nperseg))) and want["n_pairs"][i] >= 6 * k:
                assert abs(want["offset_hz"][i] / (sq.FS / nperseg) - rs.FINE_OFFSET_BINS) < 0.02, (r, want[i])
                seen["planted"] += 1

    _run(nperseg, fmt, margin, after)
    assert seen["n"] > 10 and seen["planted"] >= 2 and seen["edges"] > 10, seen
