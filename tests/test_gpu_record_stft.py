"""One complex STFT value per delivered segment (rt_fetch_record_stft) on the GPU.  Every delivered segment's value is held to the
float64 model (longdouble for float64 handles) of the snippet the same handle delivers through ``fetch_record_iq``, within the bound
of tests/record_stft_cases.py; |value|^2 to the detection's own cells; the bytes to themselves across handle kinds and fetches.

Worst |value - model| / bound seen on an MI355X (profiles/record_stft_worst_ratio.txt holds the table): 0.13 - 0.31 per case, one
value at 0.49 (complex64 at nperseg 300, margin 2); the CPU restatement of the kernel's order reaches 0.28."""
import ctypes as C

import numpy as np
import pytest

from pyradiotracking_amd import _native
from pyradiotracking_amd.analyze import BatchSignalAnalyzer, record_fine, stft_constants, stft_constants_f64
from tests import constant_cases as cst
from tests import precision64 as p64
from tests import record_iq_cases as riq
from tests import record_stft_cases as rs
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
    """(window, scale) as the analyzer hands them to the handle"""
    if f64:
        return stft_constants_f64(sq.WINDOW, nperseg, sq.FS)
    w, scale = stft_constants(sq.WINDOW, nperseg, sq.FS)
    return w, float(scale)


def _model(b, rec, fmt, nperseg):
    """(offsets, first, values, Quantities, bound ratios) of the call fetched last: every delivered segment against the model of the
    snippet ``fetch_record_iq`` hands out"""
    f64 = b.precision == "float64"
    base = riq.base_format(fmt)
    off_iq, first_iq, samples = b.fetch_record_iq()
    off, first, values = b.fetch_record_stft()
    assert np.array_equal(off * nperseg, off_iq) and np.array_equal(first, first_iq) and len(off) == len(rec) + 1
    assert values.dtype == (np.complex128 if f64 else np.complex64) and len(values) == off[-1]
    if not len(values):
        return off, first, values, None, np.zeros(0)
    w, scale = _constants(nperseg, f64)
    q = rs.model_values(rs.converted(samples, base, f64), np.repeat(rec["fi"].astype(np.int64), np.diff(off)), w, scale, nperseg, wide=f64)
    return off, first, values, q, rs.ratios(values, q, nperseg, rs.SPP[base], rs.U64 if f64 else rs.U32)


def _run(nperseg, fmt, margin, after, **extra):
    b = _handle(nperseg, fmt, margin, **extra)
    try:
        for k in range(N_CALLS):
            sq.enqueue(b, rs.gpu_feed(nperseg, k, fmt), fmt)
            after(b, k, b.fetch_records())
    finally:
        b.close()


MODEL_CASES = [(32, "c64"), (256, "c64"), (1024, "c64"), (4096, "c64"), (300, "c64"), (300, "u8"), (256, "u8"), (256, "i8"), (256, "i16"),
               (256, "c128"), (256, "u8f64"), (256, "c128-sparse"),
               # beyond the issue's table: segments of 72, 36 and 18 bytes, which the 8-, 4- and 2-byte load paths take
               (9, "c64"), (9, "i16"), (9, "u8")]


@pytest.mark.parametrize("margin", [0, 2])
@pytest.mark.parametrize("nperseg,fmt", MODEL_CASES, ids=lambda v: str(v))
def test_every_delivered_segment_against_the_model(nperseg, fmt, margin):
    extra = {}
    if fmt.endswith("-sparse"):
        fmt, extra = fmt[:-7], dict(f64_sparse=True)
    seen = dict(cells=0, back=0, worst=0.0, dc=0, neg=0, first_call=None)

    def after(b, k, rec):
        off, first, values, q, r = _model(b, rec, fmt, nperseg)
        if k == 0:
            seen["first_call"] = bool((first >= 0).all())  # D = 0: nothing reaches back
        if len(r):
            print(f"record_stft nperseg {nperseg} {fmt} margin {margin} call {k}: {len(r)} values, worst ratio {r.max():.3f}")
            seen["worst"] = max(seen["worst"], float(r.max()))
            assert r.max() <= 1.0, (k, int(r.argmax()), float(r.max()))
        seen["cells"] += len(values)
        seen["back"] += int((first < 0).sum())
        seen["dc"] += int(((rec["stream"] == rs.DC_STREAM) & (rec["fi"] == rs.DC_BIN)).sum())
        seen["neg"] += int(((rec["stream"] == rs.NEG_STREAM) & (rec["fi"] == rs.neg_bin(nperseg))).sum())

    _run(nperseg, fmt, margin, after, **extra)
    assert seen["first_call"] and seen["cells"] > 0, seen
    if nperseg >= 32:
        assert seen["cells"] > 100 and seen["back"] > 0 and seen["dc"] > 0 and seen["neg"] > 0, seen


def test_the_squared_magnitude_is_the_detections_cell():
    """``record_cells=True``: |value|^2 of a record's own cells against ``fetch_record_cells`` within twice precision64's cell bound
    (of the form that bounds the fused scans on complex64 under hamming, ``lin``)."""
    nperseg, fmt, margin = 256, "c64", 2
    n = [0]

    def after(b, k, rec):
        off_c, cells = b.fetch_record_cells()
        off_iq, _, samples = b.fetch_record_iq()
        off, first, values = b.fetch_record_stft()
        for i, r in enumerate(rec):
            fi, start, end = int(r["fi"]), int(r["start"]), int(r["end"])
            own = cells[off_c[i]:off_c[i + 1]]
            assert len(own) == end - start
            lo = max(start, int(first[i]))  # (a lead the handle does not hold clips the delivered segments, not the cells)
            if lo >= end:
                continue
            v = values[off[i] + lo - first[i]:off[i] + end - first[i]].astype(np.complex128)
            snippet = samples[off_iq[i] + (lo - first[i]) * nperseg:off_iq[i] + (end - first[i]) * nperseg]
            ref = p64.stft_power_f64(snippet, sq.FS, sq.WINDOW, nperseg)
            dP = p64.cell_bounds(ref, "lin").dP[:, fi]
            got = v.real ** 2 + v.imag ** 2
            assert (np.abs(got - own[lo - start:].astype(np.float64)) <= 2 * dP).all(), (k, i, r)
            n[0] += len(v)

    _run(nperseg, fmt, margin, after, record_cells=True)
    assert n[0] > 100


def _values_by_record(b, rec):
    off, first, values = b.fetch_record_stft()
    again = b.fetch_record_stft()
    assert values.tobytes() == again[2].tobytes() and np.array_equal(off, again[0])  # a second fetch of the same call
    return {(int(r["stream"]), int(r["fi"]), int(r["start"]), int(r["end"]), int(first[i])): values[off[i]:off[i + 1]].tobytes()
            for i, r in enumerate(rec)}


def test_the_same_samples_give_the_same_bytes_on_every_handle_kind():
    nperseg, fmt, margin = 256, "c64", 2
    runs = {}
    for name, extra in (("plain", dict(mode="sparse")), ("dense", dict(mode="dense")), ("lanes", dict(mode="sparse", lanes=2))):
        got = []
        _run(nperseg, fmt, margin, lambda b, k, rec: got.append(_values_by_record(b, rec)), **extra)
        runs[name] = got
    for name in ("dense", "lanes"):
        common = 0
        for k in range(N_CALLS):
            for key, v in runs["plain"][k].items():
                if key in runs[name][k]:
                    assert runs[name][k][key] == v, (name, k, key)
                    common += 1
        assert common >= 0.9 * sum(len(c) for c in runs["plain"]) > 20, (name, common)


def test_a_chained_handle_gives_the_bytes_of_sequential_calls():
    """One recording of four buffers: through a ``chain=4`` handle in one call, and through a plain handle in four."""
    nperseg, margin, links, T = 256, 2, 4, 24
    # (a buffer's first and last twelve whole segments: the tones are bin-centred, so the cut keeps their phase, and both the heads
    # at a buffer's start and the tails at its end that make a record reach back are kept)
    half = T // 2 * nperseg
    bufs = []
    for k in range(links):
        x = rs.gpu_buffer(nperseg, k)[rs.NEG_STREAM][:SCHED.T[k] * nperseg]
        bufs.append(np.ascontiguousarray(np.concatenate([x[:half], x[len(x) - half:]])))
    kw = dict(sq.settings(nperseg), mode="sparse", record_iq=True, record_iq_margin=margin)
    seq = {}
    b = BatchSignalAnalyzer(["0"], sdr_callback_length=T * nperseg, **kw)
    try:
        for k, x in enumerate(bufs):
            b.enqueue(x[None, :])
            for key, v in _values_by_record(b, b.fetch_records()).items():
                seq[(k,) + key[1:]] = v
    finally:
        b.close()
    c = BatchSignalAnalyzer(["0"], sdr_callback_length=T * nperseg, chain=links, **kw)
    try:
        c.enqueue(np.concatenate(bufs)[None, :], links=links)
        chained = _values_by_record(c, c.fetch_records())
    finally:
        c.close()
    common = [key for key in chained if key in seq]
    assert len(common) >= 0.9 * len(seq) > 8 and any(key[4] < 0 for key in common), (len(common), len(seq))
    for key in common:
        assert chained[key] == seq[key], key


def test_a_constant_segment_is_exactly_zero():
    """tests/constant_cases.py, int16 rails at nperseg 256: the record's head cell is the constant segment."""
    c = cst.BY_NAME["fam256box"]
    assert c.fmt == "i16" and c.nperseg == 256 and c.const == cst.RAIL16
    lengths, consts, _, want = cst.layout(c)
    (k_const, t_const), = consts
    b = BatchSignalAnalyzer([str(i) for i in range(cst.S)], sdr_callback_length=max(lengths), mode=c.mode, segs_per_chunk=c.spc, record_iq=True,
                            record_iq_margin=0, **cst.settings(c))
    hit = 0
    try:
        for k, buf in enumerate(cst.wire(c.name)):
            b.enqueue_int16(np.array(buf))
            rec = b.fetch_records()
            off, first, values = b.fetch_record_stft()
            for i, r in enumerate(rec):
                if k == k_const and r["stream"] == cst.TARGET and first[i] <= t_const < first[i] + off[i + 1] - off[i]:
                    v = values[off[i] + t_const - first[i]]
                    assert v.real == 0 and v.imag == 0, (r, v)
                    others = np.delete(values[off[i]:off[i + 1]], t_const - first[i])
                    assert (np.abs(others) > 0).all()
                    hit += 1
    finally:
        b.close()
    assert hit >= 1


def test_a_nan_sample_makes_its_segment_nan_and_no_other():
    nperseg, fmt, margin = 256, "c64", 2
    t_nan = SCHED.T[1] - 1  # call 1's last segment: the records of call 2 that start at its segment 0 deliver it as segment -1
    n_nan = [0]

    def after(b, k, rec):
        off_iq, _, samples = b.fetch_record_iq()
        off, first, values = b.fetch_record_stft()
        holds = np.isnan(samples.reshape(-1, nperseg)).any(axis=1)
        assert np.array_equal(np.isnan(values.real) & np.isnan(values.imag), holds) and np.array_equal(np.isnan(values.real) | np.isnan(values.imag), holds)
        n_nan[0] += int(holds.sum())

    b = _handle(nperseg, fmt, margin)
    try:
        for k in range(N_CALLS):
            x = rs.gpu_feed(nperseg, k, fmt).copy()
            if k == 1:
                x[rs.NEG_STREAM, t_nan * nperseg + 5] = np.nan
            b.enqueue(x)
            after(b, k, b.fetch_records())
    finally:
        b.close()
    assert n_nan[0] >= 1


def test_fetch_record_fine_against_the_models_estimate():
    """The estimate from the GPU's values against the same arithmetic on the model's, within (1 / 2 pi) sum_pairs(|c_t| e_{t+1} +
    |c_{t+1}| e_t + e_t e_{t+1}) / |R_model| bins, for the records whose model coherence exceeds 0.9 -- the two planted pulses,
    0.2 bins over their bins' centres, among them."""
    nperseg, fmt, margin = 256, "c64", 2
    seen = dict(n=0, planted=0)

    def after(b, k, rec):
        off, first, values, q, _ = _model(b, rec, fmt, nperseg)
        got = b.fetch_record_fine()
        assert len(got) == len(rec)
        if q is None:
            return
        want = record_fine(off, first, q.values, rec["start"], rec["end"], sq.FS, nperseg)
        e = rs.bound(q, nperseg, rs.SPP[fmt])
        assert np.array_equal(got["n_pairs"], want["n_pairs"])
        for i, r in enumerate(rec):
            if want["n_pairs"][i] < 1:
                assert np.isnan(got["offset_hz"][i]) and np.isnan(got["coherence"][i])
                continue
            if not want["coherence"][i] > 0.9:
                continue
            sl = slice(off[i] + max(int(r["start"]), int(first[i])) - first[i], off[i] + int(r["end"]) - first[i])
            c, ee = q.values[sl], e[sl]
            seg = np.arange(sl.start, sl.stop) - off[i] + first[i]
            keep = seg[:-1] != -1  # (the pair across the buffer boundary is not used)
            a = np.abs(c)
            allow = float(((a[:-1] * ee[1:] + a[1:] * ee[:-1] + ee[:-1] * ee[1:])[keep]).sum() / np.abs((c[1:] * np.conj(c[:-1]))[keep].sum()) / (2 * np.pi))
            d = abs(got["offset_hz"][i] - want["offset_hz"][i]) / (sq.FS / nperseg)
            assert d <= allow, (k, r, d, allow)
            seen["n"] += 1
            if (r["stream"], r["fi"]) in ((rs.DC_STREAM, rs.DC_BIN), (rs.NEG_STREAM, rs.neg_bin(nperseg))) and want["n_pairs"][i] >= 6:
                assert abs(want["offset_hz"][i] / (sq.FS / nperseg) - rs.FINE_OFFSET_BINS) < 0.02, (r, want[i])
                seen["planted"] += 1

    _run(nperseg, fmt, margin, after)
    assert seen["n"] > 10 and seen["planted"] >= 2, seen


# ---- refusals, queries, side effects -----------------------------------------------------------------------------------------------
def _fetch_stft(b, n_rec, cap=None, f64=None, n_off=None):
    lib, h = b.native._lib, b.native._handle
    f64 = (b.precision == "float64") if f64 is None else f64
    fn = lib.rt_fetch_record_stft_f64 if f64 else lib.rt_fetch_record_stft
    off = np.zeros((n_rec if n_off is None else n_off) + 1, np.int64)
    first = np.zeros(n_rec, np.int32)
    n = C.c_size_t(0)
    rc = fn(h, off.ctypes.data, off.size, first.ctypes.data, first.size, None, 0, C.byref(n))
    if rc != _native.RT_OK or cap is None:
        return rc, n.value, None
    buf = np.full(2 * max(cap, 1), 7.5, np.float64 if f64 else np.float32)
    rc = fn(h, off.ctypes.data, off.size, first.ctypes.data, first.size, buf.ctypes.data, cap, C.byref(n))
    return rc, n.value, buf


def _err(b):
    return b.native._lib.rt_last_error(b.native._handle).decode()


def test_refusals_and_the_size_query():
    nperseg, fmt = 256, "c64"
    feeds = [rs.gpu_feed(nperseg, k, fmt) for k in range(N_CALLS)]
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
            off_handle.fetch_record_stft()
        assert ei.value.code == _native.RT_E_INVALID and "rt_fetch_record_stft: rt_set_record_iq" in str(ei.value)
        # no delivered call yet
        assert _fetch_stft(b, 0)[0] == _native.RT_E_INVALID and _err(b).startswith("rt_fetch_record_stft: no samples")
        both(feeds[0])
        same()
        both(feeds[1])
        rec = same()
        n_rec = len(rec)
        assert n_rec > 0
        # a null n_cells; the wrong twin, both ways
        h = b.native._handle
        assert lib.rt_fetch_record_stft(h, None, 0, None, 0, None, 0, None) == _native.RT_E_INVALID
        assert _fetch_stft(b, n_rec, f64=True)[0] == _native.RT_E_INVALID and "float32 handle" in _err(b) and "rt_fetch_record_stft_f64" in _err(b)
        d64.enqueue(feeds[1].astype(np.complex128))
        n64 = len(d64.fetch_records())
        assert _fetch_stft(d64, n64, f64=False)[0] == _native.RT_E_INVALID and "float64 handle" in _err(d64)
        assert _fetch_stft(d64, n64)[0] == _native.RT_OK
        # size query, then fetch; cap one short; wrong counts
        rc, n_cells, _ = _fetch_stft(b, n_rec)
        assert rc == _native.RT_OK and n_cells > 0
        rc, _, buf = _fetch_stft(b, n_rec, n_cells - 1)
        assert rc == _native.RT_E_CAPACITY and np.all(buf == 7.5)
        assert _fetch_stft(b, n_rec + 1)[0] == _native.RT_E_INVALID and _fetch_stft(b, n_rec, n_off=n_rec + 1)[0] == _native.RT_E_INVALID
        rc, n2, buf = _fetch_stft(b, n_rec, n_cells)
        assert rc == _native.RT_OK and n2 == n_cells
        assert buf[:2 * n_cells].view(np.complex64).tobytes() == b.fetch_record_stft()[2].tobytes() and np.all(buf[2 * n_cells:] == 7.5)
        # after the next enqueue; with two in flight: process k, process k + 1, fetch k, then the values of k
        both(feeds[2])
        assert _fetch_stft(b, n_rec)[0] == _native.RT_E_INVALID
        both(feeds[3])
        rec = same()
        assert _fetch_stft(b, len(rec))[0] == _native.RT_OK
        # a truncated delivery
        n = C.c_size_t(0)
        out = np.zeros(2, _native.RECORD_DTYPE)
        lib.rt_fetch(h, out.ctypes.data, 2, C.byref(n))
        assert n.value > 2
        assert _fetch_stft(b, 2)[0] == _native.RT_E_INVALID and _err(b) == "rt_fetch_record_stft: the call fetched last was delivered truncated"
        twin.fetch_records()
        # after rt_extract (on both handles: it moves the look-back)
        spec = np.zeros((S, 4, nperseg), np.float32)
        d = _native.DeviceBuffer(0, spec.nbytes)
        d.upload(spec)
        for x in (b, twin):
            x.native.extract_device(d.ptr, 4, nperseg, None, 0)
            x.fetch_records()
        assert _fetch_stft(b, 0)[0] == _native.RT_E_INVALID and "rt_extract" in _err(b)
        d.free()
        # a call without records
        both(np.zeros((S, 4 * nperseg), np.complex64))
        assert len(same()) == 0
        rc, n_cells, _ = _fetch_stft(b, 0)
        assert rc == _native.RT_OK and n_cells == 0
        # the feature turned off again
        b.native.set_record_iq(-1)
        twin.native.set_record_iq(-1)
        both(feeds[0])
        same()
        assert _fetch_stft(b, 0)[0] == _native.RT_E_INVALID and "rt_set_record_iq" in _err(b)
        for k in (1, 2):
            both(feeds[k])
            same()
    finally:
        for x in (b, twin, d64, off_handle):
            x.close()


def test_the_entry_changes_nothing_else():
    """With the entry never called and with it called after every fetch, in front of everything else: the records, row means,
    record cells and record IQ are the same bytes."""
    nperseg, fmt, margin = 256, "c64", 2
    sides = {}
    for use in (False, True):
        got = []

        def after(b, k, rec, use=use, got=got):
            if use:
                b.fetch_record_stft()
            got.append([rec.tobytes(), b.fetch_row_means().tobytes()] + [a.tobytes() for a in b.fetch_record_cells()] + [a.tobytes() for a in b.fetch_record_iq()])

        _run(nperseg, fmt, margin, after, row_means=True, record_cells=True)
        sides[use] = got
    assert sides[False] == sides[True] and len(sides[True]) == N_CALLS
