"""Per-record estimates reduced on the device (rt_fetch_record_estimates) on the GPU.  Every row is held to ``record_fine`` and
``record_edges`` applied to the frames the SAME handle returns from ``fetch_record_stft(hop_div=k)`` -- the inputs are bit for bit
the same, so the frames' own round-off is out of the picture -- within the bounds tests/record_estimates_cases.py derives; the
counts and the NaN pattern of every field must be equal.  The rows' bytes are held to themselves across handle kinds, fetches and
orders of calls.

profiles/record_estimates_worst_ratio.txt holds the worst |row - model| / bound per case."""
import ctypes as C
import os

import numpy as np
import pytest

from pyradiotracking_amd import _native
from pyradiotracking_amd.analyze import ESTIMATES_DTYPE, BatchSignalAnalyzer, SignalAnalyzer
from tests import constant_cases as cst
from tests import nonfinite_cases as nf
from tests import record_estimates_cases as ec
from tests import record_stft_cases as rs
from tests import sequence_cases as sq

pytestmark = pytest.mark.gpu

SCHED = rs.GPU_SCHEDULE
S = rs.GPU_S
N_CALLS = len(SCHED.T)
NAME = "rt_fetch_record_estimates"
WORST = {}


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


def _run(nperseg, fmt, margin, after, **extra):
    b = _handle(nperseg, fmt, margin, **extra)
    try:
        for c in range(N_CALLS):
            sq.enqueue(b, rs.gpu_feed(nperseg, c, fmt), fmt)
            after(b, c, b.fetch_records())
    finally:
        b.close()


def _against_the_model(name, b, rec, nperseg, k):
    """the rows of the call fetched last against the model on the same handle's frames: (rows, model, frames' offsets, first)"""
    got = b.native.fetch_record_estimates(k)
    off, first, values = b.fetch_record_stft(hop_div=k)
    assert got.dtype == _native.ESTIMATE_DTYPE and len(got) == len(rec) == len(off) - 1
    m = ec.model(off, first, values, rec["start"], rec["end"], rec["fi"], nperseg, k)
    worst, out, bad = ec.compare(got, m, nperseg, k)
    print(f"record_estimates {name}: {len(rec)} records, " + " ".join(f"{f} {v:.3f}" for f, v in worst.items()) + f", {out} without clearance")
    assert not bad, (name, bad[:4])
    w = WORST.setdefault(name, dict.fromkeys(worst, 0.0))
    for f, v in worst.items():
        w[f] = max(w[f], v)
    # the Python method: the same rows under its names, offset_hz in the model's own units
    rows = b.fetch_record_estimates(hop_div=k)
    assert rows.dtype == ESTIMATES_DTYPE and rows["coherence"].tobytes() == got["coherence"].tobytes() and rows["rise"].tobytes() == got["rise"].tobytes()
    assert np.array_equal(rows["n_pairs"], got["n_pairs"]) and rows["r"].real.tobytes() == got["r_re"].tobytes()
    assert np.array_equal(rows["offset_hz"], got["offset_bins"] * float(b.sample_rate) / nperseg, equal_nan=True)
    return got, m, off, first, out


# (nperseg, format, k)
MODEL_CASES = [(256, "c64", 4), (256, "c64", 1), (32, "c64", 16), (1024, "c64", 2), (256, "u8", 4), (256, "i16", 4), (9, "c64", 3), (256, "c128", 4),
               (256, "c128-sparse", 4)]


@pytest.mark.parametrize("margin", [0, 2])
@pytest.mark.parametrize("nperseg,fmt,k", MODEL_CASES, ids=lambda v: str(v))
def test_every_row_against_the_model(nperseg, fmt, k, margin):
    extra = {}
    label = f"{nperseg} {fmt} k={k} margin {margin}"
    if fmt.endswith("-sparse"):
        fmt, extra = fmt[:-7], dict(f64_sparse=True)
    seen = dict(records=0, back=0, pairs=0, edges=0, left_out=0)

    def after(b, c, rec):
        got, m, off, first, out = _against_the_model(label, b, rec, nperseg, k)
        seen["records"] += len(rec)
        seen["back"] += int((first < 0).sum())
        seen["pairs"] += int((got["n_pairs"] > 0).sum())
        seen["edges"] += int(np.isfinite(got["rise"]).sum() + np.isfinite(got["fall"]).sum())
        seen["left_out"] += out

    _run(nperseg, fmt, margin, after, **extra)
    assert seen["left_out"] <= 1, seen  # (none is expected)
    assert seen["records"] > 0 and seen["pairs"] > 0, seen
    if nperseg >= 32:
        assert seen["records"] > 20 and seen["back"] > 0, seen  # records with a predecessor part occur
    if margin and nperseg >= 32:
        assert seen["edges"] > 10, seen


# ---- size edges ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("margin", [0, 2])
def test_size_edges(margin):
    """tests/record_estimates_cases.py's boxcar pulses at nperseg 32: 1, 2, 3, 63, 64, 65, 127, 128, 129 inside frames at k = 1 and
    the record of 1 105 frames at k = 16 (margin 0).  NOT COVERED, because it cannot occur: "a pulse cut by the buffer's end".  The
    reference reports a pulse that runs to the buffer's end in the next call (tests/test_record_estimates_contract.py shows the
    oracle doing so), so no record of a call ends at the buffer's end with its pulse still on; the only thing that leaves a fall
    NaN is margin 0, where nothing behind the record is delivered, and that is what this test holds.
    The pulse on segment 0 of the first buffer has nothing below half in front either: both edges NaN.  Every other record holds the
    cold cell before its pulse: the pulse is still rising at its first inside frame, and the rise is found at margin 0 too.  Call
    2's record (-6, 4) began in the previous buffer: its rise lies in the predecessor part, and no pair crosses the parts."""
    b = BatchSignalAnalyzer([str(i) for i in range(ec.EDGE_S)], sdr_callback_length=ec.EDGE_T * ec.EDGE_N, lanes=1, record_iq=True, record_iq_margin=margin,
                            **ec.edge_settings())
    N = ec.EDGE_N
    want = ec.edge_oracle_records()
    try:
        for c in range(ec.EDGE_CALLS):
            b.enqueue(ec.edge_feed(c))
            rec = b.fetch_records()
            assert [(int(r["stream"]), int(r["fi"]), int(r["start"]), int(r["end"])) for r in rec] == [(s, *t) for s, per in enumerate(want[c]) for t in per]
            got, m, off, first, out = _against_the_model(f"size edges margin {margin} k=1", b, rec, N, 1)
            assert out == 0
            if c == 0:
                assert got["n_inside"].tolist() == list(ec.EDGE_INSIDE) + [ec.EDGE_LONG]
                assert got["n_pairs"].tolist() == [n - 1 for n in got["n_inside"]]
                # the pulse on segment 0: nothing delivered lies in front of it, and at margin 0 nothing behind it
                assert np.isnan(got["rise"][0]) and np.isnan(got["fall"][0]) == (margin == 0)
                # still rising at the first inside frame: the rise is interpolated between it and its successor, inside the record
                assert np.isfinite(got["rise"][1:]).all() and (got["rise"][1:] > rec["start"][1:] * N).all() and (got["rise"][1:] < (rec["start"][1:] + 2) * N).all()
                assert np.isnan(got["fall"]).all() if margin == 0 else np.isfinite(got["fall"][1:]).all()
                # boxcar, switched at segment borders: |c| steps from noise to the level, the half level is crossed half-way
                # (from three inside frames on: the median of a cold and a hot cell is half the level)
                assert np.abs(got["rise"][2:] - (rec["start"][2:] + 1) * N).max() < 0.01 * N
                g16, m16, off16, _, out16 = _against_the_model(f"size edges margin {margin} k=16", b, rec, N, 16)
                assert out16 == 0
                if margin == 0:
                    assert np.diff(off16)[-1] == 1105 and g16["n_inside"][-1] == 1105 and g16["n_pairs"][-1] == 1104
                else:
                    assert np.diff(off16)[-1] > 1105
                assert abs(g16["coherence"][-1] - 1) < 1e-3 and abs(g16["offset_bins"][-1]) < 1e-3
            else:
                i = len(rec) - 1
                assert (int(rec["start"][i]), int(rec["end"][i])) == (-6, 4) and first[i] <= -6
                assert got["n_inside"][i] == 10 and got["n_pairs"][i] == 5 + 3  # no pair across the two parts
                assert np.isfinite(got["rise"][i]) and -6 * N < got["rise"][i] < -4 * N  # ... in the predecessor part
                assert np.isnan(got["fall"][i]) == (margin == 0)
    finally:
        b.close()


# ---- the same bytes --------------------------------------------------------------------------------------------------------------------
def _rows_by_record(b, rec, k):
    rows = b.native.fetch_record_estimates(k)
    assert rows.tobytes() == b.native.fetch_record_estimates(k).tobytes()  # a second fetch of the same call
    first = b.fetch_record_stft(hop_div=k)[1]
    return {(int(r["stream"]), int(r["fi"]), int(r["start"]), int(r["end"]), int(first[i])): rows[i].tobytes() for i, r in enumerate(rec)}


def test_the_same_samples_give_the_same_bytes_on_every_handle_kind():
    nperseg, fmt, margin, k = 256, "c64", 2, 4
    runs = {}
    for name, extra in (("plain", dict(mode="sparse")), ("dense", dict(mode="dense")), ("lanes", dict(mode="sparse", lanes=3))):
        got = []
        _run(nperseg, fmt, margin, lambda b, c, rec: got.append(_rows_by_record(b, rec, k)), **extra)
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
    """One recording of four buffers: through a ``chain=4`` handle in one call, and through a plain handle in four.  rise and fall
    count from sample 0 of the CALL's buffer, so a chained link's rows are compared with its own buffer's offset taken off."""
    nperseg, margin, links, T, k = 256, 2, 4, 24, 4
    half = T // 2 * nperseg
    bufs = []
    for c in range(links):
        x = rs.gpu_buffer(nperseg, c)[rs.NEG_STREAM][:SCHED.T[c] * nperseg]
        bufs.append(np.ascontiguousarray(np.concatenate([x[:half], x[len(x) - half:]])))
    kw = dict(sq.settings(nperseg), mode="sparse", record_iq=True, record_iq_margin=margin)
    fields = [f for f in _native.ESTIMATE_DTYPE.names if f not in ("rise", "fall")]
    seq = {}
    b = BatchSignalAnalyzer(["0"], sdr_callback_length=T * nperseg, **kw)
    try:
        for c, x in enumerate(bufs):
            b.enqueue(x[None, :])
            for key, v in _rows_by_record(b, b.fetch_records(), k).items():
                seq[(c,) + key[1:]] = np.frombuffer(v, _native.ESTIMATE_DTYPE)[0]
    finally:
        b.close()
    ch = BatchSignalAnalyzer(["0"], sdr_callback_length=T * nperseg, chain=links, **kw)
    try:
        ch.enqueue(np.concatenate(bufs)[None, :], links=links)
        chained = {key: np.frombuffer(v, _native.ESTIMATE_DTYPE)[0] for key, v in _rows_by_record(ch, ch.fetch_records(), k).items()}
    finally:
        ch.close()
    common = [key for key in chained if key in seq]
    assert len(common) >= 0.9 * len(seq) > 8 and any(key[4] < 0 for key in common), (len(common), len(seq))
    edges = 0
    for key in common:
        assert chained[key][fields].tobytes() == seq[key][fields].tobytes(), key
        for f in ("rise", "fall"):
            a, w = float(chained[key][f]), float(seq[key][f])
            assert np.isnan(a) == np.isnan(w), (key, f)
            if not np.isnan(a):
                assert a == w, (key, f, a, w)  # (a link's records count segments from the link's own buffer: so do the positions)
                edges += 1
    assert edges > 4


def test_the_order_of_calls_does_not_change_the_bytes():
    nperseg, fmt, margin = 256, "c64", 2
    n = [0]

    def after(b, c, rec):
        e4 = b.native.fetch_record_estimates(4)
        s2 = b.fetch_record_stft(hop_div=2)
        seg = b.fetch_record_stft()
        e4b = b.native.fetch_record_estimates(4)
        e2 = b.native.fetch_record_estimates(2)
        s4 = b.fetch_record_stft(hop_div=4)
        e1 = b.native.fetch_record_estimates(1)
        assert e4.tobytes() == e4b.tobytes() == b.native.fetch_record_estimates(4).tobytes()
        # ... and the other way round on a twin call: the frames first, the rows after
        assert s4[2].tobytes() == b.fetch_record_stft(hop_div=4)[2].tobytes() and seg[2].tobytes() == b.fetch_record_stft()[2].tobytes()
        assert e2.tobytes() == b.native.fetch_record_estimates(2).tobytes() and e1.tobytes() == b.native.fetch_record_estimates(1).tobytes()
        assert s2[2].tobytes() == b.fetch_record_stft(hop_div=2)[2].tobytes()
        n[0] += len(e4)

    _run(nperseg, fmt, margin, after)
    firsts = []
    _run(nperseg, fmt, margin, lambda b, c, rec: firsts.append((b.fetch_record_stft(hop_div=4)[2].tobytes(), b.native.fetch_record_estimates(4).tobytes())))
    rows_first = []
    _run(nperseg, fmt, margin, lambda b, c, rec: rows_first.append((b.native.fetch_record_estimates(4).tobytes(), b.fetch_record_stft(hop_div=4)[2].tobytes())))
    assert [(f, r) for r, f in rows_first] == firsts and n[0] > 20


# ---- a constant segment, a NaN sample --------------------------------------------------------------------------------------------------
def test_frames_of_a_constant_run_and_the_model():
    """tests/constant_cases.py, int16 rails at nperseg 256: the frames inside the run are exactly 0 + 0j; the rows keep to the model
    through them (a record whose inside frames are all zero has level 0, no edge and coherence 0 / 0)."""
    c = cst.BY_NAME["fam256box"]
    assert c.fmt == "i16" and c.nperseg == 256
    lengths, consts, _, want = cst.layout(c)
    b = BatchSignalAnalyzer([str(i) for i in range(cst.S)], sdr_callback_length=max(lengths), mode=c.mode, segs_per_chunk=c.spc, record_iq=True,
                            record_iq_margin=1, **cst.settings(c))
    zeros = 0
    try:
        for buf in cst.wire(c.name):
            b.enqueue_int16(np.array(buf))
            rec = b.fetch_records()
            got, m, off, first, out = _against_the_model("constant run", b, rec, c.nperseg, 4)
            values = b.fetch_record_stft(hop_div=4)[2]
            zeros += int(((values.real == 0) & (values.imag == 0)).sum())
    finally:
        b.close()
    assert zeros >= 1


def test_a_nan_sample_and_its_clean_twin():
    """A NaN sample in call 1's last segment: the rows equal the model's NaN pattern on the dirty handle's own frames, and every
    record none of whose frames covers the sample has the clean twin's bytes."""
    nperseg, fmt, margin, k = 256, "c64", 2, 4
    t_nan = SCHED.T[1] - 1
    sides = {}
    seen = dict(nan_rows=0, same=0, nan_frames=0)
    for dirty in (False, True):
        got = []
        b = _handle(nperseg, fmt, margin)
        try:
            for c in range(N_CALLS):
                x = rs.gpu_feed(nperseg, c, fmt).copy()
                if dirty and c == 1:
                    x[rs.NEG_STREAM, t_nan * nperseg + 5] = np.nan
                b.enqueue(x)
                rec = b.fetch_records()
                rows, m, off, first, out = _against_the_model("a NaN sample" if dirty else "the clean twin", b, rec, nperseg, k)
                values = b.fetch_record_stft(hop_div=k)[2]
                holds = np.array([np.isnan(values[off[i]:off[i + 1]]).any() for i in range(len(rec))], bool)
                got.append({(int(r["stream"]), int(r["fi"]), int(r["start"]), int(r["end"]), int(first[i])): (rows[i].tobytes(), bool(holds[i]), rows[i])
                            for i, r in enumerate(rec)})
        finally:
            b.close()
        sides[dirty] = got
    for c in range(N_CALLS):
        for key, (row, holds, r) in sides[True][c].items():
            seen["nan_frames"] += int(holds)
            seen["nan_rows"] += int(np.isnan(r["level"]) and r["n_inside"] > 0)
            if not holds and key in sides[False][c]:
                assert row == sides[False][c][key][0], (c, key)
                seen["same"] += 1
            assert not sides[False][c].get(key, (None, False))[1]
    assert seen["nan_frames"] >= 1 and seen["same"] > 20, seen


NONFINITE = nf.four_kinds_two_positions(256, "c64") + nf.four_kinds_two_positions(256, "c128")[:2]


@pytest.mark.parametrize("case", NONFINITE, ids=nf.case_id)
def test_the_nonfinite_feeds(case):
    """tests/nonfinite_cases.py: a NaN, a NaN in the imaginary part alone, +inf in the real and -inf in the imaginary part of one
    sample of stream 2, in segment 7 or in the last segment (the look-back of call 1), at a 1-hop or a 4-hop minimum.  The rows
    have the model's NaN / Inf pattern on the dirty handle's own frames (``ec.compare``), in all three calls, and every record none
    of whose frames covers the sample has the clean twin's bytes."""
    k, margin = 4, 2
    sides = {}
    for dirty in (False, True):
        kw = dict(precision="float64") if case.fmt == "c128" else dict(segs_per_chunk=nf.SEGS_PER_CHUNK)
        b = BatchSignalAnalyzer([str(i) for i in range(nf.n_streams(case.nperseg))], sdr_callback_length=nf.n_samples(case.nperseg), record_iq=True,
                                record_iq_margin=margin, **nf.settings(case.nperseg, case.hops), **kw)
        got = []
        try:
            for c, x in enumerate(nf.buffers(case, poisoned=dirty)):
                b.enqueue(np.array(x))
                rec = b.fetch_records()
                rows, m, off, first, out = _against_the_model("nonfinite " + nf.case_id(case) if dirty else "nonfinite feeds, clean", b, rec, case.nperseg, k)
                assert out == 0
                values = b.fetch_record_stft(hop_div=k)[2]
                holds = np.array([not np.isfinite(values[off[i]:off[i + 1]].view(values.real.dtype)).all() for i in range(len(rec))], bool)
                got.append({(int(r["stream"]), int(r["fi"]), int(r["start"]), int(r["end"]), int(first[i])): (rows[i].tobytes(), bool(holds[i]), rows[i])
                            for i, r in enumerate(rec)})
        finally:
            b.close()
        sides[dirty] = got
    seen = dict(holds=0, same=0, nan_level=0, nan_r=0, edge_past=0)
    for c in range(nf.N_CALLS):
        assert not any(h for _, h, _ in sides[False][c].values())
        for key, (row, holds, r) in sides[True][c].items():
            if holds:
                assert key[0] == nf.POISONED
                seen["holds"] += 1
                seen["nan_level"] += int(np.isnan(r["level"]) and r["n_inside"] > 0)
                seen["nan_r"] += int(np.isnan(r["r_re"]) and r["n_pairs"] > 0)
                seen["edge_past"] += int(np.isfinite(r["level"]))  # the frames that cover the sample lie in the margin alone
            elif key in sides[False][c]:
                assert row == sides[False][c][key][0], (c, key)
                seen["same"] += 1
    print(f"record_estimates nonfinite {nf.case_id(case)}: {seen}")
    assert seen["holds"] >= 1 and seen["nan_level"] >= 1 and seen["nan_r"] >= 1 and seen["same"] > 20, seen


# ---- refusals, queries, side effects ---------------------------------------------------------------------------------------------------
def _fetch(b, k, cap=None):
    lib, h = b.native._lib, b.native._handle
    n = C.c_size_t(0)
    rc = lib.rt_fetch_record_estimates(h, k, None, 0, C.byref(n))
    if rc != _native.RT_OK or cap is None:
        return rc, n.value, None
    buf = np.full(9 * max(cap, 1), 7.5, np.float64)
    rc = lib.rt_fetch_record_estimates(h, k, buf.ctypes.data, cap, C.byref(n))
    return rc, n.value, buf


def _err(b):
    return b.native._lib.rt_last_error(b.native._handle).decode()


def test_refusals_and_the_size_query():
    nperseg, fmt, k = 256, "c64", 4
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
        # record_iq off
        off_handle.enqueue(feeds[0])
        off_handle.fetch_records()
        with pytest.raises(_native.NativeError) as ei:
            off_handle.fetch_record_estimates(hop_div=k)
        assert ei.value.code == _native.RT_E_INVALID and NAME + ": rt_set_record_iq" in str(ei.value)
        # no delivered call yet
        assert _fetch(b, k)[0] == _native.RT_E_INVALID and _err(b).startswith(NAME + ": no samples")
        both(feeds[0])
        same()
        both(feeds[1])
        rec = same()
        n_rec = len(rec)
        assert n_rec > 1
        # a null n_out
        h = b.native._handle
        assert lib.rt_fetch_record_estimates(h, k, None, 0, None) == _native.RT_E_INVALID
        # one entry for both handle kinds
        d64.enqueue(feeds[1].astype(np.complex128))
        n64 = len(d64.fetch_records())
        rc, n, buf = _fetch(d64, k, n64)
        assert rc == _native.RT_OK and n == n64 > 0 and not np.any(buf[:9 * n64] == 7.5)
        # a hop that is no divisor of nperseg in 1 .. 16: refused, the message names k and N, nothing written
        for bad in (0, 17, 3, -4):
            rc, _, _ = _fetch(b, bad)
            assert rc == _native.RT_E_INVALID and f"k = {bad}" in _err(b) and f"N = {nperseg}" in _err(b) and _err(b).startswith(NAME + ":"), _err(b)
            with pytest.raises(_native.NativeError):
                b.fetch_record_estimates(hop_div=bad)
        assert _fetch(d64, 3)[0] == _native.RT_E_INVALID and _err(d64).startswith(NAME + ":")
        # size query, then fetch; cap one short: nothing written
        rc, n, _ = _fetch(b, k)
        assert rc == _native.RT_OK and n == n_rec
        rc, n, buf = _fetch(b, k, n_rec - 1)
        assert rc == _native.RT_E_CAPACITY and n == n_rec and np.all(buf == 7.5) and "too small" in _err(b)
        rc, n, buf = _fetch(b, k, n_rec + 3)
        assert rc == _native.RT_OK and n == n_rec and np.all(buf[9 * n_rec:] == 7.5)
        assert buf[:9 * n_rec].tobytes() == b.native.fetch_record_estimates(k).tobytes()
        # after the next enqueue; with two in flight: process c, process c + 1, fetch c, then the rows of c
        both(feeds[2])
        assert _fetch(b, k)[0] == _native.RT_E_INVALID
        both(feeds[3])
        rec = same()
        assert _fetch(b, k)[:2] == (_native.RT_OK, len(rec))
        # a truncated delivery
        n = C.c_size_t(0)
        out = np.zeros(2, _native.RECORD_DTYPE)
        lib.rt_fetch(h, out.ctypes.data, 2, C.byref(n))
        assert n.value > 2
        assert _fetch(b, k)[0] == _native.RT_E_INVALID and _err(b) == NAME + ": the call fetched last was delivered truncated"
        twin.fetch_records()
        # after rt_extract (on both handles: it moves the look-back)
        spec = np.zeros((S, 4, nperseg), np.float32)
        d = _native.DeviceBuffer(0, spec.nbytes)
        d.upload(spec)
        for x in (b, twin):
            x.native.extract_device(d.ptr, 4, nperseg, None, 0)
            x.fetch_records()
        assert _fetch(b, k)[0] == _native.RT_E_INVALID and "rt_extract" in _err(b)
        d.free()
        # a call without records
        both(np.zeros((S, 4 * nperseg), np.complex64))
        assert len(same()) == 0
        assert _fetch(b, k, 4)[:2] == (_native.RT_OK, 0) and len(b.fetch_record_estimates(hop_div=k)) == 0
        # the feature turned off again
        b.native.set_record_iq(-1)
        twin.native.set_record_iq(-1)
        both(feeds[0])
        same()
        assert _fetch(b, k)[0] == _native.RT_E_INVALID and "rt_set_record_iq" in _err(b)
        for c in (1, 2):
            both(feeds[c])
            same()
    finally:
        for x in (b, twin, d64, off_handle):
            x.close()


def test_the_entry_changes_nothing_else():
    """With the entry never called and with it called after every fetch, in front of everything else: the records, row means,
    record cells, record IQ, the segments' STFT values and the frames are the same bytes."""
    nperseg, fmt, margin = 256, "c64", 2
    sides = {}
    for use in (False, True):
        got = []

        def after(b, c, rec, use=use, got=got):
            if use:
                b.fetch_record_estimates(hop_div=4)
                b.fetch_record_estimates(hop_div=2)
            got.append([rec.tobytes(), b.fetch_row_means().tobytes()] + [a.tobytes() for a in b.fetch_record_cells()] + [a.tobytes() for a in b.fetch_record_iq()]
                       + [a.tobytes() for a in b.fetch_record_stft()] + [a.tobytes() for a in b.fetch_record_stft(hop_div=4)])

        _run(nperseg, fmt, margin, after, row_means=True, record_cells=True)
        sides[use] = got
    assert sides[False] == sides[True] and len(sides[True]) == N_CALLS


def test_a_handle_that_never_calls_the_entry_allocates_what_it_did():
    """Device memory in use once the schedule has run, read from the driver with the handle still open: a handle that never calls
    the entry uses what a second such handle uses, byte for byte; the hop entry adds its pools, and the new entry's rows and plan
    come on top of those only on the handle that calls it (never less; the driver hands memory out in pieces larger than the small
    pools, so more is not required)."""
    import torch

    nperseg, fmt, margin = 256, "c64", 2
    feeds = [torch.from_numpy(rs.gpu_feed(nperseg, c, fmt)).cuda() for c in range(N_CALLS)]

    def used(call):
        torch.cuda.synchronize()
        before = torch.cuda.mem_get_info()[0]
        b = _handle(nperseg, fmt, margin)
        try:
            for x in feeds:
                b.enqueue(x)
                b.fetch_records()
                call(b)
            torch.cuda.synchronize()
            return before - torch.cuda.mem_get_info()[0]
        finally:
            b.close()

    used(lambda b: b.fetch_record_estimates(hop_div=4))  # (what the process itself allocates once is allocated here)
    plain = used(lambda b: None)
    hop_only = used(lambda b: b.fetch_record_stft(hop_div=4))
    with_rows = used(lambda b: b.fetch_record_estimates(hop_div=4))
    again = used(lambda b: None)
    print(f"record_estimates device bytes: never called {plain} / {again}, hop entry {hop_only}, estimates {with_rows}")
    assert plain == again > 0
    assert with_rows >= hop_only >= plain


# ---- the Python layers -----------------------------------------------------------------------------------------------------------------
def test_signal_analyzer_and_replay_leave_the_rows_beside_the_values():
    """``signal_estimates`` lines up with the queued signals and their ``signal_stft``; ``replay(record_estimates=True)`` returns
    one more list, whose rows are those of the per-buffer callbacks but for the edges' origin (a link's own buffer)."""
    import datetime

    nperseg, margin, k = 256, 2, 4
    sched = sq.SCHEDULES["B"]
    n_buf = 5
    B = sched.T[0] * nperseg
    x = np.concatenate([sq.buffer(sched, nperseg, c, 1)[0] for c in range(n_buf)])
    kw = sq.settings(nperseg)
    with pytest.raises(ValueError):
        SignalAnalyzer("0", sdr_callback_length=B, record_estimates=True, **kw)
    a = SignalAnalyzer("0", sdr_callback_length=B, record_iq=True, record_iq_margin=margin, record_estimates=True, stft_hop_div=k, **kw)
    ts0 = datetime.datetime(2024, 1, 1)
    rows = []
    try:
        for c in range(n_buf):
            got = a.analyze_buffer(x[c * B:(c + 1) * B], ts0 + datetime.timedelta(seconds=c * B / sq.FS))
            assert a.signal_estimates.dtype == ESTIMATES_DTYPE and len(a.signal_estimates) == len(a.signal_stft) == len(got)
            for row, values in zip(a.signal_estimates, a.signal_stft):
                assert 0 < row["n_inside"] <= len(values)
            rows.extend(a.signal_estimates)
        with pytest.raises(ValueError):
            a.replay(x, ts0, chain=2, record_estimates=True)
        out, out_iq, out_est = a.replay(x, ts0, chain=2, record_iq=True, stft_hop_div=k, record_estimates=True)
        out4 = a.replay(x, ts0, chain=2, record_iq=True, record_stft=True, stft_hop_div=k, record_estimates=True)
    finally:
        a._batch.close()
        if a._replay_batch is not None:
            a._replay_batch.close()
    assert len(out) == len(out_iq) == len(out_est) == len(rows) > 3 and len(out4) == 4 and len(out4[3]) == len(out4[2]) == len(out)
    for got, want in zip(out_est, rows):
        for f in ("offset_hz", "coherence", "n_pairs", "level", "n_inside", "r", "pair_mag"):
            assert got[f].tobytes() == want[f].tobytes(), f


def test_zz_write_the_worst_ratios():
    """(last in the file: the table of what the tests above saw on this GPU)"""
    assert WORST
    text = ec.format_worst("rt_fetch_record_estimates on the GPU against the model on the same handle's frames", WORST)
    print(text)
    if os.environ.get("RT_WRITE_PROFILES"):
        ec.write_worst("gpu", text)
