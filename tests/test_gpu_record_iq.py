"""The samples behind every record (rt_set_record_iq / rt_fetch_record_iq) on the GPU.  Every comparison is bytes-equal against
slicing the arrays the test fed (tests/record_iq_cases.py: ``KeepEverything``), with ``offsets`` and ``first_seg`` equal to the
model's; and with the feature on, the records, row means and record cells equal those of a twin handle without it, byte for byte."""
import ctypes as C
import datetime

import numpy as np
import pytest

from pyradiotracking_amd import _native, synth
from pyradiotracking_amd.analyze import BatchSignalAnalyzer, SignalAnalyzer
from tests import chain_cases as cc
from tests import present_cases as pc
from tests import record_iq_cases as riq
from tests import sequence_cases as sq

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _need_gpu():
    if _native.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")


class DeviceFed:
    """A BatchSignalAnalyzer fed through raw device pointers: every host array is uploaded ``shift`` bytes past a 16-byte boundary,
    rows ``pad`` samples apart more than their length, and stays in place for the two calls that may be in flight."""

    def __init__(self, b, shift=0, pad=0):
        self.b, self.shift, self.pad, self.ring = b, shift, pad, []

    def __getattr__(self, name):
        return getattr(self.b, name)

    def _put(self, a, fn, per):
        a = np.ascontiguousarray(a)
        S, n = a.shape[0], a.shape[1] // per
        stride = n + self.pad
        img = np.zeros((S, stride * per), a.dtype)
        img[:, :n * per] = a
        d = _native.DeviceBuffer(0, img.nbytes + 16 + self.shift)
        assert d.ptr % 16 == 0
        d.upload(np.concatenate([np.zeros(self.shift, np.uint8), img.view(np.uint8).reshape(-1)]))
        self.ring = (self.ring + [d])[-3:]
        fn(d.ptr + self.shift, n_samples=n, stream_stride=stride)

    def enqueue(self, a):
        self._put(a, self.b.enqueue, 1)

    def enqueue_bytes(self, a):
        self._put(a, self.b.enqueue_bytes, 2)

    def enqueue_int16(self, a):
        self._put(a, self.b.enqueue_int16, 2)

    def enqueue_int8(self, a):
        self._put(a, self.b.enqueue_int8, 2)


def _handle(nperseg, max_samples, fmt, S, margin=None, **extra):
    if fmt.endswith("f64") or fmt == "c128":
        extra["precision"] = "float64"
    kw = sq.case_settings(nperseg, fmt)
    kw.update(extra)
    if margin is not None:
        kw.update(record_iq=True, record_iq_margin=margin)
    return BatchSignalAnalyzer([str(i) for i in range(S)], sdr_callback_length=max_samples, **kw)


def _side(b, rec, cells=True):
    """what the analysis delivered beside the records, as bytes"""
    out = [rec.tobytes(), b.fetch_row_means().tobytes()]
    if cells:
        out += [a.tobytes() for a in b.fetch_record_cells()]
    return out


def _sequence(nperseg, fmt, margin, pipelined, device, name="P", events=(), before_call=None, cells=True, **extra):
    """Schedule ``name`` through a handle with the feature on -- every fetch held to the model -- and through its twin without."""
    sched = sq.SCHEDULES[name]
    S = sq.n_streams(nperseg)
    model = riq.model_run(name, nperseg, fmt, margin, events=events)
    seen = {}
    recs = []
    for on in (True, False):
        b = _handle(nperseg, sq.max_samples(sched, nperseg), fmt, S, margin if on else None, row_means=True, record_cells=cells, **extra)
        fed = DeviceFed(b) if device else b

        def after(k, rec, on=on, b=b):
            side = _side(b, rec, cells)
            if on:
                riq.check_delivery(model[k], rec, b.fetch_record_iq(), f"nperseg {nperseg} {fmt} m {margin} call {k}")
                seen[k] = side
                recs.append(rec)
            else:
                assert side == seen[k], f"call {k}: the analysis differs from the twin's without the feature"

        try:
            sq.run_handle(fed, sched, nperseg, fmt, pipelined=pipelined, before_call=before_call and (lambda k, b=b: before_call(b, k)), after_fetch=after)
        finally:
            b.close()
    return model, recs


@pytest.mark.parametrize("nperseg,fmt,margin,pipelined,device", riq.GPU_SEQUENCES,
                         ids=lambda v: str(v))
def test_sequences(nperseg, fmt, margin, pipelined, device):
    model, recs = _sequence(nperseg, fmt, margin, pipelined, device)
    cov = riq.coverage(model, recs, margin)
    assert cov["back"] > 0 and cov["zero"] > 0 and (not margin or cov["front"] > 0), cov


@pytest.mark.parametrize("fmt,shift,pad", [("u8", 2, 3), ("i8", 2, 0), ("i16", 4, 1), ("c64", 8, 1)])
def test_rows_off_the_16_byte_grid(fmt, shift, pad):
    """A device pointer 2 (4, 8) bytes past a 16-byte boundary and an odd stride: the tails and the gather copy unit by unit."""
    nperseg, margin = 32, 3
    sched = sq.SCHEDULES["P"]
    S = sq.n_streams(nperseg)
    model = riq.model_run("P", nperseg, fmt, margin)
    b = _handle(nperseg, sq.max_samples(sched, nperseg), fmt, S, margin)
    n = []
    try:
        sq.run_handle(DeviceFed(b, shift, pad), sched, nperseg, fmt, pipelined=True,
                      after_fetch=lambda k, rec: n.append(riq.check_delivery(model[k], rec, b.fetch_record_iq(), f"{fmt} call {k}")))
    finally:
        b.close()
    assert sum(n) > 100


def test_a_stream_under_its_noise_and_a_pool_that_grows():
    """One stream finds hundreds of short records anywhere in its buffer (the END of the buffer clips the margin), the others the
    schedule's own, up to 38 segments long; the payload is several times the pool a slot starts with."""
    N, S, m = riq.NOISY_NPERSEG, riq.NOISY_S, riq.NOISY_MARGIN
    sched = sq.SCHEDULES["P"]
    kws = riq.noisy_settings()
    model = riq.noisy_model()
    per = dict(signal_threshold_dbw=[kw.get("signal_threshold_dbw", -90.0) for kw in kws], snr_threshold_db=[kw["snr_threshold_db"] for kw in kws])
    side = {}
    recs = []
    for on in (True, False):
        b = _handle(N, sq.max_samples(sched, N), "c64", S, m if on else None, row_means=True, record_cells=True, **per)
        try:
            b.enqueue(riq.feed("P", N, 0, "c64", S))
            for k in range(riq.NOISY_CALLS):
                if k + 1 < riq.NOISY_CALLS:
                    b.enqueue(riq.feed("P", N, k + 1, "c64", S))
                rec = b.fetch_records()
                if on:
                    got = b.fetch_record_iq()
                    riq.check_delivery(model[k], rec, got, f"call {k}")
                    side[k] = _side(b, rec)
                    recs.append(rec)
                else:
                    assert _side(b, rec) == side[k], k
        finally:
            b.close()
    cov = riq.coverage(model, recs, m)
    assert cov["back"] > 0 and cov["zero"] > 0 and cov["front"] > 0 and cov["tail"] > 0, cov
    quiet = np.concatenate([r[r["stream"] != riq.NOISY_STREAM] for r in recs])
    assert (quiet["end"] - quiet["start"]).max() == 38
    assert max(int(c.expect(r)[0][-1]) for c, r in zip(model, recs)) * 8 > 4 * (1 << 20)
    assert min(int((r["stream"] == riq.NOISY_STREAM).sum()) for r, t in zip(recs, sched.T) if t > 9) > 100


def test_lanes_with_a_last_lane_without_records():
    """Three lanes over five streams (2 + 2 + 1); the last stream is fed silence, so the last lane delivers nothing."""
    nperseg, margin, fmt = 256, 3, "c64"
    sched = sq.SCHEDULES["P"]
    S = sq.n_streams(nperseg)
    feeds = []
    for k in range(4):
        x = riq.feed("P", nperseg, k, fmt, S).copy()
        x[S - 1] = 0
        feeds.append(x)
    m = riq.KeepEverything(S, nperseg, sq.tail_cols(nperseg), margin)
    model = [m.call(x, fmt) for x in feeds]
    side = {}
    for on in (True, False):
        b = _handle(nperseg, sq.max_samples(sched, nperseg), fmt, S, margin if on else None, row_means=True, record_cells=True, lanes=3)
        try:
            b.enqueue(feeds[0])
            for k in range(4):
                if k + 1 < 4:
                    b.enqueue(feeds[k + 1])
                rec = b.fetch_records()
                assert (len(rec) > 0) == (k > 0) and not (rec["stream"] == S - 1).any()  # (the schedule's first call finds nothing)
                if on:
                    riq.check_delivery(model[k], rec, b.fetch_record_iq(), f"lanes call {k}")
                    side[k] = _side(b, rec)
                else:
                    assert _side(b, rec) == side[k], k
        finally:
            b.close()


def test_chained_runs_with_a_suffix_mask_and_a_cut():
    """chain=4: a run's first present link takes its lead from the call before, later links from their predecessor's row of the same
    call; a suffix mask (the run's last links sit a call out) and a cut (rt_reset_stream in front of a later link)."""
    nperseg, margin, links, fmt = 32, 3, 4, "i16"
    name = cc.schedule("P", links)
    sched = sq.SCHEDULES[name]
    S = cc.R * links
    n_calls = len(sched.T) // links
    m = riq.KeepEverything(S, nperseg, sq.tail_cols(nperseg), margin, links=links)
    b = _handle(nperseg, sq.max_samples(sched, nperseg), fmt, S, margin)
    b.native.set_chain(links)
    kinds = set()
    try:
        for c in range(n_calls):
            mask = np.ones(S, bool)
            if c == 2:
                mask[[2, 3, 7]] = False  # run 0 is cut to two links, run 1 to three
            if c == 3:
                b.reset_stream(5)        # a cut in front of run 1's second link
                m.reset_stream(5)
            b.native.set_present(mask)
            m.set_present(mask)
            x = cc.chained_feed(name, nperseg, c, links, fmt)
            call = m.call(x, fmt)
            sq.enqueue(b, x, fmt)
            rec = b.fetch_records()
            riq.check_delivery(call, rec, b.fetch_record_iq(), f"chained call {c}")
            for s in set(rec["stream"][rec["start"] < 0].tolist()):
                kinds.add("call" if s % links == 0 else "link")
            if c == 3:
                assert call.D(5) == 0 and call.D(6) > 0
    finally:
        b.close()
    assert kinds == {"call", "link"}


@pytest.mark.parametrize("pipelined", [False, True], ids=["serial", "pipelined"])
def test_presence_masks_with_gaps(pipelined):
    nperseg, margin, fmt = 32, 3, "u8"
    sched = sq.SCHEDULES["P"]
    S = sq.n_streams(nperseg)
    table = pc.table("P")
    m = riq.KeepEverything(S, nperseg, sq.tail_cols(nperseg), margin)
    model = []
    for k in range(len(sched.T)):
        m.set_present(table[k])
        model.append(m.call(pc.poisoned(sq.buffer(sched, nperseg, k, S, sigma=sq.case_sigma(fmt)), table[k], fmt), "u8"))
    b = _handle(nperseg, sq.max_samples(sched, nperseg), fmt, S, margin)
    across = []
    try:
        def after(k, rec):
            riq.check_delivery(model[k], rec, b.fetch_record_iq(), f"masked call {k}")
            across.extend(int(s) for s in rec["stream"][rec["start"] < 0] if k > 0 and not table[k - 1][s])

        pc.run_handle(b, "P", nperseg, fmt, pipelined=pipelined, after_fetch=after)
    finally:
        b.close()
    assert len(across) > 3  # records whose lead comes from a buffer one to four calls back


def test_clipped_leads():
    """rt_reset_stream, a changed SNR setting and a format change between calls clip the lead (first_seg says so); another margin
    forgets the tails."""
    nperseg, margin = 32, 3
    sched = sq.SCHEDULES["P"]
    S = sq.n_streams(nperseg)
    K = sq.tail_cols(nperseg)
    m = riq.KeepEverything(S, nperseg, K, margin)
    kw = sq.case_settings(nperseg, "i16")
    b = BatchSignalAnalyzer([str(i) for i in range(S)], sdr_callback_length=sq.max_samples(sched, nperseg), record_iq=True, record_iq_margin=margin, **kw)
    fmts = ["i16", "i16", "i16", "i8", "i8", "i16", "i16"]
    clipped, reaching = {}, {}
    try:
        for k, fmt in enumerate(fmts):
            if k == 1:
                b.reset_stream(1)
                m.reset_stream(1)
            if k == 2:
                b.set_stream_settings(snr_threshold_db=[sq.SNR_DB, sq.SNR_DB, sq.SNR_DB + 0.5, sq.SNR_DB, sq.SNR_DB])
                m.reset_stream(2)
            if k == 6:
                b.native.set_record_iq(margin + 1)
                m.set_margin(margin + 1)
            x = riq.feed("P", nperseg, k, fmt, S)
            call = m.call(x, fmt)
            sq.enqueue(b, x, fmt)
            rec = b.fetch_records()
            off, first, _ = got = b.fetch_record_iq()
            riq.check_delivery(call, rec, got, f"call {k} {fmt}")
            clipped[k] = sorted(set(rec["stream"][(rec["start"] < 0) & (first == 0)].tolist()))
            reaching[k] = sorted(set(rec["stream"][rec["start"] < 0].tolist()))
    finally:
        b.close()
    assert all(len(reaching[k]) >= S - 1 for k in range(1, len(fmts)))
    assert clipped[1] == [] and clipped[2] == [] and 1 not in reaching[1] and 2 not in reaching[2]  # (no look-back: no record reaches back)
    assert clipped[3] == reaching[3] and clipped[5] == reaching[5]  # another format: the detection reaches back, the samples do not
    assert clipped[4] == [] and clipped[6] == reaching[6]  # the same format again; another margin: the tails are forgotten


@pytest.mark.parametrize("fmt,kind", [("c128", "dense"), ("u8f64", "dense"), ("c128", "sparse"), ("u8f64", "sparse"), ("c128", "rescue"), ("u8f64", "rescue")])
def test_float64_handles(fmt, kind):
    """Dense, map-free, and map-free with one rescued stream: the bytes are the caller's, the records those of the handle without
    the feature."""
    nperseg, margin = 256, 3
    sched = sq.SCHEDULES["P"]
    S = 3
    extra = {}
    if kind != "dense":
        extra.update(f64_sparse=True)
    if kind == "rescue":
        # stream 1's threshold under its noise: more candidate cells than the smallest list holds
        kws = [sq.case_settings(nperseg, fmt) for _ in range(S)]
        extra.update(f64_rescue=True, hot_capacity=1024, signal_threshold_dbw=[kws[0].get("signal_threshold_dbw", -90.0), -200.0, kws[2].get("signal_threshold_dbw", -90.0)])
    n_calls = 4
    feeds = [riq.feed("P", nperseg, k, fmt, S) for k in range(n_calls)]
    m = riq.KeepEverything(S, nperseg, sq.tail_cols(nperseg), margin)
    model = [m.call(x, riq.base_format(fmt)) for x in feeds]
    seen = {}
    rescued = checked = 0
    for on in (True, False):
        kw = dict(extra)
        b = _handle(nperseg, sq.max_samples(sched, nperseg), fmt, S, margin if on else None, row_means=True, **kw)
        try:
            sq.enqueue(b, feeds[0], fmt)
            for k in range(n_calls):
                if k + 1 < n_calls:
                    sq.enqueue(b, feeds[k + 1], fmt)
                rec = b.fetch_records()
                rescued += b.call_info().n_dense_streams
                side = _side(b, rec, cells=False)
                if on:
                    checked += riq.check_delivery(model[k], rec, b.fetch_record_iq(), f"{fmt} {kind} call {k}")
                    seen[k] = side
                else:
                    assert side == seen[k], k
        finally:
            b.close()
    assert (rescued > 0) == (kind == "rescue") and checked > 20


def test_python_layer_signal_iq_and_replay():
    """``signal_iq`` lines up with the queued signals; ``replay(record_iq=True)`` equals the per-buffer callbacks'."""
    nperseg, margin = 256, 2
    sched = sq.SCHEDULES["B"]
    n_buf = 5
    B = sched.T[0] * nperseg
    x = np.concatenate([sq.buffer(sched, nperseg, k, 1)[0] for k in range(n_buf)])
    kw = sq.settings(nperseg)
    a = SignalAnalyzer("0", sdr_callback_length=B, record_iq=True, record_iq_margin=margin, **kw)
    ts0 = datetime.datetime(2024, 1, 1)
    sigs, iqs = [], []
    try:
        for k in range(n_buf):
            buf = x[k * B:(k + 1) * B]
            got = a.analyze_buffer(buf, ts0 + datetime.timedelta(seconds=k * B / sq.FS))
            assert len(a.signal_iq) == len(got)
            sigs.extend(got)
            iqs.extend(a.signal_iq)
            for s, q in zip(got, a.signal_iq):
                assert q.dtype == np.complex64 and len(q) % nperseg == 0 and len(q) >= nperseg * 3
        out, out_iq = a.replay(x, ts0, chain=2, record_iq=True)
    finally:
        a._batch.close()
        if a._replay_batch is not None:
            a._replay_batch.close()
    assert len(out) == len(sigs) > 3 and len(out_iq) == len(iqs) == len(sigs)
    for p, q in zip(out_iq, iqs):
        assert np.array_equal(riq.raw(p), riq.raw(q))
    # every snippet is a slice of the recording's whole segments (a record's samples are contiguous here: no ragged remainder)
    flat = x.view(np.uint8).tobytes()
    for q in iqs:
        at = flat.find(riq.raw(q).tobytes())
        assert at >= 0 and at % (8 * nperseg) == 0


def test_convert_gives_the_kernels_samples():
    nperseg, fmt = 32, "u8"
    sched = sq.SCHEDULES["P"]
    S = sq.n_streams(nperseg)
    b = _handle(nperseg, sq.max_samples(sched, nperseg), fmt, S, 0)
    try:
        sq.enqueue(b, riq.feed("P", nperseg, 0, fmt, S), fmt)
        rec = b.fetch_records()
        off, first, raw8 = b.fetch_record_iq()
        off2, first2, conv = b.fetch_record_iq(convert=True)
    finally:
        b.close()
    assert len(rec) and raw8.dtype == np.uint8 and raw8.shape == (off[-1], 2) and conv.dtype == np.complex64
    assert np.array_equal(off, off2) and np.array_equal(conv, synth.u8_to_complex64_like_kernel(raw8.reshape(-1)))


def _fetch_iq(b, n_rec, cap=None):
    lib, h = b.native._lib, b.native._handle
    off = np.zeros(n_rec + 1, np.int64)
    first = np.zeros(n_rec, np.int32)
    n, bps = C.c_size_t(0), C.c_int32(0)
    rc = lib.rt_fetch_record_iq(h, off.ctypes.data, off.size, first.ctypes.data, first.size, None, 0, C.byref(n), C.byref(bps))
    if rc != _native.RT_OK or cap is None:
        return rc, n.value, None
    buf = np.full(max(cap, 1), 0xA5, np.uint8)
    rc = lib.rt_fetch_record_iq(h, off.ctypes.data, off.size, first.ctypes.data, first.size, buf.ctypes.data, cap, C.byref(n), C.byref(bps))
    return rc, n.value, buf


def test_refusals_and_the_size_query():
    nperseg, fmt = 32, "c64"
    sched = sq.SCHEDULES["P"]
    S = sq.n_streams(nperseg)
    feeds = [riq.feed("P", nperseg, k, fmt, S) for k in range(4)]
    off_handle = _handle(nperseg, sq.max_samples(sched, nperseg), fmt, S, None)
    b = _handle(nperseg, sq.max_samples(sched, nperseg), fmt, S, 0)
    lib = b.native._lib
    try:
        # feature off
        off_handle.enqueue(feeds[0])
        rec = off_handle.fetch_records()
        with pytest.raises(_native.NativeError) as ei:
            off_handle.fetch_record_iq()
        assert ei.value.code == _native.RT_E_INVALID and "rt_set_record_iq" in str(ei.value)
        # no delivered call yet; pending calls refuse the setter
        assert _fetch_iq(b, 0)[0] == _native.RT_E_INVALID
        b.enqueue(feeds[0])
        assert len(b.fetch_records()) == 0  # (the schedule's first call finds nothing: it gives the second its look-back)
        b.enqueue(feeds[1])
        with pytest.raises(_native.NativeError) as ei:
            b.native.set_record_iq(2)
        assert ei.value.code == _native.RT_E_INVALID and "pending" in str(ei.value)
        assert lib.rt_set_record_iq(b.native._handle, 1025) == _native.RT_E_INVALID
        rec = b.fetch_records()
        n_rec = len(rec)
        # size query, then fetch; cap one short; wrong counts
        rc, n_bytes, _ = _fetch_iq(b, n_rec)
        assert rc == _native.RT_OK and n_bytes > 0
        rc, _, buf = _fetch_iq(b, n_rec, n_bytes - 1)
        assert rc == _native.RT_E_CAPACITY and np.all(buf == 0xA5)
        assert _fetch_iq(b, n_rec + 1)[0] == _native.RT_E_INVALID
        rc, n2, buf = _fetch_iq(b, n_rec, n_bytes)
        assert rc == _native.RT_OK and n2 == n_bytes
        m = riq.KeepEverything(S, nperseg, sq.tail_cols(nperseg), 0)
        m.call(feeds[0], fmt)
        want = m.call(feeds[1], fmt).expect(rec)
        assert np.array_equal(buf, np.concatenate([riq.raw(p) for p in want[2]]))
        # after the next enqueue; with two in flight: process k, process k + 1, fetch k, then the IQ of k
        b.enqueue(feeds[2])
        assert _fetch_iq(b, n_rec)[0] == _native.RT_E_INVALID
        b.enqueue(feeds[3])
        rec = b.fetch_records()
        assert _fetch_iq(b, len(rec))[0] == _native.RT_OK
        # a truncated delivery
        n = C.c_size_t(0)
        out = np.zeros(2, _native.RECORD_DTYPE)
        rc = lib.rt_fetch(b.native._handle, out.ctypes.data, 2, C.byref(n))
        assert n.value > 2
        assert _fetch_iq(b, 2)[0] == _native.RT_E_INVALID and "truncated" in lib.rt_last_error(b.native._handle).decode()
        # after rt_extract
        spec = np.zeros((S, 4, nperseg), np.float32)
        d = _native.DeviceBuffer(0, spec.nbytes)
        d.upload(spec)
        b.native.extract_device(d.ptr, 4, nperseg, None, 0)
        b.fetch_records()
        assert _fetch_iq(b, 0)[0] == _native.RT_E_INVALID and "rt_extract" in lib.rt_last_error(b.native._handle).decode()
        d.free()
        # a call without records
        b.enqueue(np.zeros((S, 4 * nperseg), np.complex64))
        assert len(b.fetch_records()) == 0
        rc, n_bytes, _ = _fetch_iq(b, 0)
        assert rc == _native.RT_OK and n_bytes == 0
    finally:
        b.close()
        off_handle.close()
