"""8-bit signed IQ (CS8: rt_process_i8 / rt_process_i8_host, enqueue_int8, process_int8) on the GPU.

Two yardsticks throughout (inputs and references: tests/int8_cases.py):
(a) the int8 handle delivers, as bytes, the records, row means and record cells of an identically configured handle fed the
    exact conversion (synth.i8_to_complex64 / i8_to_complex128) through ``enqueue`` -- int8 -> float and the multiplication
    by 2^-7 are exact, so there is no tolerance;
(b) against oracle.OracleAnalyzer on that complex64: the same (fi, start, end) lists and shadow verdicts, the five dB figures
    within POWER_TOL_DB, the tolerance tests/test_gpu_parity.py holds the complex64 and uint8 paths to.  Every such comparison
    first asserts that its reference has a record in every stream and buffer and, in buffer 1, one that starts in buffer 0."""
import datetime
import multiprocessing

import numpy as np
import pytest

from oracle import analyze_oracle as oracle
from pyradiotracking_amd import Signal, StateMessage, _native, synth
from pyradiotracking_amd.analyze import BatchSignalAnalyzer, SignalAnalyzer
from tests import float64_cases as fc
from tests import int8_cases as ic

pytestmark = pytest.mark.gpu

POWER_TOL_DB = 0.01  # tests/test_gpu_parity.py: POWER_TOL_DB
F64_DB_TOL = 1e-9    # tests/test_gpu_float64_path.py: DB_TOL (max / avg / noise / snr, dB)
F64_STD_TOL = 1e-5   # tests/test_gpu_float64_path.py: STD_TOL


@pytest.fixture(autouse=True)
def _need_gpu():
    if _native.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")


def _batch(kw, mode, n_streams=ic.N_STREAMS, blen=ic.BLEN, **extra):
    extra.setdefault("row_means", True)
    extra.setdefault("record_cells", True)
    return BatchSignalAnalyzer([str(i) for i in range(n_streams)], sdr_callback_length=blen, mode=mode, **kw, **extra)


def _fetch_all(b):
    """(records, row means, cell offsets, cells) of the oldest call."""
    rec = b.fetch_records()
    means = b.fetch_row_means()
    offsets, cells = b.fetch_record_cells()
    return rec, means, offsets, cells


def _assert_same(got, want, what=""):
    """(a): byte for byte."""
    for name, g, w in zip(("records", "row means", "cell offsets", "cells"), got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what} {name}: {g.dtype}{g.shape} vs {w.dtype}{w.shape}"
        assert g.tobytes() == w.tobytes(), f"{what} {name} differ"


def _assert_oracle(b, rec, ref_k, what=""):
    """(b): ``ref_k`` = [stream] -> (oracle signals, shadowed flags) of this buffer.  Returns the number of records."""
    n_streams = len(ref_k)
    for s, (want, shadowed) in enumerate(ref_k):
        mine = rec[rec["stream"] == s]
        assert [(int(r["fi"]), int(r["start"]), int(r["end"])) for r in mine] == [(x.fi, x.start, x.end) for x in want], f"{what} stream {s}"
        assert [bool(r["shadowed"]) for r in mine] == shadowed, f"{what} stream {s}: shadow verdicts"
        sigs = b._decoder.signals(mine, [str(s)] * n_streams, [ic.TS0] * n_streams)
        for g, x in zip(sigs, want):
            for name in ("max", "avg", "noise", "snr", "std"):
                d = abs(getattr(g, name) - getattr(x, name))
                assert d < POWER_TOL_DB, f"{what} stream {s} {name}: {getattr(g, name)} vs {getattr(x, name)}"
    return len(rec)


def _twins(raw_all, kw, mode, oracle_ref=None, n_buf=ic.N_BUF, blen=ic.BLEN, what="", i8_extra=None, **extra):
    """Feed the consecutive buffers to an int8 handle and to its complex64 twin; (a) per buffer, (b) where a reference is given.
    Returns (total records, [call_info of the int8 handle], [call_info of the twin])."""
    n_streams = raw_all.shape[0]
    bi = _batch(kw, mode, n_streams, blen, **dict(extra, **(i8_extra or {})))
    bc = _batch(kw, mode, n_streams, blen, **extra)
    total, infos_i, infos_c = 0, [], []
    try:
        for k in range(n_buf):
            raw = ic.buffer_of(raw_all, k, blen)
            bi.enqueue_int8(raw)
            got = _fetch_all(bi)
            infos_i.append(bi.call_info())
            bc.enqueue(synth.i8_to_complex64(raw))
            want = _fetch_all(bc)
            infos_c.append(bc.call_info())
            _assert_same(got, want, f"{what} buffer {k}:")
            if oracle_ref is not None:
                if k == 0:
                    ic.assert_not_empty(oracle_ref)
                _assert_oracle(bi, got[0], oracle_ref[k], f"{what} buffer {k}:")
            total += len(got[0])
    finally:
        bi.close()
        bc.close()
    return total, infos_i, infos_c


# nperseg 32 / 64 / 128: lane groups of 2 / 4 / 8 (load_iq_run); 256, 1024: stft_scan; 4096: stft_scan64 (LDS-DMA prefetch);
# 8192, 16384: stft_wg; 16: stft_general; 300: stft_bluestein
FAMILIES = [(32, "hamming"), (64, "hann"), (128, "hamming"), (256, "hamming"), (1024, "hann"), (4096, "hamming"), (8192, "hamming"),
            (16384, "hamming"), (16, "hamming"), (300, "hann")]


@pytest.mark.parametrize("nperseg,window", FAMILIES)
def test_every_transform_family(nperseg, window):
    """Two consecutive buffers (the look-back tail is written from int8 loads and read back): (a) and (b)."""
    fused = nperseg >= 32 and (nperseg & (nperseg - 1)) == 0
    total, _, _ = _twins(ic.wire(nperseg, window), ic.kwargs(nperseg, window), "sparse" if fused else "dense",
                         ic.wire_oracle(nperseg, window), what=f"nperseg {nperseg}")
    assert total > 20


@pytest.mark.parametrize("mode,variant", [("sparse", "quiet"), ("dense", "near"), ("prefilter", "near"), ("runfilter", "near"), ("auto", "near"),
                                          ("auto", "mixed")])
def test_every_mode_at_nperseg_256(mode, variant):
    """The variants of int8_cases: RT_MODE_SPARSE on clean input; the other modes under a threshold 2 dB over the noise floor, where
    the sparse lists overflow -- AUTO leaves the sparse level and analyses the call again, from its int8 samples --; and AUTO on a
    batch in which one stream's floor lies over the threshold: that stream alone is re-run dense, from a stream list."""
    total, infos_i, infos_c = _twins(ic.modes_wire(variant), ic.modes_kwargs(variant), mode, ic.modes_oracle(variant), n_buf=ic.M_BUF,
                                     blen=ic.M_BLEN, what=f"{mode} {variant}", segs_per_chunk=4, record_capacity=2048)
    assert total > 2 * ic.M_STREAMS
    for k, (a, b) in enumerate(zip(infos_i, infos_c)):
        assert (a.mode_used, a.fell_back, a.n_dense_streams) == (b.mode_used, b.fell_back, b.n_dense_streams), (mode, variant, k)
    first = infos_i[0]
    if variant == "mixed":
        assert first.fell_back == 1 and first.n_dense_streams == 1, (first.mode_used, first.n_dense_streams)
    elif mode == "auto":
        assert first.fell_back == 1 and first.mode_used != _native.RT_MODE_SPARSE, first.mode_used  # (the sparse lists overflow)
    elif mode != "dense":
        assert first.mode_used == {"sparse": _native.RT_MODE_SPARSE, "prefilter": _native.RT_MODE_PREFILTER,
                                   "runfilter": _native.RT_MODE_RUNFILTER}[mode]


def _all_pairs(seed):
    """65 536 samples that hold every (I, Q) byte pair once, in a seeded permutation: int8 [2 * 65 536]."""
    p = np.random.default_rng(seed).permutation(65536)
    out = np.empty(2 * 65536, dtype=np.int8)
    out[0::2] = ((p >> 8) - 128).astype(np.int8)
    out[1::2] = ((p & 255) - 128).astype(np.int8)
    return out


def test_all_65536_byte_pairs():
    """One buffer of 256 segments of 256 per stream, every (I, Q) pair once: a wrong sign extension or a swapped byte on any value
    changes a row mean.  Dense; a threshold at the level of this white input and runs of 0.3 .. 5 ms (3 to 40 segments) so that
    there are records as well (the oracle finds 97 and 71)."""
    raw = np.stack([_all_pairs(8001), _all_pairs(8002)])
    for r in raw:
        assert np.array_equal(np.unique(r.view(np.uint16)), np.arange(65536))
    kw = dict(ic.kwargs(256, "hamming", -60.0), signal_min_duration_ms=0.3, signal_max_duration_ms=5.0)
    want_n = [len(w) for w, _ in ic.oracle_buffers([synth.i8_to_complex64(raw)], kw)[0]]
    bi = _batch(kw, "dense", 2, 65536)
    bc = _batch(kw, "dense", 2, 65536)
    try:
        bi.enqueue_int8(raw)
        got = _fetch_all(bi)
        bc.enqueue(synth.i8_to_complex64(raw))
        _assert_same(got, _fetch_all(bc), "all pairs:")
        assert np.isfinite(got[1]).all() and (got[1] > 0).all()
        assert [int((got[0]["stream"] == s).sum()) for s in range(2)] == want_n and min(want_n) > 50
    finally:
        bi.close()
        bc.close()


@pytest.mark.parametrize("nperseg,gain", [(256, 30.0), (4096, 60.0)])
def test_full_scale_and_signs(nperseg, gain):
    """The noise alone reaches both rails on I and on Q, and in every buffer twelve segments of 4096 (192 of 256) are pinned to
    (127, 127), (-128, -128) and (127, -128) in streams 0, 1 and 2: whole segments clip to a constant, the guard of the detrend by
    linearity marks the streams and their calls are analysed again by the subtract-first kernels, from the int8 samples."""
    raw = ic.rails(nperseg, gain)
    a = 2 * ic.RAIL_FIRST
    for s in range(ic.N_STREAMS):
        for comp in (raw[s, 0::2], raw[s, 1::2]):
            assert (comp == -128).sum() > 30000 and (comp == 127).sum() > 30000  # (outside the pinned stretch as well)
        pinned = raw[s, a: a + 2 * ic.RAIL_SEGS * 4096].reshape(-1, 2)
        want = [127 if r > 0 else -128 for r in ic.RAILS[s]]
        assert (pinned == want).all()
    kw = ic.kwargs(nperseg, "hamming", -50.0)
    total, _, _ = _twins(raw, kw, "sparse", ic.rails_oracle(nperseg, gain, -50.0), what=f"nperseg {nperseg} gain {gain}")
    assert total > 20
    # the witness of the guard: every stream is marked in its first buffer, so the default handle's results are those of a handle
    # that was subtract-first from the start (the same kernels on the same samples) -- which the linearity form's are not
    runs = []
    for extra in (dict(), dict(subtract_first=True)):
        b = _batch(kw, "sparse", **extra)
        out = []
        for k in range(ic.N_BUF):
            b.enqueue_int8(ic.buffer_of(raw, k))
            out.append(_fetch_all(b))
        b.close()
        runs.append(out)
    for k in range(ic.N_BUF):
        _assert_same(runs[0][k], runs[1][k], f"guarded against subtract-first, buffer {k}:")


def test_reanalysis_inside_the_fetch_reads_int8():
    """record_capacity=4: stream 0 finds more, rt_fetch grows the capacity and analyses the call again from its int8 samples."""
    raw = ic.wire(256, "hamming")
    assert len(ic.wire_oracle(256, "hamming")[0][0][0]) > 4
    total, _, _ = _twins(raw, ic.kwargs(256, "hamming"), "sparse", what="capacity 4", record_capacity=4)
    assert total > 20


@pytest.mark.parametrize("nperseg,window", [(256, "hamming"), (1024, "hann")])
def test_two_lanes_equal_the_one_lane_complex64_handle(nperseg, window):
    total, _, _ = _twins(ic.wire(nperseg, window), ic.kwargs(nperseg, window), "sparse", what=f"lanes 2 nperseg {nperseg}",
                         i8_extra=dict(lanes=2))
    assert total > 20


def _strided(raw, stride_samples, byte_offset):
    """A host image of [S, 2 * B] int8 laid out with ``stride_samples`` between the streams, ``byte_offset`` bytes into a buffer
    whose start is 16-byte aligned on the device.  (bytes, n_samples)"""
    n_streams, n = raw.shape[0], raw.shape[1] // 2
    img = np.zeros(byte_offset + 2 * stride_samples * n_streams + 16, dtype=np.uint8)
    for s in range(n_streams):
        at = byte_offset + 2 * stride_samples * s
        img[at: at + 2 * n] = raw[s].view(np.uint8)
    return img, n


@pytest.mark.parametrize("nperseg", [32, 64, 128, 256])
def test_device_pointers_strides_and_alignment(nperseg):
    """stream_stride = n_samples + 3 (rows 6 bytes past a multiple of 16) at byte offsets 0, 2 and 6 from a 16-byte boundary: the
    records of the complex64 twin.  Odd byte offsets are refused before anything is launched: the next call on that handle is
    unharmed."""
    window = "hamming"
    kw = ic.kwargs(nperseg, window)
    raw = ic.buffer_of(ic.wire(256, "hamming"), 0)  # (one recipe for the four sizes)
    n = raw.shape[1] // 2
    assert (2 * (n + 3)) % 16 != 0
    ref = _batch(kw, "sparse")
    ref.enqueue(synth.i8_to_complex64(raw))
    want = _fetch_all(ref)
    ref.close()
    assert len(want[0]) > 10
    for off in (0, 2, 6):
        img, _ = _strided(raw, n + 3, off)
        d = _native.DeviceBuffer(0, img.nbytes)
        assert d.ptr % 16 == 0
        d.upload(img)
        b = _batch(kw, "sparse")
        b.enqueue_int8(d.ptr + off, n_samples=n, stream_stride=n + 3)
        _assert_same(_fetch_all(b), want, f"nperseg {nperseg} offset {off}:")
        b.close()
        d.free()
    img, _ = _strided(raw, n + 3, 0)
    d = _native.DeviceBuffer(0, img.nbytes)
    d.upload(img)
    b = _batch(kw, "sparse")
    for off in (1, 3, 7):
        with pytest.raises(_native.NativeError) as ei:
            b.enqueue_int8(d.ptr + off, n_samples=n, stream_stride=n + 3)
        assert ei.value.code == _native.RT_E_INVALID and "aligned" in str(ei.value)
    b.enqueue_int8(d.ptr, n_samples=n, stream_stride=n + 3)
    _assert_same(_fetch_all(b), want, f"nperseg {nperseg} after the refusals:")
    b.close()
    d.free()


@pytest.mark.parametrize("precision", ["float32", "float64"])
def test_odd_pointer_is_refused_on_either_precision(precision):
    kw = ic.kwargs(256, "hamming")
    d = _native.DeviceBuffer(0, 4 * 4096 * ic.N_STREAMS + 16)
    b = _batch(kw, "dense", precision=precision)
    try:
        with pytest.raises(_native.NativeError) as ei:
            b.enqueue_int8(d.ptr + 1, n_samples=4096, stream_stride=4096)
        assert ei.value.code == _native.RT_E_INVALID and "aligned" in str(ei.value)
    finally:
        b.close()
        d.free()


def test_host_entry_with_two_calls_in_flight():
    """Host arrays of different lengths, call k + 1 enqueued before call k is fetched, the caller's array overwritten as soon as
    enqueue_int8 returns: the staging copy is what is analysed, and the records are the serial ones."""
    raw_all = ic.wire(256, "hamming")
    kw = ic.kwargs(256, "hamming")
    lens = (ic.BLEN, ic.BLEN - 5000, ic.BLEN - 77)
    starts = (0, ic.BLEN, 2 * ic.BLEN - lens[2])
    bufs = [np.ascontiguousarray(raw_all[:, 2 * a: 2 * (a + n)]) for a, n in zip(starts, lens)]
    serial = _batch(kw, "sparse", row_means=False, record_cells=False)
    want = []
    for x in bufs:
        serial.enqueue_int8(x)
        want.append(serial.fetch_records())
    serial.close()
    assert sum(len(w) for w in want) > 20

    def enqueue_and_overwrite(b, x):
        mine = x.copy()
        b.enqueue_int8(mine)
        mine[:] = 123

    piped = _batch(kw, "sparse", row_means=False, record_cells=False)
    got = []
    enqueue_and_overwrite(piped, bufs[0])
    for k in range(len(bufs)):
        if k + 1 < len(bufs):
            enqueue_and_overwrite(piped, bufs[k + 1])
        got.append(piped.fetch_records())
    piped.close()
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.tobytes() == w.tobytes(), f"buffer {k}"


def _assert_f64_oracle(rec, want):
    """rt_record_f64 rows of one stream against oracle records on complex128, as tests/test_gpu_float64_path.py: _check."""
    sig = oracle.records_to_signals(want, np.zeros(4096), fc.TS0, "0", 0.0)
    kept = {(s.fi, s.start) for s in oracle.filter_shadows(sig)}
    assert [(int(r["fi"]), int(r["start"]), int(r["end"])) for r in rec] == fc.key(want)
    assert [int(r["shadowed"]) for r in rec] == [0 if (w.fi, w.start) in kept else 1 for w in want]
    if not len(want):
        return
    np.testing.assert_allclose(oracle.to_db(rec["max_p"]), [w.max_dbw for w in want], rtol=0, atol=F64_DB_TOL)
    np.testing.assert_allclose(oracle.to_db(rec["mean_p"]), [w.avg_dbw for w in want], rtol=0, atol=F64_DB_TOL)
    np.testing.assert_allclose(oracle.to_db(rec["row_mean"]), [w.noise_dbw for w in want], rtol=0, atol=F64_DB_TOL)
    np.testing.assert_allclose(oracle.to_db(rec["mean_p"] / rec["row_mean"]), [w.snr_db for w in want], rtol=0, atol=F64_DB_TOL)
    np.testing.assert_allclose(rec["std_db"], [w.std_db for w in want], rtol=0, atol=F64_STD_TOL)


@pytest.mark.parametrize("nperseg,window", [(256, "hamming"), (300, "hann")])
def test_float64_handles(nperseg, window):
    """precision="float64": int8 pairs are (double)i * 2^-7 -- the handle fed i8_to_complex128, byte for byte, and the float64
    oracle on that complex128 within the bounds the float64 path is held to."""
    raw_all = ic.wire(nperseg, window)
    kw = ic.kwargs(nperseg, window)
    bi = _batch(kw, "dense", precision="float64")
    bc = _batch(kw, "dense", precision="float64")
    last = [None] * ic.N_STREAMS
    total = 0
    for k in range(ic.N_BUF):
        raw = ic.buffer_of(raw_all, k)
        c128 = synth.i8_to_complex128(raw)
        bi.enqueue_int8(raw)
        got = _fetch_all(bi)
        bc.enqueue(c128)
        _assert_same(got, _fetch_all(bc), f"float64 nperseg {nperseg} buffer {k}:")
        assert got[0].dtype == _native.RECORD_F64_DTYPE
        for s in range(ic.N_STREAMS):
            want, spec = fc.oracle_records(c128[s], nperseg, window, ic.FS, last=last[s], signal_threshold_dbw=-80.0)
            last[s] = spec
            _assert_f64_oracle(got[0][got[0]["stream"] == s], want)
        total += len(got[0])
    bi.close()
    bc.close()
    assert total > 20


def test_absent_stream_under_set_present():
    """Calls 0 .. 2 = buffer 0, buffer 1 with stream 1 absent, buffer 1 with every stream: the int8 handle's row of the absent stream
    is poisoned (rail to rail) while the twin's holds the samples, so equal results say that the row was not read; stream 1's
    records of call 2 look back into buffer 0 on both handles."""
    raw_all = ic.wire(256, "hamming")
    kw = ic.kwargs(256, "hamming")
    bi = _batch(kw, "sparse")
    bc = _batch(kw, "sparse")
    masks = (None, (True, False, True), None)
    total = back = 0
    try:
        for k, (buf, mask) in enumerate(zip((0, 1, 1), masks)):
            raw = ic.buffer_of(raw_all, buf)
            c64 = synth.i8_to_complex64(raw)
            if mask is not None:
                raw[1, 0::3] = 127
                raw[1, 1::3] = -128
            bi.set_present(mask)
            bc.set_present(mask)
            bi.enqueue_int8(raw)
            got = _fetch_all(bi)
            bc.enqueue(c64)
            _assert_same(got, _fetch_all(bc), f"call {k}:")
            mine = got[0][got[0]["stream"] == 1]
            if mask is not None:
                assert len(mine) == 0 and np.isnan(got[1][1]).all()
            elif k == 2:
                back = int((mine["start"] < 0).sum())
            total += len(got[0])
    finally:
        bi.close()
        bc.close()
    assert total > 40 and back >= 1


class _Q:
    def __init__(self):
        self.items = []

    def put(self, x):
        self.items.append(x)


def test_signal_analyzer_process_int8_is_process_samples_on_the_conversion():
    raw_all = ic.wire(256, "hamming")
    kw = ic.kwargs(256, "hamming")
    t0 = datetime.datetime.now()  # (one start for both analyzers' running clocks: the buffers' timestamps are then the same)
    runs = []
    for feed in ("int8", "complex64"):
        q, beat = _Q(), multiprocessing.Value("d", 0.0)
        an = SignalAnalyzer("0", signal_queue=q, last_data_ts=beat, state_update_s=60, sdr_callback_length=ic.BLEN, **kw)
        an._ts = t0
        clocks = []
        for k in range(ic.N_BUF):
            raw = ic.buffer_of(raw_all, k)[0]
            if feed == "int8":
                assert an.process_int8(raw, None) is None
            else:
                assert an.process_samples(synth.i8_to_complex64(raw), None) is None
            clocks.append(an._ts)
            assert beat.value > 0
        runs.append((q.items, clocks))
        an._batch.close()
    (items_i, clocks_i), (items_c, clocks_c) = runs
    assert clocks_i == clocks_c and clocks_i[1] - clocks_i[0] == clocks_i[0] - t0 > t0 - t0
    assert [type(x) for x in items_i] == [type(x) for x in items_c]
    assert [x.state for x in items_i if isinstance(x, StateMessage)] == [x.state for x in items_c if isinstance(x, StateMessage)]
    sig_i = [x for x in items_i if isinstance(x, Signal)]
    sig_c = [x for x in items_c if isinstance(x, Signal)]
    kept = sum(flags.count(False) for flags in (ic.wire_oracle(256, "hamming")[k][0][1] for k in range(ic.N_BUF)))  # the oracle's, stream 0
    assert len(sig_i) == len(sig_c) == kept > 0
    for a, b in zip(sig_i, sig_c):
        for name in ("device", "ts", "frequency", "duration", "max", "avg", "std", "noise", "snr"):
            ga, gb = getattr(a, name), getattr(b, name)
            assert ga == gb or (isinstance(ga, float) and np.isnan(ga) and np.isnan(gb)), (name, ga, gb)
