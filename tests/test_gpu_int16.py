"""16-bit signed IQ (CS16: rt_process_i16 / rt_process_i16_host, enqueue_int16, process_int16) on the GPU.

Two yardsticks throughout (inputs and references: tests/int16_cases.py):
(a) the int16 handle delivers, as bytes, the records, row means and record cells of an identically configured handle fed the
    exact conversion (synth.i16_to_complex64 / i16_to_complex128) through ``enqueue`` -- int16 -> float and the multiplication
    by 2^-15 are exact, so there is no tolerance;
(b) against oracle.OracleAnalyzer on that complex64: the same (fi, start, end) lists and shadow verdicts, the five dB figures
    within POWER_TOL_DB, the tolerance tests/test_gpu_parity.py holds the complex64 and uint8 paths to."""
import datetime
import multiprocessing

import numpy as np
import pytest

from oracle import analyze_oracle as oracle
from pyradiotracking_amd import Signal, StateMessage, _native, synth
from pyradiotracking_amd.analyze import BatchSignalAnalyzer, SignalAnalyzer
from tests import float64_cases as fc
from tests import int16_cases as ic

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


def _twins(raw_all, kw, mode, oracle_ref=None, n_buf=ic.N_BUF, blen=ic.BLEN, what="", i16_extra=None, **extra):
    """Feed the consecutive buffers to an int16 handle and to its complex64 twin; (a) per buffer, (b) where a reference is given.
    Returns (total records, [call_info of the int16 handle], [call_info of the twin])."""
    n_streams = raw_all.shape[0]
    bi = _batch(kw, mode, n_streams, blen, **dict(extra, **(i16_extra or {})))
    bc = _batch(kw, mode, n_streams, blen, **extra)
    total, infos_i, infos_c = 0, [], []
    try:
        for k in range(n_buf):
            raw = ic.buffer_of(raw_all, k, blen)
            bi.enqueue_int16(raw)
            got = _fetch_all(bi)
            infos_i.append(bi.call_info())
            bc.enqueue(synth.i16_to_complex64(raw))
            want = _fetch_all(bc)
            infos_c.append(bc.call_info())
            _assert_same(got, want, f"{what} buffer {k}:")
            if oracle_ref is not None:
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
    """Two consecutive buffers (the look-back tail is written from int16 loads and read back): (a) and (b)."""
    fused = nperseg >= 32 and (nperseg & (nperseg - 1)) == 0
    total, _, _ = _twins(ic.wire(nperseg, window), ic.kwargs(nperseg, window), "sparse" if fused else "dense",
                         ic.wire_oracle(nperseg, window), what=f"nperseg {nperseg}")
    assert total > 20


@pytest.mark.parametrize("mode,variant", [("sparse", "quiet"), ("dense", "near"), ("prefilter", "near"), ("runfilter", "near"), ("auto", "near"),
                                          ("auto", "mixed")])
def test_every_mode_at_nperseg_256(mode, variant):
    """The variants of int16_cases: RT_MODE_SPARSE on clean input; the other modes under a threshold 2 dB over the noise floor, where
    the sparse lists overflow -- AUTO leaves the sparse level and analyses the call again, from its int16 samples --; and AUTO on a
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


@pytest.mark.parametrize("nperseg,gain", [(256, 30.0), (4096, 60.0)])
def test_full_scale_and_signs(nperseg, gain):
    """The noise alone clips: hundreds of thousands of samples per stream at -32768 and at 32767, on I and on Q."""
    raw = ic.wire(nperseg, "hamming", 77, gain)
    for s in range(ic.N_STREAMS):
        for comp in (raw[s, 0::2], raw[s, 1::2]):
            assert (comp == -32768).sum() > 50000 and (comp == 32767).sum() > 50000
        assert (raw[s] == -32768).sum() > 200000 and (raw[s] == 32767).sum() > 200000
    total, _, _ = _twins(raw, ic.kwargs(nperseg, "hamming", -50.0), "sparse", ic.wire_oracle(nperseg, "hamming", 77, gain, -50.0),
                         what=f"nperseg {nperseg} gain {gain}")
    assert total > 20


def test_reanalysis_inside_the_fetch_reads_int16():
    """record_capacity=4: stream 0 finds more, rt_fetch grows the capacity and analyses the call again from its int16 samples."""
    raw = ic.wire(256, "hamming")
    assert len(ic.wire_oracle(256, "hamming")[0][0][0]) > 4
    total, _, _ = _twins(raw, ic.kwargs(256, "hamming"), "sparse", what="capacity 4", record_capacity=4)
    assert total > 20


@pytest.mark.parametrize("nperseg,window", [(256, "hamming"), (1024, "hann")])
def test_two_lanes_equal_the_one_lane_complex64_handle(nperseg, window):
    total, _, _ = _twins(ic.wire(nperseg, window), ic.kwargs(nperseg, window), "sparse", what=f"lanes 2 nperseg {nperseg}",
                         i16_extra=dict(lanes=2))
    assert total > 20


def _strided(raw, stride_samples, byte_offset):
    """A host image of [S, 2 * B] int16 laid out with ``stride_samples`` between the streams, ``byte_offset`` bytes into a buffer
    whose start is 16-byte aligned on the device.  (bytes, n_samples)"""
    n_streams, n = raw.shape[0], raw.shape[1] // 2
    img = np.zeros(byte_offset + 4 * stride_samples * n_streams + 16, dtype=np.uint8)
    for s in range(n_streams):
        at = byte_offset + 4 * stride_samples * s
        img[at: at + 4 * n] = raw[s].view(np.uint8)
    return img, n


@pytest.mark.parametrize("nperseg", [32, 64, 128, 256])
def test_device_pointers_strides_and_alignment(nperseg):
    """stream_stride = n_samples + 3 at byte offsets 0, 4 and 12 from a 16-byte boundary: the records of the aligned upload.  Byte
    offsets 1, 2 and 3 are refused before anything is launched: the next call on that handle is unharmed."""
    window = "hamming"
    kw = ic.kwargs(nperseg, window)
    raw = ic.buffer_of(ic.wire(256, "hamming"), 0)  # (one recipe for the four sizes)
    n = raw.shape[1] // 2
    ref = _batch(kw, "sparse")
    ref.enqueue_int16(raw)
    want = _fetch_all(ref)
    ref.close()
    assert len(want[0]) > 10
    for off in (0, 4, 12):
        img, _ = _strided(raw, n + 3, off)
        d = _native.DeviceBuffer(0, img.nbytes)
        assert d.ptr % 16 == 0
        d.upload(img)
        b = _batch(kw, "sparse")
        b.enqueue_int16(d.ptr + off, n_samples=n, stream_stride=n + 3)
        _assert_same(_fetch_all(b), want, f"nperseg {nperseg} offset {off}:")
        b.close()
        d.free()
    img, _ = _strided(raw, n + 3, 0)
    d = _native.DeviceBuffer(0, img.nbytes)
    d.upload(img)
    b = _batch(kw, "sparse")
    for off in (1, 2, 3):
        with pytest.raises(_native.NativeError) as ei:
            b.enqueue_int16(d.ptr + off, n_samples=n, stream_stride=n + 3)
        assert ei.value.code == _native.RT_E_INVALID and "aligned" in str(ei.value)
    b.enqueue_int16(d.ptr, n_samples=n, stream_stride=n + 3)
    _assert_same(_fetch_all(b), want, f"nperseg {nperseg} after the refusals:")
    b.close()
    d.free()


def test_host_entry_with_two_calls_in_flight():
    """Host arrays of different lengths, call k + 1 enqueued before call k is fetched, the caller's array overwritten as soon as
    enqueue_int16 returns: the staging copy is what is analysed, and the records are the serial ones."""
    raw_all = ic.wire(256, "hamming")
    kw = ic.kwargs(256, "hamming")
    lens = (ic.BLEN, ic.BLEN - 5000, ic.BLEN - 77)
    starts = (0, ic.BLEN, 2 * ic.BLEN - lens[2])
    bufs = [np.ascontiguousarray(raw_all[:, 2 * a: 2 * (a + n)]) for a, n in zip(starts, lens)]
    serial = _batch(kw, "sparse", row_means=False, record_cells=False)
    want = []
    for x in bufs:
        serial.enqueue_int16(x)
        want.append(serial.fetch_records())
    serial.close()
    assert sum(len(w) for w in want) > 20

    def enqueue_and_overwrite(b, x):
        mine = x.copy()
        b.enqueue_int16(mine)
        mine[:] = 12345

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
    """precision="float64": int16 pairs are (double)i * 2^-15 -- the handle fed i16_to_complex128, byte for byte, and the float64
    oracle on that complex128 within the bounds the float64 path is held to."""
    raw_all = ic.wire(nperseg, window)
    kw = ic.kwargs(nperseg, window)
    bi = _batch(kw, "dense", precision="float64")
    bc = _batch(kw, "dense", precision="float64")
    last = [None] * ic.N_STREAMS
    total = 0
    for k in range(ic.N_BUF):
        raw = ic.buffer_of(raw_all, k)
        c128 = synth.i16_to_complex128(raw)
        bi.enqueue_int16(raw)
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


class _Q:
    def __init__(self):
        self.items = []

    def put(self, x):
        self.items.append(x)


def test_signal_analyzer_process_int16_is_process_samples_on_the_conversion():
    raw_all = ic.wire(256, "hamming")
    kw = ic.kwargs(256, "hamming")
    t0 = datetime.datetime.now()  # (one start for both analyzers' running clocks: the buffers' timestamps are then the same)
    runs = []
    for feed in ("int16", "complex64"):
        q, beat = _Q(), multiprocessing.Value("d", 0.0)
        an = SignalAnalyzer("0", signal_queue=q, last_data_ts=beat, state_update_s=60, sdr_callback_length=ic.BLEN, **kw)
        an._ts = t0
        clocks = []
        for k in range(ic.N_BUF):
            raw = ic.buffer_of(raw_all, k)[0]
            if feed == "int16":
                assert an.process_int16(raw, None) is None
            else:
                assert an.process_samples(synth.i16_to_complex64(raw), None) is None
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
