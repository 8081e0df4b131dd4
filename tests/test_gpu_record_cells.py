"""The cells behind every record (``record_cells=True``, RT_FLAG_RECORD_CELLS) on the GPU: every record's own statistics from
its cells in every size family, the cells against the oracle's spectrogram, the same bits on every mode, lane split and
detection form, growth of the cell pool, which call the cells belong to, the refusals, the float64 handle and
``SignalAnalyzer.signal_data``.  A record is never skipped: every case first holds the record list to its expectation."""
import ctypes as C

import numpy as np
import pytest

from oracle import analyze_oracle as oracle
from pyradiotracking_amd import _native, dB, synth
from pyradiotracking_amd.analyze import BatchSignalAnalyzer, SignalAnalyzer
from tests import float64_cases as fc
from tests import golden_util as gu
from tests import record_cells_util as rcu

pytestmark = pytest.mark.gpu

SPEC_REL_TOL = 2e-4  # tests/test_gpu_parity.py: test_spectrogram_matches_oracle's per-cell bound (with its three-term denominator)
STD_TOL_DB = 0.01    # device log10f against the host's (the tolerance of the GPU suite's dB figures)
U64 = 2.0 ** -53


@pytest.fixture(autouse=True)
def _need_gpu():
    if _native.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")


def _batch(S, blen, fs=2048000, nperseg=256, window="hamming", mode="auto", record_cells=True, **kw):
    return BatchSignalAnalyzer([str(i) for i in range(S)], sdr_callback_length=blen, sample_rate=fs, fft_nperseg=nperseg,
                               fft_window=window, mode=mode, record_cells=record_cells, **kw)


def _streams(S, n, fs, nperseg, window, seed, pulses=4, sigma=synth.NOISE_SIGMA, peak=(-80.0, -60.0), dur_ms=(9, 14), across=None):
    """S streams of n samples; ``across``: a sample index every stream has one more pulse across (6 ms before it, 15 ms long)."""
    w = oracle.window_coefficients(window, nperseg)
    out = []
    for s in range(S):
        rng = np.random.default_rng([seed, s])
        p = synth.random_pulses(rng, n, fs, w, pulses, dur_ms=dur_ms, peak_dbw=peak) if pulses else []
        if across is not None:
            p.append(synth.Pulse(across - int(0.006 * fs), int(0.015 * fs), (0.11 + 0.03 * s) * fs, synth.amp_for_peak_dbw(peak[1], w, fs)))
        out.append(synth.make_stream(synth.StreamSpec(n, fs, p, noise_sigma=sigma), seed * 1000 + s))
    return np.stack(out)


def _fetch(b):
    rec = b.fetch_records()
    off, cells = b.fetch_record_cells()
    assert off.dtype == np.int64 and len(off) == len(rec) + 1 and off[0] == 0
    assert np.array_equal(np.diff(off), rec["end"] - rec["start"])
    assert len(cells) == off[-1] and cells.dtype == (np.float64 if b.native.f64 else np.float32)
    return rec, off, cells


def _run(b, bufs, u8=False):
    out = []
    for chunk in bufs:
        (b.enqueue_bytes if u8 else b.enqueue)(np.ascontiguousarray(chunk))
        out.append(_fetch(b))
    return out


def _check_own_statistics(b, rec, off, cells, t_last, what=""):
    """Item 1: every record's figures are the canonical statistics of its cells, and the cells are the plateau the walk found.
    ``t_last``: segments of the previous buffer (None: there was none)."""
    P = cells.dtype.type
    thr, snr = P(b.signal_threshold), P(b.snr_threshold)
    start_min = 0 if t_last is None else 1 - t_last
    for r, o0, o1 in zip(rec, off[:-1], off[1:]):
        c = cells[o0:o1]
        tag = (what, int(r["stream"]), int(r["fi"]), int(r["start"]), int(r["end"]))
        mx, mean, std = rcu.run_stats(c)
        if np.isnan(mx):
            assert np.isnan(r["max_p"]), tag  # (np.max propagates NaN)
        else:
            assert rcu.bits(np.array([mx])) == rcu.bits(np.array([r["max_p"]])), (tag, mx, r["max_p"])
        assert rcu.bits(np.array([mean])) == rcu.bits(np.array([r["mean_p"]])), (tag, mean, r["mean_p"])
        assert np.isnan(r["std_db"]) == bool(np.any(c == 0)), tag  # NaN iff a cell is exactly zero
        if not np.isnan(r["std_db"]):
            assert abs(float(std) - float(r["std_db"])) <= STD_TOL_DB, (tag, std, r["std_db"])
        above = rcu.cell_above(c, r["row_mean"], thr, snr)
        assert np.all(above[1:]), (tag, np.flatnonzero(~above[1:]) + 1)
        if int(r["start"]) != start_min:
            assert not above[0], tag  # the cell the walk stopped on


def _same(a, b, what):
    """Item 3: byte-identical records, offsets and cells."""
    for k, ((r0, o0, c0), (r1, o1, c1)) in enumerate(zip(a, b)):
        assert r0.tobytes() == r1.tobytes(), (what, k, "records")
        assert np.array_equal(o0, o1) and np.array_equal(rcu.bits(c0), rcu.bits(c1)), (what, k, "cells")


# ----------------------------------------------------------------------------------------------------------------------
# 1. own statistics, every size family
# ----------------------------------------------------------------------------------------------------------------------
_SIZES = (256, 512, 1024, 2048, 32, 64, 128, 4096, 8192, 16, 300)


@pytest.mark.parametrize("u8", [False, True], ids=["c64", "u8"])
@pytest.mark.parametrize("nperseg", _SIZES)
def test_own_statistics_in_every_size_family(nperseg, u8):
    fs, S = 2048000, 3
    T = max(24, 300000 // nperseg)
    n = T * nperseg + nperseg // 3
    if u8:  # (the input of test_uint8_wire_format_ingestion: noise well over the quantisation step)
        iq = _streams(S, 2 * n, fs, nperseg, "hamming", seed=nperseg + 7, pulses=6, sigma=0.012, peak=(-62.0, -48.0), dur_ms=(9, 30), across=n)
        raw = synth.quantize_u8(iq)
        bufs = [raw[:, :2 * n], raw[:, 2 * n:]]
        b = _batch(S, n, fs, nperseg, signal_threshold_dbw=-80.0)
    else:
        iq = _streams(S, 2 * n, fs, nperseg, "hamming", seed=nperseg, pulses=6, across=n)
        bufs = [iq[:, :n], iq[:, n:]]
        b = _batch(S, n, fs, nperseg, signal_threshold_dbw=-75.0)
    runs = _run(b, bufs, u8=u8)
    b.close()
    assert len(runs[0][0]) > 0 and len(runs[1][0]) > 0
    assert np.any(runs[1][0]["start"] < 0), "no record of the second buffer reaches back into the first"
    for k, (rec, off, cells) in enumerate(runs):
        _check_own_statistics(b, rec, off, cells, None if k == 0 else T, f"nperseg {nperseg} buffer {k}")


# ----------------------------------------------------------------------------------------------------------------------
# 2. against the oracle's spectrogram
# ----------------------------------------------------------------------------------------------------------------------
def _oracle_cells(spec, spec_prev, r):
    """analyze.py:437-440 on the oracle's [F, T] maps"""
    fi, start, end = int(r["fi"]), int(r["start"]), int(r["end"])
    if start < 0:
        return np.concatenate((spec_prev[fi][start:], spec[fi][:end]))
    return spec[fi][start:end]


def _denominator(spec, nperseg):
    """[F, T]: the three-term denominator of test_spectrogram_matches_oracle"""
    med = np.median(spec, axis=0, keepdims=True)
    smax = spec.max(axis=0, keepdims=True)
    return spec + 25.0 * max(1.0, nperseg / 4096) * med + 5e-3 * np.sqrt(spec * smax)


@pytest.mark.parametrize("name", gu.iq_case_names())
def test_cells_against_the_oracle_spectrogram(name):
    meta, kwargs, buffers, ts_starts, expected = gu.iq_case(name)
    fs, nperseg, window = kwargs.get("sample_rate", 300000), kwargs.get("fft_nperseg", 256), kwargs.get("fft_window", "hamming")
    an = SignalAnalyzer("0", sdr_callback_length=meta["buffer_len"], record_cells=True, **kwargs)
    oa = oracle.OracleAnalyzer(device="0", **kwargs)
    b = an._batch
    prev = prev_den = None
    n_rec = 0
    for k, (buf, ts) in enumerate(zip(buffers, ts_starts)):
        b.enqueue(buf.reshape(1, -1))
        rec, off, cells = _fetch(b)
        want_all, _ = oa.process(buf, ts)
        assert [(int(r["fi"]), int(r["start"]), int(r["end"])) for r in rec] == [(w.fi, w.start, w.end) for w in want_all], (name, k)
        _, _, spec = oracle.stft_power(np.asarray(buf, dtype=np.complex64), fs, window, nperseg)
        den = _denominator(spec, nperseg)
        for r, o0, o1 in zip(rec, off[:-1], off[1:]):
            want = _oracle_cells(spec, prev, r)
            d = _oracle_cells(den, prev_den, r)
            rel = np.abs(cells[o0:o1].astype(np.float64) - want) / d
            assert rel.max() < SPEC_REL_TOL, (name, k, int(r["fi"]), int(r["start"]), int(np.argmax(rel)), float(rel.max()))
        _check_own_statistics(b, rec, off, cells, None if prev is None else prev.shape[1], f"{name} b{k}")
        prev, prev_den = spec, den
        n_rec += len(rec)
    assert n_rec > 0
    an._batch.close()


# ----------------------------------------------------------------------------------------------------------------------
# 3. one answer on every path
# ----------------------------------------------------------------------------------------------------------------------
def _mode_runs(bufs, modes, **kw):
    geometry = (kw.pop("sample_rate", 2048000), kw.pop("fft_nperseg", 256), kw.pop("fft_window", "hamming"))
    runs, infos = {}, {}
    for mode in modes:
        try:
            b = _batch(bufs[0].shape[0], bufs[0].shape[1], *geometry, mode=mode, **kw)
        except _native.NativeError as e:
            assert e.code == _native.RT_E_UNSUPPORTED, (mode, e)  # (a pre-filter level the geometry does not have)
            continue
        try:
            runs[mode] = []
            infos[mode] = []
            for chunk in bufs:
                b.enqueue(np.ascontiguousarray(chunk))
                runs[mode].append(_fetch(b))
                infos[mode].append(b.native.call_info())
        except _native.NativeError as e:
            assert e.code == _native.RT_E_HOT_OVERFLOW and mode not in ("auto", "dense"), (mode, e)  # (a pinned level too narrow)
            del runs[mode]
        b.close()
    return runs, infos


def test_modes_give_the_same_cells_on_clean_input():
    fs, nperseg = 2048000, 256
    B = 700 * nperseg + 40
    iq = _streams(4, 2 * B, fs, nperseg, "hamming", seed=21, pulses=8, across=B)
    runs, _ = _mode_runs([iq[:, :B], iq[:, B:]], ("dense", "sparse", "prefilter", "runfilter", "auto"), sample_rate=fs, signal_min_duration_ms=8)
    assert {"dense", "sparse", "auto"} <= set(runs) and len(runs) >= 4, sorted(runs)
    assert sum(len(r) for r, _, _ in runs["dense"]) > 0 and np.any(runs["dense"][1][0]["start"] < 0)
    for mode, got in runs.items():
        _same(runs["dense"], got, mode)


@pytest.mark.parametrize("floor_db", [0.0, 4.0])
def test_modes_give_the_same_cells_under_the_noise_floor(floor_db):
    bufs, _, kw = gu.reference_noise_floor_case(floor_db)
    bufs = [np.stack([b] * 3) for b in bufs]
    runs, _ = _mode_runs(bufs, ("dense", "sparse", "prefilter", "runfilter", "auto"), **kw)
    assert {"dense", "auto"} <= set(runs) and len(runs) >= 3, sorted(runs)
    assert sum(len(r) for r, _, _ in runs["dense"]) > 0
    for mode, got in runs.items():
        _same(runs["dense"], got, f"floor {floor_db} {mode}")


def test_auto_partial_dense_rerun_gives_the_cells_of_the_dense_run():
    """One noisy stream among clean ones overflows its candidate lists: AUTO re-runs it alone, densely -- its cells from that
    map, the others' from their lists."""
    fs, nperseg, B, S = 300000, 256, 256 * 700, 12
    w = oracle.window_coefficients("hamming", nperseg)
    iq = []
    for s in range(S):
        rng = np.random.default_rng([45, s])
        p = synth.random_pulses(rng, 2 * B, fs, w, 6, peak_dbw=(-80.0, -62.0))
        sigma = float(np.sqrt(10 ** (-88.0 / 10) * fs / 2)) if s == 5 else synth.NOISE_SIGMA
        iq.append(synth.make_stream(synth.StreamSpec(2 * B, fs, p, noise_sigma=sigma), seed=800 + s))
    iq = np.stack(iq)
    runs, infos = _mode_runs([iq[:, :B], iq[:, B:]], ("dense", "auto"), sample_rate=fs, record_capacity=2048)
    assert any(i.n_dense_streams > 0 for i in infos["auto"]), [i.n_dense_streams for i in infos["auto"]]
    assert sum(len(r) for r, _, _ in runs["dense"]) > 0
    _same(runs["dense"], runs["auto"], "auto")


@pytest.mark.parametrize("nperseg", [256, 128, 1000])
def test_lanes_and_group_detect_give_the_same_cells(nperseg):
    fs, S = 2048000, 7
    B = (200000 // nperseg) * nperseg + 5
    iq = _streams(S, 2 * B, fs, nperseg, "hamming", seed=33 + nperseg, pulses=6, across=B)
    bufs = [iq[:, :B], iq[:, B:]]
    want = None
    for lanes in (1, 2, 3):
        for gd in (False, True):
            b = _batch(S, B, fs, nperseg, lanes=lanes, group_detect=gd)
            got = _run(b, bufs)
            b.close()
            if want is None:
                want = got
                assert sum(len(r) for r, _, _ in want) > 0
            else:
                _same(want, got, (lanes, gd))


@pytest.mark.parametrize("nperseg", [256, 1024, 128])
def test_uint8_and_complex64_give_the_same_cells(nperseg):
    """set up as test_uint8_wire_format_ingestion: the bytes, and the complex64 handle fed the kernel's own conversion"""
    fs, S, blen = 2048000, 3, 256 * 1100 + 40
    iq = _streams(S, 2 * blen, fs, nperseg, "hamming", seed=321 + nperseg, pulses=8, sigma=0.012, peak=(-62.0, -48.0), dur_ms=(9, 30), across=blen)
    raw = synth.quantize_u8(iq)
    kw = dict(signal_threshold_dbw=-80.0, mode="sparse")
    b8 = _batch(S, blen, fs, nperseg, **kw)
    bc = _batch(S, blen, fs, nperseg, subtract_first=True, **kw)
    r8 = _run(b8, [raw[:, :2 * blen], raw[:, 2 * blen:]], u8=True)
    rc = _run(bc, [synth.u8_to_complex64_like_kernel(raw[:, :2 * blen]), synth.u8_to_complex64_like_kernel(raw[:, 2 * blen:])])
    b8.close()
    bc.close()
    assert sum(len(r) for r, _, _ in r8) > 20
    _same(r8, rc, "uint8 / complex64")


# ----------------------------------------------------------------------------------------------------------------------
# 4. growth and order
# ----------------------------------------------------------------------------------------------------------------------
def test_thousands_of_plateaus_and_a_cell_pool_far_too_small():
    """The stream of test_thousands_of_plateaus_in_one_stream_equal_the_oracle on a handle whose record pool starts at 64 records
    (the cell pool: sixteen cells a record of it, 1 024 cells): record capacity, record pool and cell pool all grow inside the
    fetch, the records are the oracle's and every record has its cells."""
    fs, nperseg, n_seg = 2048000, 256, 8000
    blen = n_seg * nperseg
    w = oracle.window_coefficients("boxcar", nperseg)
    pulses = []
    for j in range(9):
        amp = synth.amp_for_peak_dbw(-60.0 - 2.0 * j, w, fs)
        f = (17 + 17 * j) * fs / nperseg
        pulses += [synth.Pulse(t0 * nperseg, 7 * nperseg, f, amp) for t0 in range(3, n_seg - 12, 12)]
    heavy = synth.make_stream(synth.StreamSpec(blen, fs, pulses), seed=5)
    rng = np.random.default_rng(2)
    light = synth.make_stream(synth.StreamSpec(blen, fs, synth.random_pulses(rng, blen, fs, w, 3, dur_ms=(2, 5))), seed=6)
    iq = np.stack([heavy, light])
    kw = dict(signal_min_duration_ms=0.5, snr_threshold_db=-20.0)
    okw = dict(sample_rate=fs, fft_nperseg=nperseg, fft_window="boxcar", **kw)
    want = [oracle.OracleAnalyzer(device=str(s), **okw).process(iq[s], gu.TS0)[0] for s in range(2)]
    assert len(want[0]) > 5000
    runs = {}
    for mode, pool in (("sparse", 64), ("dense", 64), ("sparse", 0)):
        b = _batch(2, blen, fs, nperseg, "boxcar", mode=mode, record_pool=pool, **kw)
        b.enqueue(iq)
        rec, off, cells = _fetch(b)
        assert not b.native.last_truncated
        for s in range(2):
            mine = rec[rec["stream"] == s]
            assert [(int(r["fi"]), int(r["start"]), int(r["end"])) for r in mine] == [(x.fi, x.start, x.end) for x in want[s]], (mode, pool, s)
        assert len(cells) > 16 * max(pool, 1)  # (the pool the handle started with could not hold them)
        _check_own_statistics(b, rec, off, cells, None, f"{mode} pool {pool}")
        # the next, ordinary call on the grown handle
        b.enqueue(np.stack([light, light]))
        rec2, off2, cells2 = _fetch(b)
        assert len(rec2) > 0
        _check_own_statistics(b, rec2, off2, cells2, n_seg, f"{mode} pool {pool}, second call")
        b.close()
        runs[(mode, pool)] = [(rec, off, cells), (rec2, off2, cells2)]
    _same(runs[("sparse", 0)], runs[("sparse", 64)], "grown pool")
    _same(runs[("sparse", 0)], runs[("dense", 64)], "dense")


@pytest.mark.parametrize("mode", ["auto", "dense"])
def test_record_growth_beside_the_cells(mode):
    fs, nperseg, S = 2048000, 256, 3
    B = 2000 * nperseg
    iq = _streams(S, B, fs, nperseg, "hamming", seed=55, pulses=120, dur_ms=(2, 4))
    small = _batch(S, B, mode=mode, record_capacity=16, record_pool=8, signal_min_duration_ms=1)
    rs = _run(small, [iq])
    small.close()
    big = _batch(S, B, mode=mode, record_capacity=4096, signal_min_duration_ms=1)
    rb = _run(big, [iq])
    big.close()
    assert max(int((rb[0][0]["stream"] == s).sum()) for s in range(S)) > 16
    _same(rb, rs, "grown")
    _check_own_statistics(big, *rb[0], None, mode)


@pytest.mark.parametrize("lanes", [1, 2])
def test_pipelined_calls_and_invalidation(lanes):
    fs, nperseg, S = 2048000, 256, 4
    B = 300 * nperseg
    iq = _streams(S, 4 * B, fs, nperseg, "hamming", seed=44, pulses=10)
    bufs = [iq[:, k * B:(k + 1) * B] for k in range(4)]
    b = _batch(S, B, lanes=lanes)
    seq = _run(b, bufs)
    assert all(len(r) > 0 for r, _, _ in seq)
    b.reset()
    with pytest.raises(_native.NativeError) as ei:
        b.fetch_record_cells()  # (reset: nothing delivered since)
    assert ei.value.code == _native.RT_E_INVALID
    b.close()

    b = _batch(S, B, lanes=lanes)
    with pytest.raises(_native.NativeError):
        b.fetch_record_cells()  # (nothing delivered yet)
    b.enqueue(bufs[0])
    b.enqueue(bufs[1])
    got0 = _fetch(b)  # process k, process k + 1, fetch k, cells k
    got1 = _fetch(b)
    _same(seq[:2], [got0, got1], "two calls in flight")
    assert np.array_equal(rcu.bits(b.fetch_record_cells()[1]), rcu.bits(seq[1][2]))  # (a second fetch of the same cells: nothing is consumed)
    b.enqueue(bufs[2])
    with pytest.raises(_native.NativeError) as ei:
        b.fetch_record_cells()
    assert ei.value.code == _native.RT_E_INVALID
    _same(seq[2:3], [_fetch(b)], "third call")
    b.reset()
    with pytest.raises(_native.NativeError) as ei:
        b.fetch_record_cells()
    assert ei.value.code == _native.RT_E_INVALID
    b.close()


def test_refusals_and_the_size_query():
    lib = _native.load_library()
    fs, nperseg, S, B = 2048000, 256, 2, 400 * 256
    iq = _streams(S, B, fs, nperseg, "hamming", seed=77, pulses=6)
    b = _batch(S, B)
    h = b.native._handle
    b.enqueue(iq)
    n = C.c_size_t(0)
    # a fetch into a buffer too short for the call's records (cap < *n_out): the call is consumed, its cells are not handed out
    one = np.zeros(1, dtype=_native.RECORD_DTYPE)
    assert lib.rt_fetch(h, one.ctypes.data, 1, C.byref(n)) in (_native.RT_OK, _native.RT_E_CAPACITY) and n.value > 1
    assert lib.rt_fetch_record_cells(h, None, 0, None, 0, C.byref(n)) == _native.RT_E_INVALID
    # delivered in full
    b.enqueue(iq)
    rec, off, cells = _fetch(b)
    assert len(rec) > 1
    total = C.c_size_t(0)
    assert lib.rt_fetch_record_cells(h, None, 0, None, 0, C.byref(total)) == _native.RT_OK and total.value == len(cells)  # size query, no offsets
    off2 = np.zeros(len(rec) + 1, np.int64)
    assert lib.rt_fetch_record_cells(h, off2.ctypes.data, len(rec), None, 0, C.byref(total)) == _native.RT_E_INVALID  # wrong n_offsets
    assert lib.rt_fetch_record_cells(h, off2.ctypes.data, len(rec) + 2, None, 0, C.byref(total)) == _native.RT_E_INVALID
    short = np.full(len(cells), -1.0, np.float32)
    assert lib.rt_fetch_record_cells(h, off2.ctypes.data, len(off2), short.ctypes.data, len(cells) - 1, C.byref(total)) == _native.RT_E_CAPACITY
    assert total.value == len(cells) and np.all(short == -1.0)  # nothing written
    assert lib.rt_fetch_record_cells(h, off2.ctypes.data, len(off2), short.ctypes.data, len(cells), C.byref(total)) == _native.RT_OK
    assert np.array_equal(off2, off) and np.array_equal(rcu.bits(short), rcu.bits(cells))
    assert lib.rt_fetch_record_cells(h, None, 0, None, 0, None) == _native.RT_E_INVALID
    dbl = np.zeros(len(cells), np.float64)
    assert lib.rt_fetch_record_cells_f64(h, off2.ctypes.data, len(off2), dbl.ctypes.data, len(dbl), C.byref(total)) == _native.RT_E_INVALID  # the twin
    # an rt_extract call: the caller holds that map
    T = 400
    spec = np.full((S, T, nperseg), 1e-12, np.float32)
    spec[:, 50:150, 7] = 1e-6
    d = _native.DeviceBuffer(0, spec.nbytes)
    d.upload(spec)
    b.native.extract_device(d.ptr, T, nperseg, None, 0)
    with pytest.raises(_native.NativeError):
        b.fetch_record_cells()  # (an rt_extract was enqueued since)
    assert len(b.native.fetch()) > 0
    with pytest.raises(_native.NativeError) as ei:
        b.fetch_record_cells()  # (the delivered call was an rt_extract)
    assert ei.value.code == _native.RT_E_INVALID
    d.free()
    # a call without records, and a buffer shorter than a segment
    for quiet in (np.zeros((S, B), np.complex64), np.zeros((S, nperseg - 1), np.complex64)):
        b.enqueue(quiet)
        rec, off, cells = _fetch(b)
        assert len(rec) == 0 and off.tolist() == [0] and len(cells) == 0
    b.close()
    # the float64 handle refuses the float32 entry
    b64 = _batch(1, 4096, fs=fc.FS, precision="float64")
    b64.enqueue(np.zeros((1, 4096), np.complex128))
    b64.fetch_records()
    assert lib.rt_fetch_record_cells(b64.native._handle, None, 0, None, 0, C.byref(total)) == _native.RT_E_INVALID
    assert lib.rt_fetch_record_cells_f64(b64.native._handle, None, 0, None, 0, C.byref(total)) == _native.RT_OK and total.value == 0
    b64.close()


# ----------------------------------------------------------------------------------------------------------------------
# 5. flag off changes nothing
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,lanes,precision", [("auto", 1, "float32"), ("dense", 1, "float32"), ("runfilter", 1, "float32"), ("auto", 2, "float32"),
                                                  ("auto", 1, "float64")])
def test_flag_off_refuses_and_leaves_records_and_row_means_alone(mode, lanes, precision):
    fs, nperseg, S = 2048000, 256, 4
    B = 500 * nperseg
    iq = _streams(S, 2 * B, fs, nperseg, "hamming", seed=66, pulses=8, across=B)
    if precision == "float64":
        iq = iq.astype(np.complex128)
    out = {}
    for flag in (False, True):
        b = _batch(S, B, mode=mode, lanes=lanes, precision=precision, record_cells=flag, row_means=True)
        out[flag] = []
        for k in range(2):
            b.enqueue(iq[:, k * B:(k + 1) * B])
            rec = b.fetch_records()
            out[flag].append((rec, b.fetch_row_means()))
            if not flag:
                with pytest.raises(_native.NativeError) as ei:
                    b.fetch_record_cells()
                assert ei.value.code == _native.RT_E_INVALID
            else:
                b.fetch_record_cells()
        b.close()
    assert sum(len(r) for r, _ in out[True]) > 0
    for (r0, m0), (r1, m1) in zip(out[False], out[True]):
        assert r0.tobytes() == r1.tobytes() and np.array_equal(rcu.bits(m0), rcu.bits(m1))


# ----------------------------------------------------------------------------------------------------------------------
# 6. float64 handles
# ----------------------------------------------------------------------------------------------------------------------
def _pulses128(n, fs, nperseg, seed, across, sigma=synth.NOISE_SIGMA, peak=(-80.0, -60.0)):
    """complex128 buffer: noise and random pulses added in float64, one across sample ``across``"""
    rng = np.random.default_rng([128, seed])
    w = oracle.window_coefficients("hamming", nperseg)
    x = sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    pulses = synth.random_pulses(rng, n, fs, w, 6, dur_ms=(10.0, 30.0), peak_dbw=peak)
    pulses.append(synth.Pulse(across - int(0.006 * fs), int(0.015 * fs), 0.11 * fs, synth.amp_for_peak_dbw(peak[1] - 2.0, w, fs)))
    for p in pulses:
        a, b = max(0, p.start), min(n, p.start + p.length)
        if b > a:
            t = np.arange(a, b, dtype=np.float64) / fs
            x[a:b] += p.amp * np.exp(2j * np.pi * (p.freq * t + p.phase))
    return x


def _f64_cell_bound(spec, nperseg):
    """[F, T]: a float64 transform's per-cell error, 3 log2(M) 64 u sqrt(P[k, t] E_t) (M the transform length, Bluestein's padded
    one; E_t the segment's mean cell power -- the per-cell term of test_gpu_row_means._f64_bound), plus 4 u P for the square,
    the scale and the rounding.  Far inside tests/precision64.py's cell bound, which is the same expression in float32 units."""
    m = 1
    while m < (nperseg if nperseg & (nperseg - 1) == 0 else 2 * nperseg - 1):
        m <<= 1
    e_t = spec.mean(axis=0, keepdims=True)
    return 3 * np.log2(m) * 64 * U64 * np.sqrt(spec * e_t) + 4 * U64 * spec


@pytest.mark.parametrize("u8", [False, True], ids=["c128", "u8"])
@pytest.mark.parametrize("nperseg", [256, 300, 4096])
def test_float64_cells(nperseg, u8):
    fs = fc.FS if nperseg <= 300 else 2048000  # (hops of 2 ms at nperseg 4096: the pulse across the edge stays inside the duration gate)
    n = max(300000, nperseg * 64) // nperseg * nperseg + nperseg // 3
    kw = {}
    if u8:  # (the input of test_gpu_float64_path.test_wire_format_bytes: noise over the quantisation step, full scale)
        x = _pulses128(2 * n, fs, nperseg, nperseg, n, sigma=0.05, peak=(-66.0, -60.0))
        raw = synth.quantize_u8(x / np.abs(x).max() * 0.9)
        x = synth.u8_to_complex128_like_pyrtlsdr(raw)
        kw = dict(signal_threshold_dbw=-60.0)
    else:
        x = _pulses128(2 * n, fs, nperseg, nperseg, n)
    b = _batch(1, n, fs, nperseg, precision="float64", **kw)
    prev = prev_bound = None
    n_rec = n_back = 0
    for k in range(2):
        xs = x[k * n:(k + 1) * n]
        if u8:
            b.enqueue_bytes(raw[2 * k * n:2 * (k + 1) * n].reshape(1, -1))
        else:
            b.enqueue(xs.reshape(1, -1))
        rec, off, cells = _fetch(b)
        want, spec = fc.oracle_records(xs, nperseg, "hamming", fs, last=prev, **kw)
        assert [(int(r["fi"]), int(r["start"]), int(r["end"])) for r in rec] == fc.key(want), (nperseg, k)
        _check_own_statistics(b, rec, off, cells, None if prev is None else prev.shape[1], f"float64 {nperseg} b{k}")
        bound = _f64_cell_bound(spec, nperseg)
        for r, o0, o1 in zip(rec, off[:-1], off[1:]):
            err = np.abs(cells[o0:o1] - _oracle_cells(spec, prev, r))
            bd = _oracle_cells(bound, prev_bound, r)
            assert np.all(err <= bd), (nperseg, k, int(r["fi"]), int(r["start"]), float((err / bd).max()))
        prev, prev_bound = spec, bound
        n_rec += len(rec)
        n_back += int(np.sum(rec["start"] < 0))
    b.close()
    assert n_rec > 0 and n_back > 0


def test_float64_cell_pool_grows():
    fs, nperseg = fc.FS, 256
    n = 300000 // nperseg * nperseg
    x = _pulses128(2 * n, fs, nperseg, 11, n)
    runs = []
    for cap in (2, 1024):  # (record_capacity 2: a cell pool of 64 cells, and the capacity itself too small)
        b = _batch(1, n, fs, nperseg, precision="float64", record_capacity=cap)
        runs.append(_run(b, [x[:n].reshape(1, -1), x[n:].reshape(1, -1)]))
        b.close()
    assert sum(len(r) for r, _, _ in runs[1]) > 2 and sum(len(c) for _, _, c in runs[1]) > 64
    _same(runs[1], runs[0], "float64 growth")


# ----------------------------------------------------------------------------------------------------------------------
# 7. drop-in
# ----------------------------------------------------------------------------------------------------------------------
def test_signal_analyzer_signal_data():
    import queue

    meta, kwargs, buffers, ts_starts, expected = gu.iq_case("cfg1_tone")
    q = queue.Queue()
    an = SignalAnalyzer("0", sdr_callback_length=meta["buffer_len"], record_cells=True, signal_queue=q, **kwargs)
    assert an.signal_data is None
    cal = kwargs.get("calibration_db", 0.0)
    n_sig = 0
    for buf in buffers:
        an.process_samples(buf)
        sigs = []
        while not q.empty():
            m = q.get()
            if hasattr(m, "frequency"):
                sigs.append(m)
        assert len(an.signal_data) == len(sigs)
        for d, sig in zip(an.signal_data, sigs):
            assert d.dtype == np.float32
            # the reference's own expressions (analyze.py:442-445)
            assert np.float32(dB(np.max(d)) - cal) == np.float32(sig.max)
            assert abs((dB(np.mean(d)) - cal) - sig.avg) < 1e-4
            assert abs(np.std(dB(d)) - sig.std) < STD_TOL_DB
        n_sig += len(sigs)
    assert n_sig > 0
    # filtered=False: the cells of every signal extract_signals would have listed
    an2 = SignalAnalyzer("0", sdr_callback_length=meta["buffer_len"], record_cells=True, **kwargs)
    for buf, ts in zip(buffers, ts_starts):
        sigs = an2.analyze_buffer(buf, ts, filtered=False)
        assert len(an2.signal_data) == len(sigs)
    plain = SignalAnalyzer("0", sdr_callback_length=meta["buffer_len"], **kwargs)
    plain.analyze_buffer(buffers[0], ts_starts[0])
    assert plain.signal_data is None
