"""The map-free float64 path (precision="float64", f64_sparse=True: RT_FLAG_F64_SPARSE) on the GPU against the oracle on the
same complex128 values.  Inputs: tests/f64_sparse_cases.py (seeds clear of the thresholds, so that another summation order
cannot flip a decision).  Tolerances and the shape of the checks: tests/test_gpu_float64_path.py."""
import datetime

import numpy as np
import pytest

from oracle import analyze_oracle as oracle
from pyradiotracking_amd import _native, synth
from pyradiotracking_amd.analyze import BatchSignalAnalyzer, SignalAnalyzer
from tests import f64_sparse_cases as sc
from tests import float64_cases as fc

pytestmark = pytest.mark.gpu

DB_TOL = 1e-9   # max / avg / noise / snr, dB
STD_TOL = 1e-5  # std, dB
FS = sc.FS


@pytest.fixture(autouse=True)
def _need_gpu():
    if _native.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")


def _keys(rec):
    return [(int(r["fi"]), int(r["start"]), int(r["end"])) for r in rec]


def _check(rec, want, cal=0.0):
    """rt_record_f64 rows of one stream against oracle records (all of them, shadow verdicts from the oracle's filter)."""
    sig = oracle.records_to_signals(want, np.zeros(4096), fc.TS0, "0", 0.0)
    kept = {(s.fi, s.start) for s in oracle.filter_shadows(sig)}
    assert _keys(rec) == fc.key(want)
    assert [int(r["shadowed"]) for r in rec] == [0 if (w.fi, w.start) in kept else 1 for w in want]
    if not len(want):
        return
    np.testing.assert_allclose(oracle.to_db(rec["max_p"]) - cal, [w.max_dbw for w in want], rtol=0, atol=DB_TOL)
    np.testing.assert_allclose(oracle.to_db(rec["mean_p"]) - cal, [w.avg_dbw for w in want], rtol=0, atol=DB_TOL)
    np.testing.assert_allclose(oracle.to_db(rec["row_mean"]), [w.noise_dbw for w in want], rtol=0, atol=DB_TOL)
    np.testing.assert_allclose(oracle.to_db(rec["mean_p"] / rec["row_mean"]), [w.snr_db for w in want], rtol=0, atol=DB_TOL)
    np.testing.assert_allclose(rec["std_db"], [w.std_db for w in want], rtol=0, atol=STD_TOL)


def _check_signals(rec, want, cal=0.0):
    """... against OracleSignals (OracleAnalyzer.process: every signal, with the kept ones)."""
    sigs, kept = want
    kept_ids = {id(s) for s in kept}
    assert _keys(rec) == [(s.fi, s.start, s.end) for s in sigs]
    assert [int(r["shadowed"]) for r in rec] == [0 if id(s) in kept_ids else 1 for s in sigs]
    if not sigs:
        return
    np.testing.assert_allclose(oracle.to_db(rec["max_p"]) - cal, [s.max for s in sigs], rtol=0, atol=DB_TOL)
    np.testing.assert_allclose(oracle.to_db(rec["mean_p"]) - cal, [s.avg for s in sigs], rtol=0, atol=DB_TOL)
    np.testing.assert_allclose(oracle.to_db(rec["row_mean"]), [s.noise for s in sigs], rtol=0, atol=DB_TOL)
    np.testing.assert_allclose(oracle.to_db(rec["mean_p"] / rec["row_mean"]), [s.snr for s in sigs], rtol=0, atol=DB_TOL)
    np.testing.assert_allclose(rec["std_db"], [s.std for s in sigs], rtol=0, atol=STD_TOL)


def _analyzer(n_streams, n, nperseg=256, sparse=True, **kw):
    return BatchSignalAnalyzer([str(i) for i in range(n_streams)], precision="float64", f64_sparse=sparse, sdr_callback_length=n,
                               fft_nperseg=nperseg, sample_rate=FS, **kw)


def _is_sparse(b):
    return b.call_info().mode_used == _native.RT_MODE_SPARSE


# ---- 1. sizes ----
@pytest.mark.parametrize("nperseg,window,cal", sc.SIZE_CASES, ids=[f"{n}-{w if isinstance(w, str) else w[0]}" for n, w, _ in sc.SIZE_CASES])
def test_sizes_match_complex128_reference(nperseg, window, cal):
    import torch

    x = sc.size_buffer(nperseg, window, sc.SIZE_SEEDS[(nperseg, window, cal)])
    want, _ = fc.oracle_records(x, nperseg, window, FS, calibration_db=cal)
    assert len(want) >= 1
    # (nperseg 32: a pulse's skirt under the tukey window fills most of the 32 bins -- 4 254 candidate cells, over the default 4 096)
    b = _analyzer(1, len(x), nperseg, fft_window=window, calibration_db=cal, hot_capacity=8192 if nperseg == 32 else 0)
    try:
        for feed in ("host", "device"):
            b.reset_stream(0)
            b.enqueue(x[None, :] if feed == "host" else torch.from_numpy(x[None, :].copy()).cuda())
            rec = b.fetch_records()
            assert _is_sparse(b)
            _check(rec, want, cal)
    finally:
        b.close()


# ---- 2. the transform, cell by cell ----
@pytest.mark.parametrize("nperseg", sc.SIZES)
def test_transform_cells_through_row_means(nperseg):
    """T = 2 with an all-zero second segment: its powers are exactly 0, so twice the row mean is segment 0's cell."""
    rng = np.random.default_rng(nperseg)
    S = 2
    x = np.zeros((S, 2 * nperseg), dtype=np.complex128)
    seg0 = rng.standard_normal((S, nperseg)) + 1j * rng.standard_normal((S, nperseg)) + 0.3
    seg0[:, ::7] *= 1e3  # a dynamic range for the bound to mean something
    x[:, :nperseg] = seg0
    b = _analyzer(S, 2 * nperseg, nperseg, row_means=True, hot_capacity=8192)  # (segment 0's nperseg cells are all candidates)
    try:
        b.enqueue(x)
        b.fetch_records()
        assert _is_sparse(b)
        means = b.fetch_row_means()
    finally:
        b.close()
    got = 2.0 * means
    for s in range(S):
        _, _, ref = oracle.stft_power(x[s, :nperseg], FS, "hamming", nperseg)
        ref = ref[:, 0]
        bound = 1e-13 * np.log2(nperseg) * ref.max()
        assert np.all(np.abs(got[s] - ref) <= bound), float(np.max(np.abs(got[s] - ref) / bound))


# ---- 3. chunk boundaries ----
def _boundary_batch(nperseg, T, n_streams, pulse_segs=6):
    """Stream s: one bin-centred pulse of ``pulse_segs`` whole segments from segment s + 1 on, where it fits before the end."""
    n = T * nperseg
    x = np.stack([sc.noise(n, 100 + s) for s in range(n_streams)])
    for s in range(n_streams):
        if s + 1 + pulse_segs < T:
            x[s] += sc.tone(n, nperseg, 20 + s, s + 1, pulse_segs)
    return x


@pytest.mark.parametrize("nperseg,spc,T,n_streams", [(256, 4, 21, 14), (256, 4, 2, 14), (256, 4, 3, 14), (256, 4, 4, 14), (256, 4, 5, 14),
                                                     (256, 4, 9, 14), (2048, 3, 10, 3)])
def test_chunk_boundaries(nperseg, spc, T, n_streams):
    x = _boundary_batch(nperseg, T, n_streams)
    dur_ms = 5.5 * nperseg / FS * 1e3  # six segments pass (the cell before the run counts: seven hops), five do not
    # (a pulse of six segments is most of a row of nine or ten: its cells are 1.5 x the row mean -- an SNR threshold of 1 dB there)
    kw = dict(signal_min_duration_ms=dur_ms, signal_max_duration_ms=40.0 * nperseg / 256, snr_threshold_db=5.0 if T == 21 else 1.0)
    assert all(sc.clear_of_thresholds(x[s], nperseg, **kw) for s in range(n_streams))
    b = _analyzer(n_streams, x.shape[1], nperseg, segs_per_chunk=spc, **kw)
    try:
        b.enqueue(x)
        rec = b.fetch_records()
        assert _is_sparse(b)
    finally:
        b.close()
    found = 0
    for s in range(n_streams):
        want, _ = fc.oracle_records(x[s], nperseg, "hamming", FS, **kw)
        _check(rec[rec["stream"] == s], want)
        found += len(want)
    assert found >= (n_streams if T == 21 else 2 if T >= 9 else 0)


# ---- 4. the buffer's edges ----
def test_buffer_edges():
    """A plateau whose first hot cell is t = 0 takes its predecessor from the tail; one that reaches t = T - 1 is skipped, as the
    reference skips it, and the next call's look-back finds its continuation."""
    nperseg, n = 256, 256 * 100
    x = sc.noise(2 * n, 1) + sc.tone(2 * n, nperseg, 40, 96, 10) + sc.tone(2 * n, nperseg, 90, 194, 6) + sc.tone(2 * n, nperseg, 7, 100, 9)
    bufs = [x[:n], x[n:]]
    assert all(sc.clear_of_thresholds(v, nperseg) for v in bufs)
    oa = oracle.OracleAnalyzer(sample_rate=FS)
    want = [oa.process(v, fc.TS0) for v in bufs]
    assert 40 not in [s.fi for s in want[0][0]] and 90 not in [s.fi for s in want[1][0]]
    assert {(7, -1, 9), (40, -5, 6)} <= {(s.fi, s.start, s.end) for s in want[1][0]}
    b = _analyzer(1, n, nperseg)
    try:
        for v, w in zip(bufs, want):
            b.enqueue(v[None, :])
            _check_signals(b.fetch_records(), w)
            assert _is_sparse(b)
    finally:
        b.close()


# ---- 5. look-back over a sequence ----
def _sequence(lengths, nperseg=256, seed=7):
    """One stream cut into calls of ``lengths`` samples, a 20 ms pulse across every cut (and one inside every call)."""
    total = sum(lengths)
    x = sc.noise(total, seed)
    cuts = np.cumsum(lengths)[:-1]
    for i, cut in enumerate(cuts):
        k = np.arange(cut - 3000, cut + 3000)
        x[k] += sc.tone_at(k, nperseg, 20 + 5 * i)
    for i, cut in enumerate(np.concatenate(([0], cuts))):
        k = np.arange(cut + 20000, cut + 24000)
        x[k] += sc.tone_at(k, nperseg, 100 + 7 * i)
    edges = np.concatenate(([0], np.cumsum(lengths)))
    return [x[a:b] for a, b in zip(edges[:-1], edges[1:])]


def test_lookback_over_a_sequence():
    lengths = [60000, 45000, 80000, 60000, 45000, 80000, 60000]
    bufs = _sequence(lengths)
    assert all(sc.clear_of_thresholds(v) for v in bufs)
    oa = oracle.OracleAnalyzer(sample_rate=FS)
    want = [oa.process(v, fc.TS0) for v in bufs[:6]]
    assert sum(any(s.start < 0 for s in w[0]) for w in want) >= 5  # every cut is straddled
    b = _analyzer(1, 80000)
    try:
        b.enqueue(bufs[0][None, :])
        b.enqueue(bufs[1][None, :])  # two calls in flight
        got = [b.fetch_records()]
        for k in range(2, 6):
            b.enqueue(bufs[k][None, :])
            got.append(b.fetch_records())
        got.append(b.fetch_records())
        for g, w in zip(got, want):
            _check_signals(g, w)
        b.reset_stream(0)  # the next buffer without look-back, as a fresh analyzer
        b.enqueue(bufs[6][None, :])
        fresh = oracle.OracleAnalyzer(sample_rate=FS).process(bufs[6], fc.TS0)
        again = oa.process(bufs[6], fc.TS0)
        assert [(s.fi, s.start) for s in fresh[0]] != [(s.fi, s.start) for s in again[0]]  # (the look-back would have shown)
        _check_signals(b.fetch_records(), fresh)
        assert _is_sparse(b)
    finally:
        b.close()


# ---- 6. formats ----
@pytest.mark.parametrize("nperseg", [256, 1024])
@pytest.mark.parametrize("fmt", ["u8", "i16", "i8"])
def test_integer_formats(fmt, nperseg):
    n = max(300000, 64 * nperseg)
    for seed in range(sc.CANDIDATES):
        x = sc.pulses(n, FS, nperseg, "hamming", 500 + seed, sigma=0.05)
        x = x / np.abs(x).max() * 0.9
        if fmt == "u8":
            raw = synth.quantize_u8(x)
            ref = synth.u8_to_complex128_like_pyrtlsdr(raw)
        elif fmt == "i16":
            raw = synth.quantize_i16(x)
            ref = synth.i16_to_complex128(raw)
        else:
            raw = synth.quantize_i8(x)
            ref = synth.i8_to_complex128(raw)
        if sc.clear_of_thresholds(ref, nperseg, signal_threshold_dbw=-60.0):
            break
    else:
        pytest.fail("no seed clear of its thresholds")
    want, _ = fc.oracle_records(ref, nperseg, "hamming", FS, signal_threshold_dbw=-60.0)
    # (noise 8.5 dB under the threshold: 0.7 % of 300 000 cells are over it, 4 300 candidates with their predecessors)
    b = _analyzer(1, n, nperseg, signal_threshold_dbw=-60.0, hot_capacity=8192)
    try:
        {"u8": b.enqueue_bytes, "i16": b.enqueue_int16, "i8": b.enqueue_int8}[fmt](raw[None, :])
        rec = b.fetch_records()
        assert _is_sparse(b)
    finally:
        b.close()
    _check(rec, want)


# ---- 7. per-stream values ----
def test_per_stream_values():
    nperseg, n = 256, 60000
    thr = [-95.0, -85.0, -75.0]
    cal = [0.0, 3.0, -2.0]
    snr = [5.0, 3.0, 7.0]
    lo, hi = [8.0, 4.0, 10.0], [40.0, 30.0, 50.0]
    # every stream: pulses at -90, -80 and -70 dBW -- which of them a stream finds is its own threshold's business
    bufs = []
    for s in range(3):
        x = sc.noise(2 * n, 30 + s)
        for j, dbw in enumerate((-90.0, -80.0, -70.0)):
            x += sc.tone(2 * n, nperseg, 30 + 40 * j + s, 20 + 30 * j, 14, dbw=dbw)
        x += sc.tone(2 * n, nperseg, 200, 228, 12)  # across the cut between the two calls (234 segments each)
        bufs.append(x)
    calls = [np.stack([v[:n] for v in bufs]), np.stack([v[n:] for v in bufs])]
    kws = [dict(signal_threshold_dbw=thr[s], calibration_db=cal[s], snr_threshold_db=snr[s], signal_min_duration_ms=lo[s],
                signal_max_duration_ms=hi[s]) for s in range(3)]
    assert all(sc.clear_of_thresholds(c[s], nperseg, **kws[s]) for c in calls for s in range(3))
    oas = [oracle.OracleAnalyzer(sample_rate=FS, **kws[s]) for s in range(3)]
    b = BatchSignalAnalyzer(["a", "b", "c"], precision="float64", f64_sparse=True, sdr_callback_length=n, sample_rate=FS,
                            signal_threshold_dbw=thr, calibration_db=cal, snr_threshold_db=snr, signal_min_duration_ms=lo,
                            signal_max_duration_ms=hi)
    try:
        counts = []
        b.enqueue(calls[0])
        rec = b.fetch_records()
        for s in range(3):
            w = oas[s].process(calls[0][s], fc.TS0)
            _check_signals(rec[rec["stream"] == s], w, cal[s])
            counts.append(len(w[0]))
        assert counts[0] > counts[1] > counts[2] > 0  # (the emission followed each stream's own threshold)
        # stream 1's threshold changes: its look-back starts again, the others keep theirs
        thr2 = [oracle.db_to_linear(thr[s] + cal[s]) for s in range(3)]
        thr2[1] = oracle.db_to_linear(-84.0 + cal[1])
        b.native.set_stream_params(np.array(thr2, dtype=np.float64), np.array(cal, dtype=np.float64))
        kws[1]["signal_threshold_dbw"] = -84.0
        oas[1] = oracle.OracleAnalyzer(sample_rate=FS, **kws[1])
        assert sc.clear_of_thresholds(calls[1][1], nperseg, **kws[1])
        b.enqueue(calls[1])
        rec = b.fetch_records()
        back = []
        for s in range(3):
            w = oas[s].process(calls[1][s], fc.TS0)
            _check_signals(rec[rec["stream"] == s], w, cal[s])
            back.append(any(x.start < 0 for x in w[0]))
        assert back == [True, False, True]
    finally:
        b.close()


# ---- 8. absent streams ----
def test_absent_streams():
    nperseg, n = 256, 45000
    bufs = []
    for s in range(4):
        x = sc.noise(3 * n, 60 + s) + sc.tone(3 * n, nperseg, 50 + s, 60, 14)
        # pulses that end just behind the start of the second and of the third call (175 segments each, 200 samples dropped)
        for cut in (n, 2 * n):
            k = np.arange(cut - 2500, cut + 2000)
            x[k] += sc.tone_at(k, nperseg, 120 + s)
        bufs.append(x)
    calls = [np.stack([v[i * n:(i + 1) * n] for v in bufs]) for i in range(3)]
    assert all(sc.clear_of_thresholds(c[s], nperseg) for c in calls for s in range(4))
    masked = _analyzer(4, n, nperseg, row_means=True)
    twin = _analyzer(4, n, nperseg, row_means=True)
    try:
        recs, means = [], []
        for k, c in enumerate(calls):
            masked.set_present([True, False, True, False] if k == 1 else None)
            for b in (masked, twin):
                b.enqueue(c)
            recs.append((masked.fetch_records(), twin.fetch_records()))
            means.append((masked.fetch_row_means(), twin.fetch_row_means()))
        for k in range(3):
            m, t = recs[k]
            for s in (0, 2):  # the present streams: the twin's bytes
                assert m[m["stream"] == s].tobytes() == t[t["stream"] == s].tobytes(), (k, s)
                assert means[k][0][s].tobytes() == means[k][1][s].tobytes(), (k, s)
        m1 = recs[1][0]
        assert not np.any((m1["stream"] == 1) | (m1["stream"] == 3)) and np.isnan(means[1][0][[1, 3]]).all()
        # the absent streams' third buffer looks back into their first one
        for s in (1, 3):
            oa = oracle.OracleAnalyzer(sample_rate=FS)
            oa.process(calls[0][s], fc.TS0)
            w = oa.process(calls[2][s], fc.TS0)
            m2 = recs[2][0]
            _check_signals(m2[m2["stream"] == s], w)
            assert means[2][0][s].tobytes() == means[2][1][s].tobytes()
    finally:
        masked.close()
        twin.close()


# ---- 9. non-finite input ----
@pytest.mark.parametrize("nperseg", [256, 32])
@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
def test_nonfinite_sample(bad, nperseg):
    segs = int(np.ceil(0.008 * FS / nperseg)) + 4  # a pulse the duration gate passes
    T = 6 * segs
    n = T * nperseg
    clean = np.stack([sc.noise(n, 80 + s) + sc.tone(n, nperseg, 3 + s, segs, segs) for s in range(4)])
    assert all(sc.clear_of_thresholds(clean[s], nperseg) for s in range(4))
    poisoned = clean.copy()
    at = (4 * segs) * nperseg + nperseg // 3
    poisoned[2, at] = complex(bad, 0.0)
    kw = dict(hot_capacity=max(1024, 4 * nperseg))  # the poisoned column's 2 N cells (the segment and the one before it)
    b, twin = _analyzer(4, n, nperseg, **kw), _analyzer(4, n, nperseg, **kw)
    try:
        for h, v in ((b, poisoned), (twin, clean)):
            h.enqueue(v)
        got, ref = b.fetch_records(), twin.fetch_records()
        assert _is_sparse(b)
        for s in (0, 1, 3):
            assert got[got["stream"] == s].tobytes() == ref[ref["stream"] == s].tobytes(), s
        with np.errstate(all="ignore"):
            oa = oracle.OracleAnalyzer(sample_rate=FS, fft_nperseg=nperseg)
            w = oa.process(poisoned[2], fc.TS0)
            mine = got[got["stream"] == 2]
            assert len(w[0]) >= 1 and np.isnan([s.noise for s in w[0]]).all()
            _check_signals(mine, w)
        for h in (b, twin):  # the following call
            h.enqueue(clean)
        assert b.fetch_records().tobytes() == twin.fetch_records().tobytes()
    finally:
        b.close()
        twin.close()


# ---- 10. capacity ----
def test_record_capacity_grows():
    nperseg, n = 256, 300000
    for seed in range(sc.CANDIDATES):
        x = sc.pulses(n, FS, nperseg, "hamming", 40 + seed)
        rng = np.random.default_rng(9)
        w = oracle.window_coefficients("hamming", nperseg)
        amp = np.sqrt(10 ** (-60 / 10) * FS * (w * w).sum()) / w.sum()
        for k0 in range(0, n - 6000, 9000):  # hundreds of plateaus: a pulse train in many bins
            fb = int(rng.integers(1, 250))
            k = np.arange(4000)
            x[k0:k0 + 4000] += amp * np.exp(2j * np.pi * fb * (k0 + k) / nperseg)
        if sc.clear_of_thresholds(x, nperseg):
            break
    else:
        pytest.fail("no seed clear of its thresholds")
    want, _ = fc.oracle_records(x)
    assert len(want) >= 30
    b = _analyzer(1, n, nperseg, record_capacity=4)
    try:
        b.enqueue(x[None, :])
        rec = b.fetch_records()
        assert _is_sparse(b)
    finally:
        b.close()
    _check(rec, want)


def test_hot_capacity_overflow():
    nperseg, n = 256, 60000
    quiet = [sc.noise(2 * n, 90 + s) + sc.tone(2 * n, nperseg, 70 + s, 100, 14) + sc.tone(2 * n, nperseg, 170 + s, 334, 14) for s in range(2)]
    assert all(sc.clear_of_thresholds(q[i * n:(i + 1) * n], nperseg) for q in quiet for i in range(2))
    loud = quiet[0][:n].copy()
    w = oracle.window_coefficients("hamming", nperseg)
    sigma = np.sqrt(10 ** (-87 / 10) * FS / 2)  # white noise whose density sits 3 dB over the -90 dBW threshold
    rng = np.random.default_rng(91)
    loud += sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    b = _analyzer(2, n, nperseg, hot_capacity=1024)
    try:
        b.enqueue(np.stack([loud, quiet[1][:n]]))
        with pytest.raises(_native.NativeError) as ei:
            b.fetch_records()
        assert ei.value.code == _native.RT_E_HOT_OVERFLOW
        # the call is consumed; the next clean call is served, the neighbour's records (its look-back is the overflowed call's) right
        b.enqueue(np.stack([quiet[0][n:], quiet[1][n:]]))
        rec = b.fetch_records()
        assert _is_sparse(b)
        oa = oracle.OracleAnalyzer(sample_rate=FS)
        oa.process(quiet[1][:n], fc.TS0)
        _check_signals(rec[rec["stream"] == 1], oa.process(quiet[1][n:], fc.TS0))
        fresh = oracle.OracleAnalyzer(sample_rate=FS).process(quiet[0][n:], fc.TS0)
        assert len(fresh[0]) >= 1 and all(s.start >= 0 for s in fresh[0])
        _check_signals(rec[rec["stream"] == 0], fresh)
    finally:
        b.close()


# ---- 11. against the dense handle ----
def test_against_the_dense_handle():
    nperseg = 256
    x = np.stack([sc.size_buffer(nperseg, w, sc.SIZE_SEEDS[(nperseg, w, c)]) for w, c in sc.WINDOWS[:1] * 2 + sc.WINDOWS[:1]])
    x[1] = sc.pulses(x.shape[1], FS, nperseg, "hamming", 77)
    x[2] = sc.pulses(x.shape[1], FS, nperseg, "hamming", 78)
    assert all(sc.clear_of_thresholds(v, nperseg) for v in x)
    out = []
    for sparse in (True, True, False):
        b = _analyzer(3, x.shape[1], nperseg, sparse=sparse, row_means=True)
        try:
            b.enqueue(x)
            rec = b.fetch_records()
            assert _is_sparse(b) == sparse
            out.append((rec, b.fetch_row_means()))
        finally:
            b.close()
    (r0, m0), (r1, m1), (rd, md) = out
    assert r0.tobytes() == r1.tobytes() and m0.tobytes() == m1.tobytes()  # two runs: the same bytes
    assert len(rd) >= 6
    for f in ("stream", "fi", "start", "end", "shadowed"):
        assert np.array_equal(r0[f], rd[f]), f
    for f in ("max_p", "mean_p", "row_mean"):
        np.testing.assert_allclose(oracle.to_db(r0[f]), oracle.to_db(rd[f]), rtol=0, atol=DB_TOL)
    np.testing.assert_allclose(r0["std_db"], rd["std_db"], rtol=0, atol=STD_TOL)
    np.testing.assert_allclose(oracle.to_db(m0), oracle.to_db(md), rtol=0, atol=DB_TOL)


# ---- 12. no map ----
def test_no_map_is_allocated():
    import torch

    def taken(sparse):
        torch.cuda.synchronize()
        free0, _ = torch.cuda.mem_get_info()
        b = _analyzer(8, 2 ** 21, 256, sparse=sparse)
        torch.cuda.synchronize()
        free1, _ = torch.cuda.mem_get_info()
        b.close()
        return free0 - free1

    torch.zeros(1, device="cuda")  # (the context's own memory first)
    sparse, dense = taken(True), taken(False)
    assert dense >= 128 << 20, dense  # the map is 8 x 2^21 x 8 B: the method sees it
    assert sparse < 64 << 20, sparse


# ---- 13. drop-in ----
def test_signal_analyzer_drop_in():
    import queue

    import torch

    x = fc.threshold_buffer(sc.THRESHOLD_SEEDS[0])
    ts = datetime.datetime(2024, 1, 1, tzinfo=datetime.timezone.utc)
    _, kept = oracle.OracleAnalyzer().process(x, ts)
    assert len(kept) >= 1
    q = queue.Queue()
    sa = SignalAnalyzer("0", precision="float64", f64_sparse=True, signal_queue=q, sdr_callback_length=len(x))
    dense = SignalAnalyzer("0", precision="float64", signal_queue=queue.Queue(), sdr_callback_length=len(x))
    try:
        sa.process_samples(x)
        got = []
        while not q.empty():
            m = q.get()
            if hasattr(m, "frequency"):
                got.append(m)
        assert sa._batch.call_info().mode_used == _native.RT_MODE_SPARSE
        assert [(s.frequency, s.duration) for s in got] == [(k.frequency, k.duration) for k in kept]
        for g, k in zip(got, kept):
            assert abs(g.max - k.max) < DB_TOL and abs(g.avg - k.avg) < DB_TOL and abs(g.snr - k.snr) < DB_TOL
            assert abs(g.noise - k.noise) < DB_TOL and abs(g.std - k.std) < STD_TOL
        sa._batch.reset_stream(0)
        again = sa.analyze_buffer(x, ts)
        assert [(s.frequency, s.ts, s.duration) for s in again] == [(k.frequency, k.ts, k.duration) for k in kept]
        # rt_extract_f64 and rt_spectrogram_f64 work on caller-supplied memory: the sparse handle gives what the dense one gives
        freqs, times, spec = oracle.stft_power(x, fc.FS, "hamming", fc.NPERSEG)
        ex, exd = sa.extract_signals(freqs, times, spec, ts), dense.extract_signals(freqs, times, spec, ts)
        assert len(ex) >= 1 and [(e.frequency, e.ts, e.duration, e.max, e.avg, e.std, e.noise, e.snr) for e in ex] == \
            [(e.frequency, e.ts, e.duration, e.max, e.avg, e.std, e.noise, e.snr) for e in exd]
        d = torch.from_numpy(x[None, :].copy()).cuda()
        T = len(x) // fc.NPERSEG
        maps = []
        for a in (sa, dense):
            out = torch.zeros((1, T, fc.NPERSEG), dtype=torch.float64, device="cuda")
            a._batch.native.spectrogram_device(d.data_ptr(), len(x), len(x), out.data_ptr())
            maps.append(out.cpu().numpy())
        assert maps[0].tobytes() == maps[1].tobytes() and maps[0].max() > 0
    finally:
        sa._batch.close()
        dense._batch.close()
