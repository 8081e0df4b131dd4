"""RT_FLAG_F64_RESCUE on the GPU (precision="float64", f64_sparse=True, f64_rescue=True): a stream that emits more candidate
cells than hot_capacity is analysed again on its own inside the fetch, from a float64 map the scan's own arithmetic fills.
Without the flag each of these calls ends in RT_E_HOT_OVERFLOW (tests/test_gpu_f64_sparse.py::test_hot_capacity_overflow).
Byte comparisons run GPU against GPU; every comparison against the oracle first asserts on the CPU that its input is clear of
its thresholds (tests/f64_sparse_cases.py).  Tolerances: tests/test_gpu_float64_path.py."""
import numpy as np
import pytest

from oracle import analyze_oracle as oracle
from pyradiotracking_amd import _native, synth
from pyradiotracking_amd.analyze import BatchSignalAnalyzer
from tests import f64_sparse_cases as sc
from tests import float64_cases as fc

pytestmark = pytest.mark.gpu

DB_TOL = 1e-9   # max / avg / noise / snr, dB
STD_TOL = 1e-5  # std, dB
FS = sc.FS
HOT_MIN = 1024


@pytest.fixture(autouse=True)
def _need_gpu():
    if _native.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")


def _keys(rec):
    return [(int(r["fi"]), int(r["start"]), int(r["end"])) for r in rec]


def _check_signals(rec, want, cal=0.0):
    """rt_record_f64 rows of one stream against OracleSignals (OracleAnalyzer.process: every signal, with the kept ones)."""
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


def _analyzer(n_streams, n, nperseg=256, rescue=True, **kw):
    kw.setdefault("hot_capacity", HOT_MIN)
    return BatchSignalAnalyzer([str(i) for i in range(n_streams)], precision="float64", f64_sparse=True, f64_rescue=rescue,
                               sdr_callback_length=n, fft_nperseg=nperseg, sample_rate=FS, **kw)


def _info(b):
    i = b.call_info()
    return i.mode_used, i.n_dense_streams, i.fell_back


def white(n, seed, density_dbw):
    """White complex noise whose power density (a spectrogram cell's mean) is ``density_dbw``."""
    rng = np.random.default_rng([4180, seed])
    sigma = np.sqrt(10 ** (density_dbw / 10) * FS / 2)
    return sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))


def emitted(x, nperseg, thr_dbw=-90.0, window="hamming"):
    """Cells the scan's emission rule takes of ``x``: not below the threshold, or directly before one that is not."""
    _, _, spec = oracle.stft_power(x, FS, window, nperseg)  # [F][T]
    hot = ~(spec < oracle.db_to_linear(thr_dbw))
    need = hot.copy()
    need[:, :-1] |= hot[:, 1:]
    return int(need.sum())


def first_clear(make, check, tries=sc.CANDIDATES * 2):
    """``make(seed)`` for the first seed whose buffers all pass ``check`` (clear of their thresholds)."""
    for seed in range(tries):
        v = make(seed)
        if check(v):
            return v
    pytest.fail("no seed clear of its thresholds")


# ---- 1. rescued = un-overflowed, byte for byte ----
# (nperseg, T): T = 3 (mod 5) and no multiple of the group G = 1024 / nperseg: several chunks of 5 segments, a ragged last chunk and a
# ragged last group; at least five times a pulse the duration gate passes, so that its cells stand 5 dB over their row's mean
SHAPES = [(32, 473), (64, 253), (128, 143), (256, 83), (512, 73), (1024, 73), (2048, 73), (4096, 73)]


def _sizes_row(nperseg, T, seed):
    n = T * nperseg + nperseg // 2  # (a remainder the analysis drops)
    # noise under the threshold: about 1 500 of the T * nperseg cells over it, twice as many emitted
    p_hot = 1500.0 / (T * nperseg)
    x = white(n, 100 * nperseg + seed, -90.0 - 10 * np.log10(-np.log(p_hot)))
    segs = int(np.ceil(0.008 * FS / nperseg)) + 4
    for j, fi in enumerate((3, nperseg // 2 + 1, nperseg - 5)):
        x += sc.tone(n, nperseg, fi, 2 + j * (segs // 3), segs)
    return x


@pytest.mark.parametrize("nperseg,T", SHAPES, ids=[str(n) for n, _ in SHAPES])
def test_rescued_equals_unoverflowed(nperseg, T):
    G = max(1, 1024 // nperseg)
    assert T % 5 == 3 and (G == 1 or T % G != 0)
    x = first_clear(lambda seed: _sizes_row(nperseg, T, seed), lambda v: sc.clear_of_thresholds(v, nperseg))
    cells = emitted(x, nperseg)
    assert HOT_MIN + 1 <= cells <= 8192, cells
    out = []
    for rescue, cap in ((False, 8192), (True, HOT_MIN)):
        b = _analyzer(1, len(x), nperseg, rescue=rescue, hot_capacity=cap, segs_per_chunk=5, row_means=True)
        try:
            b.enqueue(x[None, :])
            rec = b.fetch_records()
            out.append((rec, b.fetch_row_means(), _info(b), int(b.call_info().n_hot)))
        finally:
            b.close()
    (ra, ma, ia, _), (rb, mb, ib, hot_b) = out
    assert ia == (_native.RT_MODE_SPARSE, 0, 0)
    assert ib == (_native.RT_MODE_SPARSE, 1, 1)
    assert hot_b == cells  # (the counter, not the 1 024 cells stored -- and the GPU's cells decide as the oracle's do)
    assert len(ra) >= 1
    assert rb.tobytes() == ra.tobytes()
    assert mb.tobytes() == ma.tobytes()


# ---- 2. against the oracle over a sequence ----
def _sequence(seed):
    """Three streams x three calls of 60 000 samples.  Stream 1: white noise 3 dB over the threshold in calls 1 and 2, a pulse
    across the cut between them, quiet in call 3 with a pulse across the cut into it; streams 0 and 2 quiet, with pulses."""
    nperseg, n = 256, 60000
    rows = []
    for s in range(3):
        x = sc.noise(3 * n, 200 + 10 * seed + s)
        x += sc.tone(3 * n, nperseg, 40 + 9 * s, 50, 14) + sc.tone(3 * n, nperseg, 120 + 9 * s, 300, 14) + sc.tone(3 * n, nperseg, 200 + 9 * s, 560, 14)
        if s == 1:
            x[:2 * n] += white(2 * n, 300 + seed, -87.0)
            for cut, fi in ((n, 77), (2 * n, 177)):
                k = np.arange(cut - 2500, cut + 2000)
                x[k] += sc.tone_at(k, nperseg, fi)
        rows.append(x)
    return [np.stack([v[i * n:(i + 1) * n] for v in rows]) for i in range(3)]


def test_sequence_against_the_oracle():
    calls = first_clear(_sequence, lambda cs: all(sc.clear_of_thresholds(c[s]) for c in cs for s in range(3)))
    assert emitted(calls[0][1], 256) > 8192 and emitted(calls[1][1], 256) > 8192
    assert all(emitted(c[s], 256) < HOT_MIN for c in calls for s in (0, 2)) and emitted(calls[2][1], 256) < HOT_MIN
    oas = [oracle.OracleAnalyzer(sample_rate=FS) for _ in range(3)]
    want = [[oas[s].process(c[s], fc.TS0) for s in range(3)] for c in calls]
    assert any(x.start < 0 for x in want[1][1][0])  # inside a rescued call: a plateau that began in the call before
    assert any(x.start < 0 for x in want[2][1][0])  # from a normal call back into a rescued call's tail
    assert all(len(want[k][s][0]) >= 1 for k in range(3) for s in range(3))
    b = _analyzer(3, 60000)
    try:
        dense = []
        for k, c in enumerate(calls):
            b.enqueue(c)
            rec = b.fetch_records()
            mode, n_dense, fell = _info(b)
            assert mode == _native.RT_MODE_SPARSE and fell == (1 if n_dense else 0)
            dense.append(n_dense)
            for s in range(3):
                _check_signals(rec[rec["stream"] == s], want[k][s])
        assert dense == [1, 1, 0]
    finally:
        b.close()


# ---- 3. integer formats ----
def u8_to_complex128(raw):
    """What a float64 handle makes of wire bytes (include/rt_analyze.h): (double)b / 127.5 - 1.0 per component, a real division.
    (NumPy's complex ``iq /= 127.5`` multiplies by a rounded reciprocal instead: the last bit of some bytes' values differs.)"""
    v = np.asarray(raw, dtype=np.float64) / 127.5 - 1.0
    out = np.empty(v.shape[:-1] + (v.shape[-1] // 2,), dtype=np.complex128)
    out.real = v[..., 0::2]
    out.imag = v[..., 1::2]
    return out


@pytest.mark.parametrize("fmt", ["u8", "i16", "i8"])
def test_integer_formats(fmt):
    nperseg, n = 256, 150000
    x = sc.pulses(n, FS, nperseg, "hamming", 510, sigma=0.05)
    x = x / np.abs(x).max() * 0.9
    quantize, convert = {"u8": (synth.quantize_u8, u8_to_complex128), "i16": (synth.quantize_i16, synth.i16_to_complex128),
                         "i8": (synth.quantize_i8, synth.i8_to_complex128)}[fmt]
    raw = quantize(x)
    ref = convert(raw)
    assert emitted(ref, nperseg, -60.0) > HOT_MIN
    out = []
    for integer in (True, False):
        b = _analyzer(1, n, nperseg, signal_threshold_dbw=-60.0, row_means=True)
        try:
            if integer:
                {"u8": b.enqueue_bytes, "i16": b.enqueue_int16, "i8": b.enqueue_int8}[fmt](raw[None, :])
            else:
                b.enqueue(ref[None, :])
            rec = b.fetch_records()
            assert _info(b) == (_native.RT_MODE_SPARSE, 1, 1)
            out.append((rec, b.fetch_row_means()))
        finally:
            b.close()
    assert len(out[0][0]) >= 1
    assert out[0][0].tobytes() == out[1][0].tobytes()
    assert out[0][1].tobytes() == out[1][1].tobytes()


# ---- 4. per-stream values, absence ----
def test_own_threshold_overflows():
    """Two streams of the same noise, 10 dB under the handle's threshold: stream 1's own threshold lies 3 dB under that noise."""
    nperseg, n = 256, 60000
    thr = [-90.0, -103.0]

    def make(seed):
        return np.stack([white(n, 400 + 2 * seed + s, -100.0) + sc.tone(n, nperseg, 60 + s, 40, 14) + sc.tone(n, nperseg, 160 + s, 150, 14)
                         for s in range(2)])

    x = first_clear(make, lambda v: all(sc.clear_of_thresholds(v[s], nperseg, signal_threshold_dbw=thr[s]) for s in range(2)))
    assert emitted(x[0], nperseg, thr[0]) < HOT_MIN < 8192 < emitted(x[1], nperseg, thr[1])
    b = _analyzer(2, n, nperseg, signal_threshold_dbw=thr)
    try:
        b.enqueue(x)
        rec = b.fetch_records()
        assert _info(b) == (_native.RT_MODE_SPARSE, 1, 1)
    finally:
        b.close()
    for s in range(2):
        want = oracle.OracleAnalyzer(sample_rate=FS, signal_threshold_dbw=thr[s]).process(x[s], fc.TS0)
        assert len(want[0]) >= 2
        _check_signals(rec[rec["stream"] == s], want)


def test_absent_stream_is_not_rescued():
    """Call 1: stream 0 loud and present (rescued), stream 1 loud and absent (not touched).  Call 2: stream 1 looks back into call 0."""
    nperseg, n = 256, 45000

    def make(seed):
        rows = []
        for s in range(2):
            x = sc.noise(3 * n, 500 + 2 * seed + s) + sc.tone(3 * n, nperseg, 50 + s, 60, 14) + sc.tone(3 * n, nperseg, 90 + s, 400, 14)
            k = np.arange(2 * n - 2500, 2 * n + 2000)  # ends just behind the start of the third call
            x[k] += sc.tone_at(k, nperseg, 120 + s)
            rows.append(x)
        rows[0][n:2 * n] += white(n, 520 + seed, -87.0)
        # stream 1's radio delivered nothing in call 1: its third buffer follows its first
        third = rows[1][2 * n:].copy()
        k = np.arange(n - 2500, n)
        rows[1][k] += sc.tone_at(k + n, nperseg, 121)  # (the pulse's first part, as if the second buffer had never been)
        calls = [np.stack([v[i * n:(i + 1) * n] for v in rows]) for i in range(3)]
        calls[2][1] = third
        calls[1][1] = white(n, 540 + seed, -80.0)  # what lies in the absent stream's row: loud, never analysed
        return calls

    calls = first_clear(make, lambda cs: all(sc.clear_of_thresholds(cs[k][s], nperseg) for k, s in ((0, 0), (0, 1), (1, 0), (2, 0), (2, 1))))
    assert emitted(calls[1][0], nperseg) > 8192 and emitted(calls[1][1], nperseg) > 8192
    oas = [oracle.OracleAnalyzer(sample_rate=FS) for _ in range(2)]
    want = {(k, s): oas[s].process(calls[k][s], fc.TS0) for k in range(3) for s in range(2) if (k, s) != (1, 1)}
    assert any(x.start < 0 for x in want[(2, 1)][0])
    b = _analyzer(2, n, nperseg, row_means=True)
    try:
        for k in range(3):
            b.set_present([True, False] if k == 1 else None)
            b.enqueue(calls[k])
            rec = b.fetch_records()
            means = b.fetch_row_means()
            assert _info(b) == ((_native.RT_MODE_SPARSE, 1, 1) if k == 1 else (_native.RT_MODE_SPARSE, 0, 0))
            for s in range(2):
                if (k, s) == (1, 1):
                    assert not np.any(rec["stream"] == 1) and np.isnan(means[1]).all()
                else:
                    _check_signals(rec[rec["stream"] == s], want[(k, s)])
                    assert np.isfinite(means[s]).all()
    finally:
        b.close()


# ---- 5. rounds ----
def test_more_streams_than_a_round_holds():
    """int8 at nperseg 4096, T = 64: a map of 2 MiB a stream, 128 of them in the scratch -- 129 streams of one row."""
    nperseg, T = 4096, 64
    n = T * nperseg
    per_round = (256 << 20) // (T * nperseg * 8)  # rt_core.h: f64_rescue_rounds (tests/test_f64_rescue_contract.py)
    assert per_round == 128
    S = per_round + 1
    rng = np.random.default_rng(55)
    x = 0.25 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))  # full-scale noise: -63.8 dBW a cell
    k = np.arange(20 * nperseg, 21 * nperseg)
    x[k] += 0.4 * np.exp(2j * np.pi * 1000 * k / nperseg)
    row = synth.quantize_i8(x)
    raw = np.ascontiguousarray(np.broadcast_to(row, (S, row.size)))
    # (an SNR threshold of 15 dB: no cell of the noise stands that far over its row's mean, the tone's does)
    b = _analyzer(S, n, nperseg, signal_threshold_dbw=-66.0, snr_threshold_db=15.0)
    try:
        b.enqueue_int8(raw)
        rec = b.fetch_records()
        assert _info(b) == (_native.RT_MODE_SPARSE, S, 1)
    finally:
        b.close()
    first = rec[rec["stream"] == 0]
    assert len(first) >= 1 and len(rec) == S * len(first)
    for s in range(1, S):
        mine = rec[rec["stream"] == s].copy()
        mine["stream"] = 0
        assert mine.tobytes() == first.tobytes(), s


# ---- 6. record growth ----
def test_record_capacity_grows_in_a_rescued_call():
    nperseg, n = 256, 300000

    def make(seed):
        x = sc.pulses(n, FS, nperseg, "hamming", 40 + seed) + white(n, 600 + seed, -87.0)
        rng = np.random.default_rng(9)
        w = oracle.window_coefficients("hamming", nperseg)
        amp = np.sqrt(10 ** (-60 / 10) * FS * (w * w).sum()) / w.sum()
        for k0 in range(0, n - 6000, 9000):  # a pulse train in many bins (tests/test_gpu_f64_sparse.py::test_record_capacity_grows)
            fb = int(rng.integers(1, 250))
            k = np.arange(4000)
            x[k0:k0 + 4000] += amp * np.exp(2j * np.pi * fb * (k0 + k) / nperseg)
        return x

    x = first_clear(make, lambda v: sc.clear_of_thresholds(v, nperseg))
    assert emitted(x, nperseg) > 8192
    want = oracle.OracleAnalyzer(sample_rate=FS).process(x, fc.TS0)
    assert len(want[0]) >= 30
    b = _analyzer(1, n, nperseg, record_capacity=4)
    try:
        b.enqueue(x[None, :])
        rec = b.fetch_records()
        assert _info(b) == (_native.RT_MODE_SPARSE, 1, 1)
    finally:
        b.close()
    _check_signals(rec, want)


# ---- 7. two calls in flight ----
def test_two_calls_in_flight():
    nperseg, n = 256, 60000
    rows = [sc.noise(2 * n, 700 + s) + sc.tone(2 * n, nperseg, 30 + s, 100, 14) + sc.tone(2 * n, nperseg, 130 + s, 334, 14) for s in range(3)]
    for s in range(3):
        k = np.arange(n - 2500, n + 2000)
        rows[s][k] += sc.tone_at(k, nperseg, 220 + s)
    rows[1][:n] += white(n, 710, -87.0)
    rows[2][n:] += white(n, 711, -87.0)
    calls = [np.stack([v[:n] for v in rows]), np.stack([v[n:] for v in rows])]
    assert emitted(calls[0][1], nperseg) > HOT_MIN and emitted(calls[1][2], nperseg) > HOT_MIN
    flight, single = _analyzer(3, n, nperseg, row_means=True), _analyzer(3, n, nperseg, row_means=True)
    try:
        flight.enqueue(calls[0])
        flight.enqueue(calls[1])
        got = []
        for k in range(2):
            got.append((flight.fetch_records(), flight.fetch_row_means(), _info(flight)))
        ref = []
        for k in range(2):
            single.enqueue(calls[k])
            ref.append((single.fetch_records(), single.fetch_row_means(), _info(single)))
    finally:
        flight.close()
        single.close()
    for k in range(2):
        assert got[k][2] == ref[k][2] == (_native.RT_MODE_SPARSE, 1, 1)
        assert len(ref[k][0]) >= 3
        assert got[k][0].tobytes() == ref[k][0].tobytes(), k
        assert got[k][1].tobytes() == ref[k][1].tobytes(), k
    assert np.any(ref[1][0]["start"] < 0)


# ---- 8. a NaN sample in a rescued stream ----
def test_nan_sample_in_a_rescued_stream():
    nperseg, n = 256, 30000

    def make(seed):
        x = np.stack([sc.noise(n, 800 + 3 * seed + s) + sc.tone(n, nperseg, 20 + s, 30, 14) for s in range(3)])
        x[1] += white(n, 830 + seed, -87.0)
        return x

    clean = first_clear(make, lambda v: all(sc.clear_of_thresholds(v[s], nperseg) for s in range(3)))
    assert emitted(clean[1], nperseg) > 8192
    poisoned = clean.copy()
    poisoned[1, 70 * nperseg + nperseg // 3] = complex(np.nan, 0.0)
    b, twin = _analyzer(3, n, nperseg), _analyzer(3, n, nperseg)
    try:
        b.enqueue(poisoned)
        twin.enqueue(clean)
        got, ref = b.fetch_records(), twin.fetch_records()
        assert _info(b) == _info(twin) == (_native.RT_MODE_SPARSE, 1, 1)
    finally:
        b.close()
        twin.close()
    for s in (0, 2):
        assert len(ref[ref["stream"] == s]) >= 1
        assert got[got["stream"] == s].tobytes() == ref[ref["stream"] == s].tobytes(), s
    with np.errstate(all="ignore"):
        w = oracle.OracleAnalyzer(sample_rate=FS).process(poisoned[1], fc.TS0)
        assert len(w[0]) >= 1 and np.isnan([s.noise for s in w[0]]).all()
        _check_signals(got[got["stream"] == 1], w)


# ---- 9. no scratch before a stream overflows ----
def test_no_scratch_without_an_overflow():
    """tests/test_gpu_f64_sparse.py::test_no_map_is_allocated for a flag handle, a clean call included: neither the float64 map
    (8 x 2^21 x 8 B = 128 MiB) nor the rescue scratch is there."""
    import torch

    n = 2 ** 21
    x = torch.zeros((8, n), dtype=torch.complex128, device="cuda")
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    b = _analyzer(8, n, 256)
    try:
        b.enqueue(x)
        b.fetch_records()
        assert _info(b) == (_native.RT_MODE_SPARSE, 0, 0)
        torch.cuda.synchronize()
        free1, _ = torch.cuda.mem_get_info()
    finally:
        b.close()
    assert free0 - free1 < 64 << 20, free0 - free1
