"""The float32 round-off model of ``tests/precision64.py`` on the CPU: honest float32 arithmetic (SciPy's pocketfft through
the oracle, and NumPy restatements of the kernels' other forms) stays inside it, and results that are subtly wrong do not.
``python -m tests.test_precision_model`` prints the worst ratio per transform family (the SciPy column of the profile)."""
import math

import numpy as np
import pytest
import scipy.fft

from oracle import analyze_oracle as oracle
from pyradiotracking_amd import synth
from tests import precision64 as p64

FS = 2048000
KAISER = ("kaiser-array", None)  # the kaiser window passed as a coefficient array
WINDOWS = ("hann", "hamming", "blackmanharris", KAISER, ("tukey", 0.3))
INPUTS = ("clean", "dc2e-3", "dc60", "dc80", "tones80")

# every size of every transform family the GPU tests cover
SIZES = {
    "general": (8, 16),
    "scan_lanegroups": (32, 64, 128),
    "scan": (256, 512, 1024, 2048),
    "scan64": (4096,),
    "wg": (8192, 16384),
    "bluestein": (9, 17, 129, 257, 300, 1000, 1025, 2049, 4097, 8191),
}
FAMILY = {n: f for f, ns in SIZES.items() for n in ns}


def window_arg(window, nperseg):
    if window is KAISER or window == KAISER:
        return oracle.window_coefficients(("kaiser", 8.0), nperseg)
    return window


def make_input(kind, nperseg, T, window, seed):
    """One stream of T segments (plus a ragged tail).  Noise sigma 1e-5 per component; ``dc60`` / ``dc80``: the offset
    0.1 - 0.07j at 60 / 80 dB over the noise's per-sample power; ``tones80``: pulses 80 dB over the noise level of a bin."""
    rng = np.random.default_rng(seed)
    n = T * nperseg + nperseg // 3
    w = oracle.window_coefficients(window, nperseg)
    sigma = synth.NOISE_SIGMA
    dc = 0j
    if kind == "dc2e-3":
        dc = complex(2e-3, -1e-3)
    elif kind in ("dc60", "dc80"):
        dc = complex(0.1, -0.07)
        sigma = abs(dc) / math.sqrt(2.0 * 10.0 ** ((60 if kind == "dc60" else 80) / 10.0))
    noise_db = 10 * math.log10(2 * sigma ** 2 / FS)
    pulses = []
    if kind in ("tones80", "dc2e-3", "dc60") or T >= 40:
        hop_ms = 1e3 * nperseg / FS
        lo = max(0.5, 3 * hop_ms)
        dur = (lo, max(lo, min(30.0, 0.4 * T * hop_ms)))
        pulses = synth.random_pulses(rng, n, FS, w, 4, dur_ms=dur, peak_dbw=(noise_db + 60, noise_db + 80))
    return synth.make_stream(synth.StreamSpec(n, FS, pulses, noise_sigma=sigma, dc=dc), seed), noise_db


def analyzer_kwargs(nperseg, T, window, noise_db):
    hop_ms = 1e3 * nperseg / FS
    return dict(sample_rate=FS, fft_nperseg=nperseg, fft_window=window, signal_threshold_dbw=noise_db + 30,
                signal_min_duration_ms=min(8.0, 2.5 * hop_ms), signal_max_duration_ms=1e3 * T * hop_ms)


# ----------------------------------------------------------------------------------------------------------------------
# float32 restatements of the kernels' forms that SciPy does not compute
# ----------------------------------------------------------------------------------------------------------------------
def stft_f32(x, w32, scale32, mean_fn=None):
    """SciPy's float32 arithmetic (oracle.stft_power) with the window and scale given, optionally another segment mean."""
    N = len(w32)
    T = len(x) // N
    seg = x[: T * N].reshape(T, N)
    m = seg.mean(axis=1, keepdims=True) if mean_fn is None else mean_fn(seg)
    spec = scipy.fft.fft((seg - m) * w32.astype(np.complex64), axis=1)
    spec = np.conjugate(spec) * spec
    spec *= np.float32(scale32)
    return spec.real.astype(np.float32)


def stft_lin_f32(x, window, nperseg):
    """Detrend by linearity in float32: FFT(w x) - m W_k on bins 0 and +-1 (the fused scans' LIN form)."""
    w32 = p64.window_f32(window, nperseg).astype(np.float32)
    W = np.fft.fft(w32.astype(np.float64)).astype(np.complex64)
    T = len(x) // nperseg
    seg = x[: T * nperseg].reshape(T, nperseg)
    m = seg.mean(axis=1)
    X = scipy.fft.fft(seg * w32, axis=1)
    for k in (0, 1, nperseg - 1):
        X[:, k] -= m * W[k]
    return ((X.real ** 2 + X.imag ** 2) * np.float32(p64.scale_f32(window, nperseg, FS))).astype(np.float32)


def stft_bluestein_f32(x, window, nperseg):
    """Bluestein's algorithm in float32 as stft_bluestein runs it: window * sqrt(scale) * chirp folded into one table, a
    transform of length M, the product with the filter's transform (1/M folded in), a second transform of the conjugate."""
    N, M = nperseg, p64.bluestein_m(nperseg)
    w = p64.window_f32(window, N)
    n = np.arange(N, dtype=np.float64)
    ch = np.exp(-1j * np.pi * ((n * n) % (2 * N)) / N)
    cwin = (w * math.sqrt(p64.scale_f32(window, N, FS)) * ch).astype(np.complex64)
    filt = np.zeros(M, np.complex128)
    filt[:N] = np.conj(ch)
    filt[M - N + 1 :] = np.conj(ch[1:][::-1])
    bf = (np.fft.fft(filt) / M).astype(np.complex64)
    T = len(x) // N
    seg = x[: T * N].reshape(T, N)
    seg = seg - seg.mean(axis=1, keepdims=True)
    a = np.zeros((T, M), np.complex64)
    a[:, :N] = seg * cwin
    C = scipy.fft.fft(a, axis=1) * bf
    out = scipy.fft.fft(np.conj(C), axis=1)[:, :N]
    return (out.real ** 2 + out.imag ** 2).astype(np.float32)


# ----------------------------------------------------------------------------------------------------------------------
# the sweep: honest float32 passes
# ----------------------------------------------------------------------------------------------------------------------
def _sweep_cases():
    cases = []
    for i, (nperseg, fam) in enumerate(sorted(FAMILY.items())):
        for j in range(2):
            window = WINDOWS[(i + j) % len(WINDOWS)]
            kind = INPUTS[(2 * i + j) % len(INPUTS)]
            T = int(np.clip(600000 // nperseg, 2, 400)) if j == 0 else (2, 3, 17, 31, 40)[i % 5]
            cases.append((nperseg, window, kind, T))
    cases.append((256, "hamming", "tones80", 8000))
    cases.append((256, "hann", "dc80", 150))
    return cases


SWEEP = _sweep_cases()


def run_case(nperseg, window, kind, T, seed=0):
    """SciPy (and the restatements) against float64 on one case; returns {name: worst ratio} and the record ratios."""
    warg = window_arg(window, nperseg)
    x, noise_db = make_input(kind, nperseg, T, warg, seed + nperseg + 7 * T)
    ref = p64.stft_power_f64(x, FS, warg, nperseg)
    worst = {}
    _, _, sci = oracle.stft_power(x, FS, warg, nperseg)
    b_sub = p64.cell_bounds(ref, "sub", "direct")
    worst["scipy"] = float(p64.cell_ratios(sci.T, ref, b_sub).max())
    if nperseg & (nperseg - 1):
        worst["bluestein-f32"] = float(p64.cell_ratios(stft_bluestein_f32(x, warg, nperseg), ref, p64.cell_bounds(ref, "sub", "bluestein")).max())
    elif window in ("hann", "hamming"):
        worst["lin-f32"] = float(p64.cell_ratios(stft_lin_f32(x, warg, nperseg), ref, p64.cell_bounds(ref, "lin", "direct")).max())
    # records: two consecutive buffers (look-back), the oracle's own arithmetic
    half = (T // 2) * nperseg
    rec_worst = {}
    if T >= 4:
        oa = oracle.OracleAnalyzer(**analyzer_kwargs(nperseg, T // 2, warg, noise_db))
        prev = None
        for k in range(2):
            buf = x[k * half : (k + 1) * half]
            _, _, spec = oracle.stft_power(buf, FS, warg, nperseg)
            recs = oracle.extract_records(np.arange(spec.shape[1]) * nperseg / FS + nperseg / 2 / FS, spec, oa.spec_last, oa.params)
            oa.spec_last = spec
            r64 = p64.stft_power_f64(buf, FS, warg, nperseg)
            b64 = p64.cell_bounds(r64, "sub", "direct")
            fields = p64.oracle_record_fields(recs, spec, prev[0] if prev else None)
            chk = p64.check_records(fields, r64, b64, 32, prev[1] if prev else None, prev[2] if prev else None, what=f"buffer {k}")
            assert not chk.failures, "\n".join(chk.failures[:10])
            for f, v in chk.worst.items():
                rec_worst[f] = max(rec_worst.get(f, 0.0), v)
            rec_worst["n_records"] = rec_worst.get("n_records", 0) + len(recs)
            prev = (spec, r64, b64)
    return worst, rec_worst


@pytest.mark.parametrize("nperseg,window,kind,T", SWEEP, ids=[f"{n}-{w if isinstance(w, str) else w[0]}-{k}-T{t}" for n, w, k, t in SWEEP])
def test_float32_arithmetic_meets_the_model(nperseg, window, kind, T):
    worst, _ = run_case(nperseg, window, kind, T)
    for name, r in worst.items():
        assert r <= 1.0, f"{name}: worst cell at {r:.3f} of its bound"


def test_the_sweep_finds_records_and_the_model_is_not_slack():
    """The record checks above ran on records (look-back ones among them), and SciPy reaches a fair share of the cell bound
    somewhere in the sweep: the constants are not an order of magnitude over float32's own round-off."""
    n_rec, worst_cells, worst_rec = 0, 0.0, {}
    for case in SWEEP[::3] + SWEEP[-2:]:
        w, r = run_case(*case)
        worst_cells = max(worst_cells, w["scipy"])
        n_rec += r.get("n_records", 0)
        for f, v in r.items():
            if f != "n_records":
                worst_rec[f] = max(worst_rec.get(f, 0.0), v)
    assert n_rec > 100
    assert 0.1 < worst_cells <= 1.0
    assert all(0.0 < v <= 1.0 for v in worst_rec.values()), worst_rec


# ----------------------------------------------------------------------------------------------------------------------
# acceptance figures
# ----------------------------------------------------------------------------------------------------------------------
def test_row_mean_bound_at_config2_geometry_is_tighter_than_one_segment():
    T, N = 8000, 256
    x = synth.make_stream(synth.StreamSpec(T * N, FS, []), 5)
    ref = p64.stft_power_f64(x, FS, "hamming", N)
    bound = p64.row_mean_bound(ref, p64.cell_bounds(ref, "lin", "direct"), L=32)
    assert np.all(bound / ref.P.mean(axis=0) < 1.0 / (4 * T))


def test_max_bound_of_a_cell_20db_over_the_noise():
    N, T = 256, 200
    w = oracle.window_coefficients("hamming", N)
    noise_db = 10 * math.log10(2 * synth.NOISE_SIGMA ** 2 / FS)
    rng = np.random.default_rng(3)
    pulses = synth.random_pulses(rng, T * N, FS, w, 6, dur_ms=(1, 10), peak_dbw=(noise_db + 20, noise_db + 40))
    x = synth.make_stream(synth.StreamSpec(T * N, FS, pulses), 3)
    ref = p64.stft_power_f64(x, FS, "hamming", N)
    for form in ("sub", "lin"):
        b = p64.cell_bounds(ref, form, "direct")
        strong = ref.P >= 100.0 * np.median(ref.P)  # (the noise level: the median cell)
        assert strong.sum() > 100
        assert (b.dP[strong] / ref.P[strong]).max() <= 1e-5, form


# ----------------------------------------------------------------------------------------------------------------------
# wrong results fail
# ----------------------------------------------------------------------------------------------------------------------
def _tone_case(T, nperseg=256, seed=11):
    """Pulses 60 - 80 dB over the noise, records from the oracle, their linear fields and the float64 reference."""
    x, noise_db = make_input("tones80", nperseg, T, "hamming", seed)
    if T >= 1000:
        rng = np.random.default_rng(seed)
        w = oracle.window_coefficients("hamming", nperseg)
        n = T * nperseg
        pulses = synth.random_pulses(rng, n, FS, w, 12, dur_ms=(5, 20), peak_dbw=(noise_db + 60, noise_db + 80))
        x = synth.make_stream(synth.StreamSpec(n, FS, pulses), seed)
    kw = analyzer_kwargs(nperseg, T, "hamming", noise_db)
    oa = oracle.OracleAnalyzer(**kw)
    _, _, spec = oracle.stft_power(x, FS, "hamming", nperseg)
    recs = oracle.extract_records(np.arange(spec.shape[1]) * nperseg / FS + nperseg / 2 / FS, spec, None, oa.params)
    assert len(recs) >= 3
    ref = p64.stft_power_f64(x, FS, "hamming", nperseg)
    b = p64.cell_bounds(ref, "sub", "direct")
    fields = p64.oracle_record_fields(recs, spec, None)
    ok = p64.check_records(fields, ref, b, 32)
    assert not ok.failures, ok.failures[:5]
    return x, spec, recs, fields, ref, b


@pytest.mark.parametrize("T", [8000, 150])
@pytest.mark.parametrize("how", ["dropped", "doubled"])
def test_a_segment_dropped_or_doubled_in_a_row_sum_fails(T, how):
    x, spec, recs, fields, ref, b = _tone_case(T)
    sign = -1.0 if how == "dropped" else 1.0
    # (a) every record's row, with one of its plateau's segments dropped from / doubled in the sum
    mut = fields.copy()
    for i, r in enumerate(recs):
        row = spec[r.fi].astype(np.float64)
        t = (max(r.start, 0) + r.end) // 2
        mut["row_mean"][i] = np.float32((row.sum() + sign * row[t]) / T)
    chk = p64.check_records(mut, ref, b, 32)
    assert len({f.split(" row_mean")[0] for f in chk.failures if "row_mean" in f}) == len(recs), chk.worst
    # (b) every row of a noise-only stream: a segment in the middle of the buffer
    x = synth.make_stream(synth.StreamSpec(T * 256, FS, []), 12)
    ref = p64.stft_power_f64(x, FS, "hamming", 256)
    rm_bound = p64.row_mean_bound(ref, p64.cell_bounds(ref, "lin", "direct"), 32)
    t = T // 2
    rows = oracle.stft_power(x, FS, "hamming", 256)[2].astype(np.float64)
    assert np.all(np.abs((rows.sum(axis=1) / T).astype(np.float32) - ref.P.mean(axis=0)) <= rm_bound)
    mut_rm = ((rows.sum(axis=1) + sign * rows[:, t]) / T).astype(np.float32)
    flagged = np.abs(mut_rm - ref.P.mean(axis=0)) > rm_bound
    assert flagged.mean() > 0.9, flagged.mean()


def test_a_plateau_cell_from_the_neighbouring_segment_fails():
    x, spec, recs, fields, ref, b = _tone_case(8000)
    mut = fields.copy()
    for i, r in enumerate(recs):
        cells = spec[r.fi, r.start : r.end].copy()
        j = int(np.argmax(cells))
        cells[j] = spec[r.fi, r.start + j + 1] if r.start + j + 1 < spec.shape[1] else spec[r.fi, r.start + j - 1]
        mut[i]["max_p"], mut[i]["mean_p"], mut[i]["std_db"] = np.max(cells), np.mean(cells), np.std(oracle.to_db(cells))
    chk = p64.check_records(mut, ref, b, 32)
    assert len({f.split(" max_p")[0] for f in chk.failures if " max_p" in f}) == len(recs), chk.worst


def _spec_fails(got, ref, form="sub"):
    return p64.cell_ratios(got, ref, p64.cell_bounds(ref, form, "direct")).max()


def test_window_off_by_1e_4_fails():
    x, spec, recs, fields, ref, b = _tone_case(150)
    w32 = p64.window_f32("hamming", 256).astype(np.float32)
    n = np.arange(256)
    fast = (w32 * (1.0 + 1e-4 * np.cos(2 * np.pi * 37 * n / 256 + 0.4))).astype(np.float32)  # a cosine good to 1e-4
    scale = p64.scale_f32("hamming", 256, FS)
    assert _spec_fails(stft_f32(x, w32, scale), ref) <= 1.0  # (the restatement itself is honest)
    assert _spec_fails(stft_f32(x, fast, scale), ref) > 1.0


def test_scale_off_by_1e_5_fails():
    x, spec, recs, fields, ref, b = _tone_case(150)
    w32 = p64.window_f32("hamming", 256).astype(np.float32)
    scale = p64.scale_f32("hamming", 256, FS)
    mutated = stft_f32(x, w32, scale * (1 + 1e-5))
    assert _spec_fails(mutated, ref) > 1.0
    # ... and the records built on it
    mut = fields.copy()
    for k in ("max_p", "mean_p", "row_mean"):
        mut[k] = (fields[k].astype(np.float64) * (1 + 1e-5)).astype(np.float32)
    assert p64.check_records(mut, ref, b, 32).failures


def test_segment_mean_off_by_1000_ulp_fails():
    x, _ = make_input("dc80", 256, 150, "hamming", 4)
    ref = p64.stft_power_f64(x, FS, "hamming", 256)
    w32 = p64.window_f32("hamming", 256).astype(np.float32)
    scale = p64.scale_f32("hamming", 256, FS)

    def off(seg):
        m = seg.mean(axis=1, keepdims=True)
        re, im = m.real.astype(np.float32), m.imag.astype(np.float32)
        return (re + 1000 * np.spacing(re)) + 1j * (im + 1000 * np.spacing(im))

    for form in ("sub", "lin"):
        assert _spec_fails(stft_f32(x, w32, scale), ref, form) <= 1.0
        assert _spec_fails(stft_f32(x, w32, scale, mean_fn=lambda s: off(s).astype(np.complex64)), ref, form) > 1.0


def test_a_sequential_float32_row_sum_fails_at_config2_length():
    """The summation term encodes float32 partial rows of at most segs_per_chunk cells (and 16 lane groups), added in
    float64.  A row summed by one sequential float32 loop over 8 000 cells is outside it: after a strong burst at the start
    of a row the running sum's half-ulp exceeds every later noise cell, and they are lost."""
    T, N = 8000, 256
    noise_db = 10 * math.log10(2 * synth.NOISE_SIGMA ** 2 / FS)
    w = oracle.window_coefficients("hamming", N)
    f = 40 * FS / N  # bin 40, centred
    pulse = synth.Pulse(0, 20 * N, f, synth.amp_for_peak_dbw(noise_db + 60, w, FS))
    x = synth.make_stream(synth.StreamSpec(T * N, FS, [pulse]), 9)
    _, _, spec = oracle.stft_power(x, FS, "hamming", N)
    ref = p64.stft_power_f64(x, FS, "hamming", N)
    bound = p64.row_mean_bound(ref, p64.cell_bounds(ref, "sub", "direct"), L=32)
    want = ref.P.mean(axis=0)
    pairwise = np.array([np.mean(row) for row in spec])  # (the oracle's row mean: np.mean of one row, pairwise)
    partial = np.array([sum(float(np.sum(r[i : i + 32], dtype=np.float32)) for i in range(0, T, 32)) / T for r in spec[38:43]])
    sequential = np.cumsum(spec, axis=1, dtype=np.float32)[:, -1] / np.float32(T)
    assert np.all(np.abs(pairwise - want) <= bound)
    assert np.all(np.abs(partial - want[38:43]) <= bound[38:43])
    assert abs(sequential[40] - want[40]) > bound[40], (sequential[40], want[40], bound[40])


def test_a_finite_value_where_nan_is_due_fails_and_the_reverse():
    """tests/nonfinite_cases.py: a NaN cell in the reference makes the record's max, mean and std (and its row's mean) NaN."""
    import dataclasses

    x, spec, recs, fields, ref, b = _tone_case(150)
    r = recs[0]
    P = ref.P.copy()
    P[(max(r.start, 0) + r.end) // 2, r.fi] = np.nan
    due = p64.check_records(fields[:1], dataclasses.replace(ref, P=P), b, 32).failures
    assert len(due) == 4 and all(any(f" {k}: " in f for f in due) for k in ("max_p", "mean_p", "std_db", "row_mean")), due  # finite where NaN is due
    mut = fields.copy()
    for k in ("max_p", "mean_p", "std_db", "row_mean"):
        mut[k][0] = np.nan
    assert len(p64.check_records(mut[:1], ref, b, 32).failures) == 4  # NaN where a finite value is due
    assert not p64.check_records(mut[:1], dataclasses.replace(ref, P=P), b, 32).failures  # NaN where NaN is due


if __name__ == "__main__":
    by_family = {}
    for case in SWEEP:
        w, r = run_case(*case)
        fam = FAMILY[case[0]]
        d = by_family.setdefault(fam, {})
        for k, v in list(w.items()) + [(f"record {k}", v) for k, v in r.items() if k != "n_records"]:
            d[k] = max(d.get(k, 0.0), v)
    for fam, d in by_family.items():
        print(f"{fam:16s} " + "  ".join(f"{k} {v:.3f}" for k, v in sorted(d.items())))
