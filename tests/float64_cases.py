"""Inputs of the float64-path tests, rebuilt from seeds (tests/test_float64_contract.py, tests/test_gpu_float64_path.py).

Family (a): threshold-level buffers -- config-1 geometry (300 kS/s, nperseg 256, hamming), one bin-centred 20 ms pulse, noise
sigma = 1e-9, the pulse scaled so its full cells sit within +-1e-7 (relative) of -90 dBW.  complex64 round-off (6e-8) then
decides some of them: the reference gives a different record list on complex64 and on complex128 input.
"""
import datetime

import numpy as np

from oracle import analyze_oracle as oracle

TS0 = datetime.datetime(2024, 1, 1, tzinfo=datetime.timezone.utc)
FS = 300000
NPERSEG = 256
BIN = 43
THR_DBW = -90.0


def threshold_buffer(seed: int, n: int = 300000) -> np.ndarray:
    """complex128 buffer of family (a)."""
    rng = np.random.default_rng([64064, seed])
    w = oracle.window_coefficients("hamming", NPERSEG)
    p_target = 10 ** (THR_DBW / 10) * (1.0 + rng.uniform(-1e-7, 1e-7))
    amp = np.sqrt(p_target * FS * (w * w).sum()) / w.sum()  # a bin-centred tone covering a segment: |X|^2 scale = p_target
    x = 1e-9 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    length = int(0.020 * FS)
    start = int(rng.integers(NPERSEG * 8, n - length - NPERSEG * 8))
    k = np.arange(length)
    x[start:start + length] += amp * np.exp(2j * np.pi * BIN * (start + k) / NPERSEG)
    return x


def oracle_records(x: np.ndarray, nperseg: int = NPERSEG, window="hamming", fs=FS, last=None, **params):
    """(records, spec) of the oracle on ``x`` as given (its dtype decides the precision, as in SciPy)."""
    _, times, spec = oracle.stft_power(x, fs, window, nperseg)
    return oracle.extract_records(times, spec, last, oracle.ExtractParams(**params)), spec


def margin_ok(spec: np.ndarray, thr: float, snr: float, rel: float = 1e-12) -> bool:
    """Every cell is at least ``rel`` (relative) from the absolute threshold, and from the SNR threshold against its row mean."""
    spec = np.asarray(spec, dtype=np.float64)
    if np.any(np.abs(spec / thr - 1.0) < rel):
        return False
    ratio = spec / spec.mean(axis=1, keepdims=True) / snr
    return not np.any(np.abs(ratio - 1.0) < rel)


def key(records):
    return [(r.fi, r.start, r.end) for r in records]


def threshold_seeds(n_seeds: int = 60):
    """Seeds of family (a) whose complex64 and complex128 record lists differ, with every cell clear of its thresholds."""
    p = oracle.ExtractParams()
    out = []
    for seed in range(n_seeds):
        x = threshold_buffer(seed)
        r128, spec = oracle_records(x)
        r64, _ = oracle_records(x.astype(np.complex64))
        if key(r128) != key(r64) and margin_ok(spec, p.signal_threshold, p.snr_threshold):
            out.append(seed)
    return out
