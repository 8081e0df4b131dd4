"""Inputs of the map-free float64 path's tests (RT_FLAG_F64_SPARSE: tests/test_f64_sparse_contract.py,
tests/test_gpu_f64_sparse.py), rebuilt from seeds.

The fused scan transforms in another summation order than SciPy (and than the dense handle), so a cell's float64 power and a
row's mean differ from the oracle's in their last bits.  Every case therefore keeps only seeds whose oracle map (complex128)
holds no cell within 1e-6 (relative) of the absolute threshold or of the SNR threshold against its row mean
(``float64_cases.margin_ok(spec, thr, snr, rel=1e-6)``): round-off of 1e-15 cannot flip a decision there.  The selection
runs when the module is imported and every case must keep a seed.  (The threshold-level family of float64_cases cannot meet
1e-6 by its construction: see threshold_seeds.)
"""
import functools

import numpy as np

from oracle import analyze_oracle as oracle
from pyradiotracking_amd import synth
from tests import float64_cases as fc

FS = 300000
REL = 1e-6
SIZES = (32, 64, 128, 256, 512, 1024, 2048, 4096)
WINDOWS = (("hamming", 0.0), (("tukey", 0.25), 0.0), (("kaiser", 8.0), 2.5))  # (window, calibration_db)
CANDIDATES = 6  # seeds tried per case, in order


def pulses(n, fs, nperseg, window, seed, sigma=synth.NOISE_SIGMA, n_pulses=4):
    """complex128 buffer: noise and ``n_pulses`` random pulses, added in float64 (the recipe of the dense handle's GPU test)."""
    rng = np.random.default_rng([128, seed])
    w = oracle.window_coefficients(window, nperseg)
    x = sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for p in synth.random_pulses(rng, n, fs, w, n_pulses, dur_ms=(10.0, 30.0), peak_dbw=(-80.0, -60.0)):
        a, b = max(0, p.start), min(n, p.start + p.length)
        if b > a:
            t = np.arange(a, b, dtype=np.float64) / fs
            x[a:b] += p.amp * np.exp(2j * np.pi * (p.freq * t + p.phase))
    return x


def clear_of_thresholds(x, nperseg=256, window="hamming", fs=FS, **params):
    """margin_ok at REL on the oracle's map of ``x`` (a complex128 buffer analysed alone)."""
    p = oracle.ExtractParams(**params)
    _, _, spec = oracle.stft_power(x, fs, window, nperseg)
    return fc.margin_ok(spec, p.signal_threshold, p.snr_threshold, rel=REL)


def size_buffer(nperseg, window, seed):
    return pulses(max(300000, 64 * nperseg), FS, nperseg, window, 1000 * nperseg + seed)


@functools.lru_cache(maxsize=None)
def size_seed(nperseg, window, cal):
    """The first candidate seed of the sizes test's case that is clear of its thresholds."""
    for seed in range(CANDIDATES):
        if clear_of_thresholds(size_buffer(nperseg, window, seed), nperseg, window, calibration_db=cal):
            return seed
    return None


THRESHOLD_REL = 1e-11


def threshold_seeds(n_seeds=60, keep=2):
    """float64_cases' family (a) -- complex64 and complex128 disagree -- for the drop-in test.  Its pulse cells sit within 1e-7
    (relative) of the absolute threshold by construction, so REL cannot hold there; the margin asked instead is THRESHOLD_REL:
    the scan's power stays within 1e-13 log2(N) max(row) of the oracle's (the transform test's bound, 8e-13 at nperseg 256), and
    the cells near the threshold are their row's largest, so a cell 1e-11 clear of it cannot change sides."""
    p = oracle.ExtractParams()
    out = []
    for seed in range(n_seeds):
        x = fc.threshold_buffer(seed)
        r128, spec = fc.oracle_records(x)
        if not fc.margin_ok(spec, p.signal_threshold, p.snr_threshold, rel=THRESHOLD_REL):
            continue
        r64, _ = fc.oracle_records(x.astype(np.complex64))
        if fc.key(r128) != fc.key(r64):
            out.append(seed)
        if len(out) == keep:
            break
    return out


def tone_at(k, nperseg, fi, dbw=-70.0, window="hamming", fs=FS):
    """Samples ``k`` (absolute indices) of a tone centred on bin ``fi`` whose full cells hold ``dbw``."""
    w = oracle.window_coefficients(window, nperseg)
    amp = np.sqrt(10 ** (dbw / 10) * fs * (w * w).sum()) / w.sum()
    return amp * np.exp(2j * np.pi * fi * np.asarray(k) / nperseg)


def tone(n, nperseg, fi, seg0, n_segs, dbw=-70.0, window="hamming", fs=FS):
    """A bin-centred pulse over whole segments [seg0, seg0 + n_segs): full cells at ``dbw``, nothing outside them."""
    x = np.zeros(n, dtype=np.complex128)
    k = np.arange(seg0 * nperseg, (seg0 + n_segs) * nperseg)
    x[k] = tone_at(k, nperseg, fi, dbw, window, fs)
    return x


def noise(n, seed, sigma=1e-9):
    rng = np.random.default_rng([4170, seed])
    return sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))


SIZE_CASES = [(n, w, c) for n in SIZES for (w, c) in WINDOWS]
SIZE_SEEDS = {case: size_seed(*case) for case in SIZE_CASES}
assert all(v is not None for v in SIZE_SEEDS.values()), [c for c, v in SIZE_SEEDS.items() if v is None]
THRESHOLD_SEEDS = threshold_seeds()
assert THRESHOLD_SEEDS, "no threshold-level seed is clear of its thresholds at THRESHOLD_REL"
