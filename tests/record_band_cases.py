"""The bins beside each record's bin (``rt_fetch_record_band``): the NumPy restatement of the host book, the kernel's order column
by column with three planted faults, the twin case of the bit-identity test and the shapes of the GPU suite -- shared by
tests/test_record_band_contract.py (CPU) and tests/test_gpu_record_band.py (GPU).  The model of a value, its bound and the GPU
suite's buffers are tests/record_stft_cases.py's: a column is the single-bin value at the column's own bin, with the same
summation depth.

Twin case.  Bit identity 2 of the contract needs records of ONE stream at neighbouring bins with the same cells, so that their
frames hold the same samples.  A boxcar window and a tone half a bin above ``fi`` give them: the tone leaks 1 / (pi |d - 1/2|) of
its amplitude into bin fi + d, far over the threshold for every |d| <= 8 at amplitude 0.1 over noise of sigma 1e-6, and every bin
switches on and off in the same segments.  Bin 0 alone has no record: the mean is removed.  The pulse is ``twin_need`` segments
long -- 10 ms and two segments, over the default minimum duration of 8 ms at every size -- between quiet stretches twice as long,
so that the rows' means stay far under their tones (the SNR gate).
"""
import math

import numpy as np

from oracle import analyze_oracle as oracle
from tests import record_stft_cases as rs
from tests import sequence_cases as sq

FS = sq.FS
MAX_HALF = 8


# ---- the host book -----------------------------------------------------------------------------------------------------------------
def band_ok(N, k, w):
    return 1 <= k <= 16 and N >= 1 and N % k == 0 and 0 <= w <= MAX_HALF and 2 * w + 1 <= N


def band_bin(fi, j, w, N):
    return (fi + j - w) % N


def band_elems(frames, w):
    if frames < 0 or not 0 <= w <= MAX_HALF:
        return -1
    n = frames * (2 * w + 1)
    return n if n * 16 <= 2 ** 63 - 1 else -1


# ---- the kernel's order, column by column ------------------------------------------------------------------------------------------
FAULTS = ("reversed", "clamped", "centre_twiddles")


def column_bins(fi, half, N, fault=None):
    """the bin each of the 2 half + 1 columns is computed at -- ``fault``: what a wrong kernel would take instead"""
    d = np.arange(-half, half + 1)
    if fault == "reversed":
        d = -d
    if fault == "clamped":
        return np.clip(fi + d, 0, N - 1)
    if fault == "centre_twiddles":
        return np.full(len(d), fi)
    return (fi + d) % N


def restate_band(x, fi, half, w, root, nperseg, spp, ft=np.float32, fault=None):
    """[n_frames, 2 half + 1]: ``rs.restate`` -- the kernel's arithmetic, operation by operation -- per column at the column's bin"""
    return np.stack([rs.restate(x, int(b), w, root, nperseg, spp, ft) for b in column_bins(fi, half, nperseg, fault)], axis=1)


def model_band(x, fi, half, w, scale, nperseg, wide=False):
    """the model's ``Quantities`` per column (a list of 2 half + 1)"""
    return [rs.model_values(x, int(b), w, scale, nperseg, wide=wide) for b in column_bins(fi, half, nperseg)]


def band_ratios(got, qs, nperseg, spp, u=rs.U32):
    """[n_frames, B]: |got - model| / bound, column by column"""
    return np.stack([rs.ratios(got[:, j], q, nperseg, spp, u) for j, q in enumerate(qs)], axis=1)


# ---- the twin case -----------------------------------------------------------------------------------------------------------------
TWIN_WINDOW, TWIN_AMP, TWIN_SIGMA, TWIN_STREAM = "boxcar", 0.1, 1e-6, 1
TWIN_SIZES = (32, 256, 300, 4096)


def twin_bins(N):
    return (N - 1, N // 2 - 1, 5)


def twin_need(N):
    return math.ceil(0.010 * FS / N) + 2


def twin_layout(N):
    """(segments of the buffer, first hot segment, segments of the pulse)"""
    need = twin_need(N)
    return 5 * need, 2 * need, need


def twin_settings(N):
    """analysis keywords: the defaults but for the window, and at nperseg 4096 -- three segments are 41 ms -- a longer maximum"""
    kw = dict(sample_rate=FS, fft_nperseg=N, fft_window=TWIN_WINDOW)
    if twin_need(N) * N / FS > 0.038:
        kw["signal_max_duration_ms"] = 100.0
    return kw


def twin_buffer(N, fi, S=rs.GPU_S):
    """complex64 [S, T N]: noise in every stream, and in stream ``TWIN_STREAM`` the tone half a bin above ``fi`` (fftfreq order: a
    bin in the upper half is a negative frequency) over the pulse's segments"""
    T, a, need = twin_layout(N)
    rng = np.random.default_rng([N, fi])
    x = (rng.standard_normal((S, T * N)) + 1j * rng.standard_normal((S, T * N))) * TWIN_SIGMA
    f = (fi + 0.5) - (N if fi >= N // 2 else 0)
    n = np.arange(a * N, (a + need) * N)
    x[TWIN_STREAM, a * N:(a + need) * N] += TWIN_AMP * np.exp(2j * np.pi * f * (n - a * N) / N)
    return x.astype(np.complex64)


def twin_oracle_records(N, fi, x=None):
    """the oracle's records of the twin stream: [(fi, start, end)]"""
    x = twin_buffer(N, fi) if x is None else x
    kw = twin_settings(N)
    _, times, spec = oracle.stft_power(x[TWIN_STREAM], FS, TWIN_WINDOW, N)
    return sq.key(sq.extract(times, spec, None, sq.params_of(kw)))


# ---- record_band_spectrum, as a loop ------------------------------------------------------------------------------------------------
def spectrum_loop(offsets, first_segment, values, start, end, N, k):
    """the mean of |value|^2 per column over the frames wholly inside the record's own cells, frame by frame"""
    values = np.asarray(values)
    n = len(offsets) - 1
    out = np.full((n, values.shape[1]), np.nan)
    h = N // k
    for i in range(n):
        L = int(offsets[i + 1] - offsets[i])
        lead = min((-int(first_segment[i]) - 1) * k + 1, L) if first_segment[i] < 0 else 0
        acc, cnt = np.zeros(values.shape[1]), 0
        for j in range(L):
            pos = int(first_segment[i]) * N + j * h if j < lead else max(int(first_segment[i]), 0) * N + (j - lead) * h
            if start[i] * N <= pos and pos + N <= end[i] * N:
                acc += np.abs(values[offsets[i] + j].astype(np.complex128)) ** 2
                cnt += 1
        if cnt:
            out[i] = acc / cnt
    return out


# ---- the GPU suite -----------------------------------------------------------------------------------------------------------------
#: (nperseg, format): the smallest shapes at which each branch of the kernel exists
GPU_SHAPES = [(32, "u8"),        # G = 8
              (128, "u8"),       # G = 16
              (256, "u8"),       # G = 32
              (256, "c64"),      # G = 64, pieces held
              (4096, "c64"),     # several rounds, not held
              (300, "c64"),      # a last partial piece, 8-byte loads
              (300, "u8"),       # ... 2-byte loads
              (256, "i16"),
              (256, "c128"), (300, "c128")]
GPU_PAIRS = [(1, 0), (1, 2), (2, 1), (4, 2), (4, 8)]


def gpu_pairs(nperseg):
    return GPU_PAIRS + ([(16, 8)] if nperseg == 32 else [])


#: (nperseg, format) of the twin runs
TWIN_RUNS = [(32, "u8"), (256, "c64"), (300, "c64"), (256, "c128")]


def twin_feed(N, fi, fmt):
    """what the twin call feeds a handle: uint8 without a gain (the tone spans 13 steps either way, the noise none)"""
    from pyradiotracking_amd import synth

    x = twin_buffer(N, fi)
    if fmt == "u8":
        return np.stack([synth.quantize_u8(row) for row in x])
    return x.astype(np.complex128) if fmt == "c128" else x
