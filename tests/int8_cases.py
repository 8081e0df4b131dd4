"""Inputs and oracle references of the int8 tests (tests/test_gpu_int8.py), rebuilt from seeds and computed once per session.

The wire recipe is that of test_uint8_wire_format_ingestion (tests/test_gpu_parity.py): 3 streams, 2 consecutive buffers of
256 * 1100 + 40 samples at 2.048 MS/s, noise sigma 0.012 (one and a half quantisation steps), 8 random pulses of 9 .. 30 ms at
-62 .. -48 dBW per stream, quantised with synth.quantize_i8.

Checked on the CPU against the oracle (the comparisons of tests/test_gpu_int8.py assert the two conditions that keep a case from
passing empty: every stream and buffer has a record, buffer 1 has one that reaches back into buffer 0):
  wire recipe    8 .. 16 records per stream and buffer at nperseg 256, 10 .. 15 at nperseg 4096; 4 records reach back at nperseg
                 256, 6 and 7 at nperseg 4096; no sample clips
  modes batch    8 .. 30 records per stream and buffer, 3 .. 6 reaching back per stream in buffer 1; no sample clips"""
import datetime
import functools

import numpy as np

from oracle import analyze_oracle as oracle
from pyradiotracking_amd import synth

TS0 = datetime.datetime(2024, 1, 1, tzinfo=datetime.timezone.utc)
FS = 2048000
N_STREAMS, N_BUF = 3, 2
BLEN = 256 * 1100 + 40


def kwargs(nperseg, window, threshold_dbw=-80.0):
    return dict(sample_rate=FS, fft_nperseg=nperseg, fft_window=window, signal_threshold_dbw=threshold_dbw)


def _wire_streams(nperseg, window, seed):
    w = oracle.window_coefficients(window, nperseg)
    rng = np.random.default_rng(321 + nperseg if seed is None else seed)
    out = []
    for s in range(N_STREAMS):
        pulses = synth.random_pulses(rng, N_BUF * BLEN, FS, w, 8, dur_ms=(9, 30), peak_dbw=(-62, -48))
        out.append(synth.make_stream(synth.StreamSpec(N_BUF * BLEN, FS, pulses, noise_sigma=0.012), 900 + s))
    return out


@functools.lru_cache(maxsize=None)
def wire(nperseg, window, seed=None, gain=1.0):
    """int8 [S, 2 * N_BUF * BLEN] (read-only); ``seed`` None = 321 + nperseg."""
    raw = np.stack([synth.quantize_i8(x, gain=gain) for x in _wire_streams(nperseg, window, seed)])
    raw.setflags(write=False)
    return raw


# ---- full scale: the wire recipe under a gain at which the noise alone reaches both rails, and in every buffer a stretch of
# kRailSegs segments of 4096 in which stream s carries an offset that pins I and Q to a rail each -- (127, 127), (-128, -128),
# (127, -128): whole segments clip to a constant, x - mean is exactly zero there in the reference, and the guard of the detrend by
# linearity (rt_kernels.h: StftParams::dc_flag) marks the stream, whose call is analysed again on the subtract-first kernels.
RAIL_FIRST, RAIL_SEGS = 20 * 4096, 12
RAILS = ((1.0, 1.0), (-1.0, -1.0), (1.0, -1.0))


@functools.lru_cache(maxsize=None)
def rails(nperseg, gain, seed=86):
    out = []
    for s, x in enumerate(_wire_streams(nperseg, "hamming", seed)):
        x = np.array(x, dtype=np.complex128)
        for k in range(N_BUF):
            a = k * BLEN + RAIL_FIRST
            x[a: a + RAIL_SEGS * 4096] += 4.0 * (RAILS[s][0] + 1j * RAILS[s][1]) / gain * 8.0
        out.append(synth.quantize_i8(x, gain=gain))
    raw = np.stack(out)
    raw.setflags(write=False)
    return raw


@functools.lru_cache(maxsize=None)
def rails_oracle(nperseg, gain, threshold_dbw):
    raw = rails(nperseg, gain)
    return oracle_buffers([synth.i8_to_complex64(buffer_of(raw, k)) for k in range(N_BUF)], kwargs(nperseg, "hamming", threshold_dbw))


def buffer_of(raw_all, k, blen=BLEN):
    """Buffer k of every stream, contiguous and writable: int8 [S, 2 * blen]."""
    return np.ascontiguousarray(raw_all[:, 2 * k * blen: 2 * (k + 1) * blen])


def oracle_buffers(bufs_c, kw):
    """[buffer][stream] -> (signals, shadowed flags) of oracle.OracleAnalyzer over the consecutive buffers ``bufs_c`` ([S, B] complex
    each; their dtype decides the oracle's precision, as in SciPy)."""
    n_streams = bufs_c[0].shape[0]
    oas = [oracle.OracleAnalyzer(device=str(s), **kw) for s in range(n_streams)]
    out = []
    for c in bufs_c:
        row = []
        for s in range(n_streams):
            want, kept = oas[s].process(c[s], TS0)
            kept_ids = {id(x) for x in kept}
            row.append((want, [id(x) not in kept_ids for x in want]))
        out.append(row)
    return out


def assert_not_empty(ref):
    """The two conditions every oracle comparison asserts: every stream and buffer has a record, and buffer 1 has at least one that
    starts in the previous buffer (start < 0), so the look-back is read."""
    for k, row in enumerate(ref):
        for s, (want, _) in enumerate(row):
            assert len(want) >= 1, f"buffer {k} stream {s}: no record"
    assert any(x.start < 0 for want, _ in ref[1] for x in want), "buffer 1: no record reaches back into buffer 0"


@functools.lru_cache(maxsize=None)
def wire_oracle(nperseg, window, seed=None, gain=1.0, threshold_dbw=-80.0):
    raw = wire(nperseg, window, seed, gain)
    return oracle_buffers([synth.i8_to_complex64(buffer_of(raw, k)) for k in range(N_BUF)], kwargs(nperseg, window, threshold_dbw))


# ---- the batch of the mode test: tests/int16_cases.py's (nperseg 256 at 300 kS/s, a floor of -160 dBW under pulses of -140 .. -126
# dBW) with the gain changed to 3000 (69.5 dB), which puts the floor at about 1.5 quantisation steps of int8.  Three variants, as there:
#   "quiet"  threshold -150 dBW (+ 69.5): clean input, what RT_MODE_SPARSE is for (a sparse call whose lists overflow has no result)
#   "near"   threshold -158 dBW (+ 69.5), 2 dB over the floor: the sparse lists overflow -- AUTO leaves the sparse level with the whole batch
#   "mixed"  the quiet threshold with stream 2 raised by 12 dB: its floor lies 2 dB over the threshold, its lists alone overflow --
#            AUTO re-runs that stream dense from a stream list
M_FS, M_NPERSEG, M_STREAMS, M_BUF = 300000, 256, 6, 2
M_BLEN = 256 * 700
M_GAIN = 3000.0
M_GAIN_DB = float(20 * np.log10(M_GAIN))
M_NOISY = 2
M_THRESHOLD = {"quiet": -150.0 + M_GAIN_DB, "near": -158.0 + M_GAIN_DB, "mixed": -150.0 + M_GAIN_DB}


def modes_kwargs(variant):
    return dict(sample_rate=M_FS, fft_nperseg=M_NPERSEG, fft_window="hamming", signal_threshold_dbw=M_THRESHOLD[variant])


@functools.lru_cache(maxsize=None)
def _modes_wire(mixed):
    w = oracle.window_coefficients("hamming", M_NPERSEG)
    sigma = float(np.sqrt(10 ** (-160.0 / 10) * M_FS / 2))
    raw = []
    for s in range(M_STREAMS):
        rng = np.random.default_rng([256, s])
        pulses = synth.random_pulses(rng, M_BUF * M_BLEN, M_FS, w, 6 * M_BUF, dur_ms=(10, 30), peak_dbw=(-140.0, -126.0))
        pulses.append(synth.Pulse(M_BLEN - int(0.006 * M_FS) - 11 * s, int(0.015 * M_FS), (0.05 + 0.04 * s) * M_FS, synth.amp_for_peak_dbw(-128.0, w, M_FS)))  # across the buffers
        x = synth.make_stream(synth.StreamSpec(M_BUF * M_BLEN, M_FS, pulses, noise_sigma=sigma), seed=2560 + s)
        raw.append(synth.quantize_i8(x, gain=M_GAIN * (4.0 if mixed and s == M_NOISY else 1.0)))
    raw = np.stack(raw)
    raw.setflags(write=False)
    return raw


def modes_wire(variant):
    return _modes_wire(variant == "mixed")


@functools.lru_cache(maxsize=None)
def modes_oracle(variant):
    raw = modes_wire(variant)
    return oracle_buffers([synth.i8_to_complex64(buffer_of(raw, k, M_BLEN)) for k in range(M_BUF)], modes_kwargs(variant))
