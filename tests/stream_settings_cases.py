"""Input and settings of the per-stream-settings tests (tests/test_gpu_stream_settings.py): one IQ for every stream of a
batch, so that only the settings can make the streams' records differ, and the eight settings.

Two consecutive 1-s buffers at 300 kS/s (``make_stream``, seeds 1 and 2), pulses at peak -60 dBW unless noted:

* first buffer: 10 ms at +20 kHz, 18 ms at -35 kHz, 30 ms at +50 kHz, 50 ms at -70 kHz, 20 ms at +90 kHz with peak -84 dBW,
  and 12 ms at +110 kHz from 988 ms on -- across the buffer edge;
* second buffer: 10 ms at +110 kHz from sample 0 (the edge pulse goes on, phase-continuous: 110 kHz x 1 s is a whole number
  of cycles) and 12 ms at +5 kHz from 400 ms on.

Where 8 ms is under two STFT hops (nperseg 4096: 13.7 ms, 8192: 27.3 ms) the whole time axis -- buffer, pulse starts and
lengths, and the streams' duration settings -- is stretched by ``time_scale(nperseg)``, the smallest whole factor that makes
the stretched 8 ms three hops long: with two, the stretched 10-ms pulse (2.5 hops) and its leading cell last longer than the
stretched 15-ms minimum (3.75 hops) at nperseg 8192, and the oracle keeps the same records with both minima.
"""
import math

import numpy as np

from oracle import analyze_oracle as oracle
from pyradiotracking_amd import synth

FS = 300000
WINDOW = "hamming"
SIGMA_QUIET = 1e-5   # noise far under every threshold: the SNR settings keep the same records
SIGMA_FLOOR = 8.7e-3  # noise floor 2 sigma^2 / fs = -93 dBW/Hz, near the -90 dBW threshold: the SNR settings separate

#: (name, keywords that differ from the defaults 8 ms / 40 ms / 5 dB / -90 dBW)
STREAMS = (
    ("defaults", {}),
    ("min15", dict(signal_min_duration_ms=15.0)),
    ("max25", dict(signal_max_duration_ms=25.0)),
    ("max60", dict(signal_max_duration_ms=60.0)),
    ("thr-80", dict(signal_threshold_dbw=-80.0)),
    ("centre", dict(center_freq=433920000)),
    ("snr3", dict(snr_threshold_db=3.0)),
    ("snr12", dict(snr_threshold_db=12.0)),
)
DEFAULTS = dict(signal_min_duration_ms=8.0, signal_max_duration_ms=40.0, signal_threshold_dbw=-90.0, snr_threshold_db=5.0,
                center_freq=150150000)
NAMES = [n for n, _ in STREAMS]
#: settings chosen to differ in their records: at the quiet level the duration gates and the threshold, under the floor the SNR
DIFFER_QUIET = ("defaults", "min15", "max25", "max60", "thr-80")
DIFFER_FLOOR = ("snr3", "defaults", "snr12")


def time_scale(nperseg: int) -> int:
    hop_ms = 1000.0 * nperseg / FS
    return 1 if 8.0 >= 2.0 * hop_ms else math.ceil(3.0 * hop_ms / 8.0)


def stream_kwargs(i: int, nperseg: int, threshold_shift_db: float = 0.0) -> dict:
    """The analysis keywords of stream ``i`` (oracle and analyzer alike), durations stretched for ``nperseg``."""
    kw = dict(DEFAULTS)
    kw.update(STREAMS[i][1])
    k = time_scale(nperseg)
    kw["signal_min_duration_ms"] *= k
    kw["signal_max_duration_ms"] *= k
    kw["signal_threshold_dbw"] += threshold_shift_db
    return kw


def batch_kwargs(nperseg: int, threshold_shift_db: float = 0.0, streams=None) -> dict:
    """The same as per-device sequences for BatchSignalAnalyzer."""
    idx = range(len(STREAMS)) if streams is None else streams
    per = [stream_kwargs(i, nperseg, threshold_shift_db) for i in idx]
    out = {name: [p[name] for p in per] for name in DEFAULTS}
    out.update(sample_rate=FS, fft_nperseg=nperseg, fft_window=WINDOW)
    return out


def buffers(nperseg: int, sigma: float):
    """``[2, B]`` complex64: the two buffers every stream gets."""
    k = time_scale(nperseg)
    blen = k * FS
    w = oracle.window_coefficients(WINDOW, nperseg)
    ms = lambda v: int(round(v * 1e-3 * k * FS))
    amp = lambda dbw: synth.amp_for_peak_dbw(dbw, w, FS)
    first = [
        synth.Pulse(ms(100), ms(10), 20e3, amp(-60.0)),
        synth.Pulse(ms(250), ms(18), -35e3, amp(-60.0)),
        synth.Pulse(ms(400), ms(30), 50e3, amp(-60.0)),
        synth.Pulse(ms(550), ms(50), -70e3, amp(-60.0)),
        synth.Pulse(ms(700), ms(20), 90e3, amp(-84.0)),
        synth.Pulse(ms(988), ms(12), 110e3, amp(-60.0)),
    ]
    second = [
        synth.Pulse(0, ms(10), 110e3, amp(-60.0)),
        synth.Pulse(ms(400), ms(12), 5e3, amp(-60.0)),
    ]
    a = synth.make_stream(synth.StreamSpec(blen, FS, first, noise_sigma=sigma), 1)
    b = synth.make_stream(synth.StreamSpec(blen, FS, second, noise_sigma=sigma), 2)
    return np.stack([a, b])


def oracle_run(bufs, nperseg: int, streams=None, threshold_shift_db: float = 0.0, ts=None):
    """Per stream and buffer ``(all signals, kept signals, spectrogram, previous spectrogram)`` of an OracleAnalyzer built
    with that stream's keywords, look-back included."""
    import datetime

    import pytz

    ts = ts or datetime.datetime(2024, 3, 1, 12, 0, 0, tzinfo=pytz.utc)
    out = []
    for i in (range(len(STREAMS)) if streams is None else streams):
        oa = oracle.OracleAnalyzer(device=str(i), sample_rate=FS, fft_nperseg=nperseg, fft_window=WINDOW,
                                   **stream_kwargs(i, nperseg, threshold_shift_db))
        per = []
        for buf in bufs:
            prev = oa.spec_last
            every, kept = oa.process(buf, ts)
            per.append((every, kept, oa.spec_last, prev))
        out.append(per)
    return out


def keys(signals):
    return [(x.fi, x.start, x.end) for x in signals]
