"""Host-side mirror of the reference's ``SignalAnalyzer`` for the analysis path.

Same constructor keywords, same method names, same ``Signal`` records on the
same kind of queue as ``radiotracking/analyze.py:20-452`` -- but the arithmetic
of ``process_samples`` (STFT power, plateau extraction with look-back, shadow
verdicts) runs in the gfx950 HIP kernels behind ``librt_analyze.so``.  This
module only derives parameters, stages buffers and turns the integer/float32
records the kernels return into ``Signal`` objects (float64 / datetime parts
are computed here with the reference's own expressions, so they are bit-exact
by construction).

Not mirrored (out of scope): opening an RTL-SDR, the
SIGALRM watchdog, the process itself (the per-stream life-cycle rules of the
reference's Runner are in :mod:`pyradiotracking_amd.runner`).

Two entry levels:

* :class:`SignalAnalyzer` -- one stream, drop-in for the reference class.
* :class:`BatchSignalAnalyzer` -- ``S`` independent streams per call, IQ
  resident in HBM (``[S, B]`` complex64); this is what ``bench.py`` drives.
"""
from __future__ import annotations

import collections.abc
import datetime
import logging
import time
from typing import List, Optional, Sequence, Union

import numpy as np
import pytz
import scipy.fft
import scipy.signal

from . import Signal, StateMessage, dB, from_dB
from . import _native

logger = logging.getLogger(__name__)


def window_coefficients(fft_window, nperseg: int) -> np.ndarray:
    """What ``scipy.signal.spectrogram`` makes of its ``window`` argument
    (scipy/signal/_spectral_py.py:2239-2263): names/tuples go through
    ``get_window`` (periodic), arrays are taken as coefficients."""
    if isinstance(fft_window, (str, tuple)):
        return scipy.signal.get_window(fft_window, nperseg)
    win = np.asarray(fft_window)
    if win.ndim != 1:
        raise ValueError("window must be 1-D")
    if win.shape[0] != nperseg:
        raise ValueError("value specified for nperseg is different from length of window")
    return win


def stft_constants(fft_window, nperseg: int, sample_rate):
    """float32 window and PSD scale exactly as SciPy forms them for complex64
    input (_spectral_py.py:2083-2087): the window is cast to complex64 and
    ``scale = 1/(fs * sum(win*win))`` is evaluated in that dtype."""
    win = window_coefficients(fft_window, nperseg).astype(np.complex64)
    scale = 1.0 / (sample_rate * (win * win).sum())
    return np.ascontiguousarray(win.real, dtype=np.float32), np.float32(scale.real)


def stft_constants_f64(fft_window, nperseg: int, sample_rate):
    """float64 window and PSD scale as SciPy forms them for complex128 input (_spectral_py.py:2083-2087): the float64
    window is kept (its result type with complex64 is already complex128) and ``scale = 1/(fs * sum(win*win))`` is a
    float64 figure."""
    win = np.asarray(window_coefficients(fft_window, nperseg), dtype=np.float64)
    scale = 1.0 / (sample_rate * (win * win).sum())
    return np.ascontiguousarray(win), float(scale)


PRECISIONS = ("float32", "float64")


class _Heartbeat:
    """Stand-in for the ``multiprocessing.Value("d")`` the reference's Runner hands to every analyzer."""

    def __init__(self):
        self.value = 0.0


class _RecordDecoder:
    """rt_record arrays -> Signal field columns (analyze.py:360, 420-449)."""

    def __init__(self, nperseg: int, sample_rate, center_freq, calibration_db, f64: bool = False):
        """``calibration_db`` and ``center_freq``: one value, or one per stream (the reference has one analyzer, one
        calibration and one centre frequency per SDR, __main__.py:140-141, analyze.py:360).  ``f64``: the records are float64 (a float64 handle), and so are the
        calibrations subtracted from them."""
        self.f64 = f64
        self.nperseg = nperseg
        self.sample_rate = sample_rate
        self.center_freq = center_freq
        self.calibration_db = calibration_db
        self.freqs = scipy.fft.fftfreq(nperseg, 1 / sample_rate)  # _spectral_py.py:2113

    def times(self, k: np.ndarray) -> np.ndarray:
        # element k of  arange(N/2, B - N/2 + 1, N) / float(fs)   (_spectral_py.py:2136)
        return (self.nperseg / 2 + np.asarray(k, dtype=np.float64) * self.nperseg) / float(self.sample_rate)

    @staticmethod
    def noise_dbw(row_mean):
        """``Signal.noise`` from a row mean: ``dB(freq_avg)``, uncalibrated as in the reference (analyze.py:446)."""
        with np.errstate(divide="ignore", invalid="ignore"):
            return dB(row_mean)

    def decode(self, rec: np.ndarray, freqs: Optional[np.ndarray] = None, times: bool = True):
        """Signal field columns of ``rec``; ``freqs`` replaces the analyzer's own frequency axis (caller-supplied
        spectrograms may have any number of bins, ``extract_signals``).  ``times=False``: without start time and duration
        (``None`` in their places -- the native row builder derives them from the cell coordinates itself)."""
        t_start = duration_s = None
        if times:
            start = rec["start"].astype(np.int64)
            end = rec["end"].astype(np.int64)
            t_end = self.times(end)
            t_start = np.where(start < 0, -self.times(np.abs(start)), self.times(np.maximum(start, 0)))
            duration_s = t_end - t_start
        cal = self.calibration_db
        if np.ndim(cal):
            # float32 dB figure minus a Python float is a float32 subtraction (NEP 50): the same bits as
            # subtracting the calibration rounded to float32
            cal = np.asarray(cal, dtype=np.float64 if self.f64 else np.float32)[rec["stream"]]
        with np.errstate(divide="ignore", invalid="ignore"):
            max_dbw = dB(rec["max_p"]) - cal  # float32, analyze.py:442
            avg_dbw = dB(rec["mean_p"]) - cal  # :444
            noise_dbw = self.noise_dbw(rec["row_mean"])  # :446
            snr_db = dB(rec["mean_p"] / rec["row_mean"])  # :447
        center = self.center_freq
        if np.ndim(center):
            center = np.asarray(center)[rec["stream"]]  # every stream's SDR is tuned on its own
        frequency = (self.freqs if freqs is None else np.asarray(freqs))[rec["fi"]] + center  # :360
        return t_start, duration_s, frequency, max_dbw, avg_dbw, rec["std_db"], noise_dbw, snr_db

    def signal_columns(self, rec: np.ndarray, device_names: Sequence[str], ts_starts: Sequence[datetime.datetime]):
        """The nine ``Signal`` fields of every record of ``rec`` as nine Python lists (analyze.py:420-450), the reference's
        expressions evaluated column-wise: start and duration are whole hops, so a call holds few distinct values of either and
        one ``timedelta`` serves all records that share it; a stream's start time is taken to UTC once where its UTC offset
        does not change over the buffer (else record by record, as the reference does)."""
        t_start, duration_s, frequency, max_dbw, avg_dbw, std_db, noise_dbw, snr_db = self.decode(rec)

        def deltas(x):
            uniq, inv = np.unique(x, return_inverse=True)
            objs = np.empty(len(uniq), dtype=object)
            objs[:] = [datetime.timedelta(seconds=v) for v in uniq.tolist()]  # :428, :434
            return objs, inv

        start_td, start_i = deltas(t_start)
        dur_td, dur_i = deltas(duration_s)
        streams = rec["stream"]
        utc = pytz.utc
        # (ts_start + delta).astimezone(utc) == ts_start.astimezone(utc) + delta unless the zone's offset changes in between:
        # checked per stream at both ends of what the call can hold
        lo, hi = start_td[0], start_td[-1]
        n_names = len(device_names)
        base = np.empty(n_names, dtype=object)
        exact = True
        for s_ in np.unique(streams).tolist():
            b0 = ts_starts[s_]
            bu = b0.astimezone(utc)
            base[s_] = bu
            exact = exact and (b0 + lo).astimezone(utc) == bu + lo and (b0 + hi).astimezone(utc) == bu + hi
        starts = start_td[start_i].tolist()
        if exact:
            ts = [b + d for b, d in zip(base[streams].tolist(), starts)]  # :434, :449
        else:
            ts = [(ts_starts[s_] + d).astimezone(utc) for s_, d in zip(streams.tolist(), starts)]
        names = np.empty(n_names, dtype=object)
        names[:] = list(device_names)
        cols = [np.asarray(c, dtype=np.float64).tolist() for c in (frequency, max_dbw, avg_dbw, std_db, noise_dbw, snr_db)]  # float(np.float32): exact
        return [names[streams].tolist(), ts, cols[0], dur_td[dur_i].tolist()] + cols[1:]

    def signals(self, rec: np.ndarray, device_names: Sequence[str], ts_starts: Sequence[datetime.datetime]) -> List[Signal]:
        """``Signal`` objects of ``rec``: the columns above, the objects filled slot by slot (what ``Signal.__init__`` would store
        for these types, without its conversions)."""
        n = len(rec)
        if n == 0:
            return []
        new = Signal.__new__
        out = [new(Signal) for _ in range(n)]
        for sig, dv, ts, fr, du, mx, av, sd, no, sn in zip(out, *self.signal_columns(rec, device_names, ts_starts)):
            sig.device = dv
            sig.ts = ts
            sig.frequency = fr
            sig.duration = du
            sig.max = mx
            sig.avg = av
            sig.std = sd
            sig.noise = no
            sig.snr = sn
        return out

    def signal_batch(self, rec: np.ndarray, device_names: Sequence[str], ts_starts: Sequence[datetime.datetime]) -> "SignalBatch":
        """The same signals as a lazy sequence: the field columns are built at once, a ``Signal`` object only when an element
        is asked for -- for consumers that look at some of the signals, or hand the columns on (CSV rows, the matcher)."""
        if len(rec) == 0:
            return SignalBatch([[] for _ in range(9)])
        return SignalBatch(self.signal_columns(rec, device_names, ts_starts))


class SignalBatch(collections.abc.Sequence):
    """A read-only sequence of ``Signal`` over nine field columns (``_RecordDecoder.signal_batch``)."""

    __slots__ = ("columns",)

    def __init__(self, columns):
        self.columns = columns

    def __len__(self):
        return len(self.columns[0])

    def __getitem__(self, i):
        if isinstance(i, slice):
            return SignalBatch([c[i] for c in self.columns])
        sig = Signal.__new__(Signal)
        (sig.device, sig.ts, sig.frequency, sig.duration, sig.max, sig.avg, sig.std, sig.noise, sig.snr) = [c[i] for c in self.columns]
        return sig

    def __eq__(self, other):
        """equal to any sequence of the same ``Signal`` values, a plain list included (``analyze_buffer(...) == []``)"""
        if not isinstance(other, (collections.abc.Sequence, SignalBatch)) or isinstance(other, (str, bytes)):
            return NotImplemented
        return len(self) == len(other) and all(_same_signal(a, b) for a, b in zip(self, other))

    __hash__ = None

    def __repr__(self):
        return f"SignalBatch({list(self)!r})"


def _same_signal(a, b) -> bool:
    fields = ("device", "ts", "frequency", "duration", "max", "avg", "std", "noise", "snr")
    try:
        return all(getattr(a, f) == getattr(b, f) or (getattr(a, f) != getattr(a, f) and getattr(b, f) != getattr(b, f)) for f in fields)
    except AttributeError:
        return False


FINE_DTYPE = np.dtype([("offset_hz", np.float64), ("coherence", np.float64), ("n_pairs", np.int32)])
#: a row of :meth:`BatchSignalAnalyzer.fetch_record_estimates`: what ``record_fine`` and ``record_edges`` give, reduced on the device
ESTIMATES_DTYPE = np.dtype([("offset_hz", np.float64), ("coherence", np.float64), ("n_pairs", np.int32), ("level", np.float64), ("rise", np.float64),
                            ("fall", np.float64), ("n_inside", np.int32), ("r", np.complex128), ("pair_mag", np.float64)])
#: a row of :func:`input_levels`: what an operator reads off :meth:`BatchSignalAnalyzer.fetch_input_stats`
LEVELS_DTYPE = np.dtype([("dc_i", np.float64), ("dc_q", np.float64), ("power_dbfs", np.float64), ("rail_fraction", np.float64), ("peak", np.float64),
                         ("nonfinite", np.int64)])


def input_levels(stats) -> np.ndarray:
    """One ``LEVELS_DTYPE`` row per row of ``stats`` (``_native.INPUT_STATS_DTYPE``, :meth:`BatchSignalAnalyzer.fetch_input_stats`),
    in VALUE units (raw / ``unit``: full scale is 1): ``dc_i``, ``dc_q`` the mean of each component, ``power_dbfs`` =
    ``10 log10(sum_sq / (n unit^2))`` (0 dBFS: a complex tone of amplitude 1; both components square from rail to rail: +3 dB; -inf for silence), ``rail_fraction`` =
    ``n_rail / (2 n)`` the share of components at full scale, ``peak`` the largest ``|component|``, ``nonfinite`` the NaN and
    infinite components.  The means are over all ``2 n`` components' slots, the non-finite ones counting as absent values; a
    stream without samples (``n_samples == 0``: absent from the call, or an empty buffer) has NaN in every float field."""
    st = np.atleast_1d(np.asarray(stats))
    out = np.zeros(st.shape, dtype=LEVELS_DTYPE)
    n = st["n_samples"].astype(np.float64)
    unit = st["unit"].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        out["dc_i"] = st["sum_i"] / (n * unit)
        out["dc_q"] = st["sum_q"] / (n * unit)
        out["power_dbfs"] = 10.0 * np.log10(st["sum_sq"] / (n * unit * unit))
        out["rail_fraction"] = st["n_rail"] / (2.0 * n)
        out["peak"] = st["peak"] / unit
    out["nonfinite"] = st["n_nonfinite"]
    for name in ("dc_i", "dc_q", "power_dbfs", "rail_fraction", "peak"):
        out[name][st["n_samples"] == 0] = np.nan
    return out


def _stft_frames(offsets, first_segment, nperseg: int, hop_div: int):
    """``(record, in_predecessor_part, position)`` of every frame ``fetch_record_stft(hop_div)`` delivers.  A record with
    ``first_segment < 0`` delivers its predecessor part first: all ``(-first_segment - 1) k + 1`` frames of it, or fewer where
    the record ends inside it."""
    offsets = np.asarray(offsets, dtype=np.int64)
    first = np.asarray(first_segment, dtype=np.int64)
    N, k = int(nperseg), int(hop_div)
    if k < 1 or N % k:
        raise ValueError(f"hop_div {k} must be >= 1 and divide nperseg {N}")
    h = N // k
    n = len(first)
    rec = np.repeat(np.arange(n), np.diff(offsets))
    j = np.arange(int(offsets[-1]) if len(offsets) else 0, dtype=np.int64) - offsets[rec]
    lead = np.where(first < 0, np.minimum((-first - 1) * k + 1, np.diff(offsets)), 0)  # frames of the predecessor part
    pred = j < lead[rec]
    pos = np.where(pred, first[rec] * N + j * h, np.maximum(first[rec], 0) * N + (j - lead[rec]) * h)
    return rec, pred, pos


def stft_frame_positions(offsets, first_segment, nperseg: int, hop_div: int) -> np.ndarray:
    """int64, one entry per frame of ``fetch_record_stft(hop_div)``: the frame's first sample relative to sample 0 of the call's
    buffer.  Frames of a record's predecessor part are negative, counted back from the end of the predecessor buffer's last whole
    segment as ``first_segment`` counts: segment ``-1`` starts at ``-nperseg``."""
    return _stft_frames(offsets, first_segment, nperseg, hop_div)[2]


def record_fine(offsets, first_segment, values, start, end, sample_rate: float, nperseg: int, hop_div: int = 1, fi=None) -> np.ndarray:
    """The pulse-pair estimate of :meth:`BatchSignalAnalyzer.fetch_record_fine` from what ``fetch_record_stft`` returns and the
    records' ``start`` / ``end``: one ``FINE_DTYPE`` row per record.  Over the record's own cells -- the segments ``[start, end)``
    that were delivered -- ``R = sum c[t + 1] * conj(c[t])``, ``offset_hz = angle(R) / (2 pi) * sample_rate / nperseg`` and
    ``coherence = |R| / sum |c[t + 1]| |c[t]|``.  The pair (segment -1, segment 0) is never used: the predecessor buffer's
    ragged remainder lies between the two.  A record with no pair left has NaN and ``n_pairs == 0``.  float64 arithmetic.

    ``hop_div`` k > 1: ``values`` are the frames of ``fetch_record_stft(hop_div=k)`` and ``fi`` (required) the records' bins.
    The pairs are consecutive frames of the same part that both lie wholly inside the record's own cells (``start * nperseg <=
    position`` and ``position + nperseg <= end * nperseg``); ``R`` is turned back by the bin's own rotation over one hop,
    ``exp(-2 pi i (fi mod k) / k)``, which the frame-local phase reference leaves in, and ``offset_hz = angle(R) / (2 pi) * k *
    sample_rate / nperseg``: unambiguous within ``k / 2`` bins either side."""
    offsets = np.asarray(offsets, dtype=np.int64)
    first_segment = np.asarray(first_segment, dtype=np.int64)
    n = len(first_segment)
    k = int(hop_div)
    out = np.zeros(n, dtype=FINE_DTYPE)
    out["offset_hz"] = out["coherence"] = np.nan
    v = np.asarray(values).astype(np.complex128)
    if k != 1 and fi is None:
        raise ValueError("record_fine with hop_div > 1 needs the records' bins (fi)")
    if n == 0 or v.size < 2:
        return out
    if k == 1:
        rec = np.repeat(np.arange(n), np.diff(offsets))  # the record of every delivered cell
        seg = np.arange(v.size) - offsets[rec] + first_segment[rec]  # ... and its segment
        own = (seg >= np.asarray(start, dtype=np.int64)[rec]) & (seg < np.asarray(end, dtype=np.int64)[rec])
        pair = own[:-1] & own[1:] & (rec[:-1] == rec[1:]) & (seg[:-1] != -1)
    else:
        rec, pred, pos = _stft_frames(offsets, first_segment, nperseg, k)
        own = (pos >= np.asarray(start, dtype=np.int64)[rec] * int(nperseg)) & (pos + int(nperseg) <= np.asarray(end, dtype=np.int64)[rec] * int(nperseg))
        pair = own[:-1] & own[1:] & (rec[:-1] == rec[1:]) & (pred[:-1] == pred[1:])
    at = rec[:-1][pair]
    prod = (v[1:] * np.conj(v[:-1]))[pair]
    mag = (np.abs(v[1:]) * np.abs(v[:-1]))[pair]
    R = np.bincount(at, weights=prod.real, minlength=n) + 1j * np.bincount(at, weights=prod.imag, minlength=n)
    M = np.bincount(at, weights=mag, minlength=n)
    cnt = np.bincount(at, minlength=n)
    has = cnt > 0
    out["n_pairs"] = cnt
    if k != 1:
        R = R * np.exp(-2j * np.pi * (np.asarray(fi, dtype=np.int64) % k) / k)
    out["offset_hz"][has] = np.angle(R[has]) / (2.0 * np.pi) * k * float(sample_rate) / int(nperseg)
    with np.errstate(divide="ignore", invalid="ignore"):
        out["coherence"][has] = np.abs(R[has]) / M[has]
    return out


def record_edges(offsets, first_segment, values, start, end, nperseg: int, hop_div: int) -> np.ndarray:
    """float64 ``[n_records, 2]``: ``(rise, fall)`` of every record's pulse in samples relative to sample 0 of the call's buffer,
    from the frames of ``fetch_record_stft(hop_div)``.  ``level`` is the median of ``|c|`` over the frames that lie wholly inside
    the record's own cells (``start * nperseg <= position``, ``position + nperseg <= end * nperseg``).  ``rise``: from the first
    such frame that reaches ``level / 2`` (the first of them, but for a pulse that is still rising there) back, within its part,
    to the first frame with ``|c| < level / 2``; ``|c|`` is interpolated linearly between that frame and its successor, and half
    a window, ``nperseg / 2``, is added: a frame's value weighs the samples about its centre.  ``fall``: the mirror image forward
    from the last such frame.  NaN where the part ends before ``|c|`` falls below ``level / 2`` (margin 0, a pulse cut by the
    buffer's end) and for a record without a frame inside its own cells."""
    N, k = int(nperseg), int(hop_div)
    rec, pred, pos = _stft_frames(offsets, first_segment, N, k)
    offsets = np.asarray(offsets, dtype=np.int64)
    n = len(offsets) - 1
    a = np.abs(np.asarray(values).astype(np.complex128))
    start = np.asarray(start, dtype=np.int64)
    end = np.asarray(end, dtype=np.int64)
    out = np.full((n, 2), np.nan)
    for i in range(n):
        lo, hi = int(offsets[i]), int(offsets[i + 1])
        ai, pi, parti = a[lo:hi], pos[lo:hi], pred[lo:hi]
        inside = np.flatnonzero((pi >= start[i] * N) & (pi + N <= end[i] * N))
        if not len(inside):
            continue
        half = 0.5 * float(np.median(ai[inside]))
        if not half > 0:
            continue
        up = inside[ai[inside] >= half]
        for col, q, step in ((0, int(up[0]), -1), (1, int(up[-1]), 1)):
            part = parti[q]
            q += step
            while 0 <= q < len(ai) and parti[q] == part and not ai[q] < half:
                q += step
            if not (0 <= q < len(ai)) or parti[q] != part:
                continue  # the part ends first
            p = q - step  # the frame next to q on the pulse's side: |c| >= level / 2 there
            t = (half - ai[q]) / (ai[p] - ai[q])
            out[i, col] = pi[q] + t * (pi[p] - pi[q]) + 0.5 * N
    return out


def band_bins(fi, half_width: int, nperseg: int) -> np.ndarray:
    """int64 ``[n, 2 * half_width + 1]``: the bin of every column of :meth:`BatchSignalAnalyzer.fetch_record_band` for records at
    the bins ``fi`` -- column ``j`` is ``(fi + j - half_width) mod nperseg`` in fftfreq order; the band is circular."""
    w, N = int(half_width), int(nperseg)
    if w < 0 or 2 * w + 1 > N:
        raise ValueError(f"half_width {w} must be >= 0 with 2 * half_width + 1 <= nperseg {N}")
    return (np.atleast_1d(np.asarray(fi, dtype=np.int64))[:, None] + np.arange(-w, w + 1, dtype=np.int64)[None, :]) % N


def record_band_spectrum(offsets, first_segment, values, start, end, nperseg: int, hop_div: int = 1) -> np.ndarray:
    """float64 ``[n_records, 2 w + 1]``: the pulse's spectrum around its bin -- per column of
    :meth:`BatchSignalAnalyzer.fetch_record_band` the mean of ``|value| ** 2`` over the frames that lie wholly inside the record's
    own cells (``start * nperseg <= position`` and ``position + nperseg <= end * nperseg``, the rule of
    :meth:`BatchSignalAnalyzer.fetch_record_estimates`).  A record without such a frame has a NaN row."""
    offsets = np.asarray(offsets, dtype=np.int64)
    v = np.asarray(values)
    if v.ndim != 2:
        raise ValueError("values must be [n_frames, 2 * half_width + 1], as fetch_record_band returns them")
    n, N = len(offsets) - 1, int(nperseg)
    out = np.full((n, v.shape[1]), np.nan)
    if n == 0 or not len(v):
        return out
    rec, _, pos = _stft_frames(offsets, first_segment, N, hop_div)
    own = (pos >= np.asarray(start, dtype=np.int64)[rec] * N) & (pos + N <= np.asarray(end, dtype=np.int64)[rec] * N)
    p = v.real.astype(np.float64) ** 2 + v.imag.astype(np.float64) ** 2
    cnt = np.bincount(rec[own], minlength=n)
    for j in range(v.shape[1]):
        total = np.bincount(rec[own], weights=p[own, j], minlength=n)
        out[cnt > 0, j] = total[cnt > 0] / cnt[cnt > 0]
    return out


#: a row of :meth:`BatchSignalAnalyzer.fetch_record_spectrum` and of :func:`record_band_rows` (``_native.SPECTRUM_DTYPE``)
SPECTRUM_DTYPE = _native.SPECTRUM_DTYPE


def record_band_rows(offsets, first_segment, values, start, end, nperseg: int, hop_div: int = 1):
    """``(rows, mean, peak)`` from what :meth:`BatchSignalAnalyzer.fetch_record_band` returns and the records' ``start`` /
    ``end``: the definition :meth:`BatchSignalAnalyzer.fetch_record_spectrum` is held to within round-off, in plain NumPy.
    Over the frames that lie wholly inside the record's own cells (the rule of :func:`record_band_spectrum`), per column ``j``
    of ``p = re ** 2 + im ** 2`` in float64: ``mean[i, j]`` its mean and ``peak[i, j]`` its largest value (a NaN propagates).
    ``rows`` is one ``SPECTRUM_DTYPE`` row per record from the means ``m`` with ``d = j - w``: ``total = sum m``,
    ``centre_share = m[w] / total``, ``centroid = sum m d / total``, ``width = sqrt(sum m (d - centroid) ** 2 / total)`` (both
    in bins), ``peak_col`` the lowest column of the largest mean, and ``peak_bins`` the vertex of the parabola through the
    logarithms of the three means around it -- exact for a Gaussian main lobe -- where ``peak_col`` is no edge column and the
    three are finite and positive, else NaN.  A record without an inside frame, or with a NaN mean, has NaN in every scalar and
    ``peak_col == -1``."""
    offsets = np.asarray(offsets, dtype=np.int64)
    v = np.asarray(values)
    if v.ndim != 2 or v.shape[1] % 2 != 1:
        raise ValueError("values must be [n_frames, 2 * half_width + 1], as fetch_record_band returns them")
    n, N, B = len(offsets) - 1, int(nperseg), v.shape[1]
    w = B // 2
    rows = np.zeros(n, dtype=SPECTRUM_DTYPE)
    for name in ("total", "centre_share", "centroid", "width", "peak_bins"):
        rows[name] = np.nan
    rows["peak_col"] = -1
    mean = np.full((n, B), np.nan)
    peak = np.full((n, B), np.nan)
    if n == 0:
        return rows, mean, peak
    rec, _, pos = _stft_frames(offsets, first_segment, N, hop_div)
    own = (pos >= np.asarray(start, dtype=np.int64)[rec] * N) & (pos + N <= np.asarray(end, dtype=np.int64)[rec] * N)
    with np.errstate(all="ignore"):
        p = v.real.astype(np.float64) ** 2 + v.imag.astype(np.float64) ** 2
        d = np.arange(-w, w + 1, dtype=np.float64)
        for i in range(n):
            mine = p[offsets[i]:offsets[i + 1]][own[offsets[i]:offsets[i + 1]]]
            rows["n_inside"][i] = len(mine)
            if not len(mine):
                continue
            m = mean[i] = mine.mean(axis=0)
            peak[i] = mine.max(axis=0)
            if np.isnan(m).any():
                continue
            total = m.sum()
            centroid = (m * d).sum() / total
            col = int(np.argmax(m))
            rows["total"][i], rows["centre_share"][i], rows["centroid"][i] = total, m[w] / total, centroid
            rows["width"][i] = np.sqrt((m * (d - centroid) ** 2).sum() / total)
            rows["peak_col"][i] = col
            if 0 < col < 2 * w and np.isfinite(m[col - 1:col + 2]).all() and (m[col - 1:col + 2] > 0).all():
                a, b, c = np.log(m[col - 1:col + 2])
                rows["peak_bins"][i] = d[col] + 0.5 * (a - c) / (a - 2.0 * b + c)
    return rows, mean, peak


def spectrum_hz(rows, sample_rate: float, nperseg: int) -> np.ndarray:
    """A copy of the ``SPECTRUM_DTYPE`` rows with ``centroid``, ``width`` and ``peak_bins`` scaled from bins to Hz
    (``sample_rate / nperseg`` a bin); the other fields are unchanged."""
    out = np.array(rows, dtype=SPECTRUM_DTYPE, copy=True)
    for name in ("centroid", "width", "peak_bins"):
        out[name] = out[name] * (float(sample_rate) / int(nperseg))
    return out


def default_lanes(fft_nperseg: int, n_streams: int) -> int:
    """Stream groups per GPU (``rt_config.lanes``) that measured best: three up to nperseg 512 while the launches of a group are
    small enough to have ends worth filling by another group's kernels (fewer than 16 384 streams on the GPU) -- config 2 +14 % with
    two lanes and another +1.5 % with three, the reference's defaults under a noise floor +3 ... 4 % over two; four lanes -16 % at
    config 2 (the HIP runtime's four hardware queues: with GPU_MAX_HW_QUEUES=8 four lanes equal three, six lose); one lane from nperseg 1024 on, where the scans are chip-filling grids of persistent workgroups (config 3: 676 k
    MSamples/s with one lane, 650 k with two).  ``profiles/r05_n_lanes_by_batch_size.txt``; ``bench.py`` uses the same rule."""
    return 3 if (fft_nperseg <= 512 and 3 <= n_streams < 16384) else 1


def _per_stream(name: str, value, devices: Sequence[str]):
    """A keyword that may be given per stream: ``None`` for a scalar, else its values as a list (one per device)."""
    if not np.ndim(value):
        return None
    values = list(value)
    if len(values) != len(devices):
        raise ValueError(f"{name} values {values} do not match devices {list(devices)}")
    return values


class BatchSignalAnalyzer:
    """``S`` independent analyzers on one GPU, one per device as in the reference (``__main__.py:140-141``).  They share the
    STFT -- ``sample_rate``, ``fft_nperseg`` and ``fft_window`` set the scan's geometry and scale and stay per handle -- while
    every detection setting may differ per stream: ``calibration_db``, ``signal_threshold_dbw``, ``snr_threshold_db``,
    ``signal_min_duration_ms``, ``signal_max_duration_ms`` and ``center_freq`` each take one value, or one per device.

    ``process_batch`` is the batched body of the reference callback
    (analyze.py:231-251, 268) for one buffer of every stream.  Per-stream
    carried state (the look-back tail replacing ``_spectrogram_last``) lives in
    HBM inside the native handle.
    """

    chain = 0  # links per run (``chain=L``), 0: every stream is a device of its own

    def __init__(
        self,
        devices: Sequence[str],
        calibration_db: Union[float, Sequence[float]] = 0.0,
        sample_rate: int = 300000,
        center_freq: int = 150150000,
        fft_nperseg: int = 256,
        fft_window="hamming",
        signal_min_duration_ms: float = 8,
        signal_max_duration_ms: float = 40,
        signal_threshold_dbw: float = -90.0,
        snr_threshold_db: float = 5.0,
        sdr_callback_length: Optional[int] = None,
        gpu: int = 0,
        mode: str = "auto",
        hot_capacity: int = 0,
        record_capacity: int = 0,
        segs_per_chunk: int = 0,
        timing: bool = False,
        hip_stream: Optional[int] = None,
        lanes: Union[int, str] = 1,
        subtract_first: bool = False,
        record_pool: int = 0,
        group_detect: Optional[bool] = None,
        precision: str = "float32",
        row_means: bool = False,
        record_cells: bool = False,
        f64_sparse: bool = False,
        f64_rescue: bool = False,
        chain: int = 0,
        record_iq: bool = False,
        record_iq_margin: int = 0,
        input_stats: bool = False,
        **kwargs,
    ):
        """``input_stats`` (``rt_set_input_stats``): every enqueued buffer is also read once by a streaming kernel of its own that
        leaves, per stream, the level, DC, clipping and non-finite counts of the RAW input (:meth:`fetch_input_stats`,
        :func:`input_levels`).  On every kind of analyzer; the analysis itself is unchanged.

        ``record_iq`` (``rt_set_record_iq``): keep the sample tail of every stream's previous buffer, so that
        :meth:`fetch_record_iq` can hand out the IQ samples behind every record of a call, ``record_iq_margin`` whole segments
        on either side included.  On every kind of analyzer (any ``mode``, ``lanes``, ``chain``, ``precision``).

        ``chain=L`` (``rt_set_chain``, ``L >= 2``): every device is a RECORDING, analysed ``L`` consecutive buffers per call.
        The handle has ``len(devices) * L`` streams -- run ``r`` (streams ``r * L ... r * L + L - 1``, :meth:`run_of` /
        :meth:`link_of`) holds device ``r``'s buffers of a call in time order, each looking back into the one before it, the
        first into the run's last buffer of the call before.  ``devices`` then lists every STREAM's device name (each name ``L``
        times), ``run_devices`` the names as given; per-device values are repeated over the run.  ``enqueue*`` take
        ``[R, l * B]`` with ``l <= L`` (``links=l``, or ``B = sdr_callback_length``; ``l < L``: the run's last ``L - l``
        streams sit the call out), :meth:`process_batch` returns per device the signals of all its links in time order.
        ``lanes`` is 1 (an explicit ``lanes > 1``: ``ValueError``, a run could straddle two lanes), and so is
        ``precision="float64"``.

        ``record_cells`` (``RT_FLAG_RECORD_CELLS``): keep the spectrogram cells every record of a call consists of -- the
        reference's ``data`` (analyze.py:437-440), which it reduces to max / mean / std and drops -- for
        :meth:`fetch_record_cells`.

        ``row_means`` (``RT_FLAG_ROW_MEANS``): keep every bin's noise level, the reference's ``freq_avg = np.mean(row)``
        (analyze.py:373-375), of each call for :meth:`fetch_row_means` -- not only of the bins a signal was found in.

        ``precision``: ``"float32"`` (default) analyses complex64; ``"float64"`` runs the reference's float64 arithmetic on
        complex128 buffers (what pyrtlsdr delivers) -- float64 window, scale, thresholds, map and statistics
        (``rt_create_f64``).  A float64 analyzer runs the dense path only (``mode`` ``"auto"`` or ``"dense"``), nperseg 8 ...
        4096 or a power of two up to 8192, one lane; ``enqueue`` takes complex128 device tensors, host complex arrays
        (complex64 widened exactly) and uint8 (converted as pyrtlsdr does, in float64); ``fetch_records`` returns
        ``RECORD_F64_DTYPE``.

        ``f64_sparse`` (``RT_FLAG_F64_SPARSE``; needs ``precision="float64"``, ``mode="auto"`` and no ``record_cells``, else
        ``ValueError``): the float64 analyzer without its float64 map -- a fused scan emits only candidate cells and the
        detection works from those lists; nperseg a power of two 32 ... 4096.  ``hot_capacity`` then
        counts candidate cells per stream and call (0: 4096; 1024 ... 8192); a stream that emits more makes
        ``fetch_records`` raise ``RT_E_HOT_OVERFLOW`` for that call.  ``segs_per_chunk``: segments a scan workgroup walks.

        ``f64_rescue`` (``RT_FLAG_F64_RESCUE``; needs ``f64_sparse=True``, else ``ValueError``): such a stream no longer costs
        the call -- ``fetch_records`` analyses the overflowing streams again on their own from a per-stream float64 map in a
        scratch area and delivers what a large enough ``hot_capacity`` would have, byte for byte;
        ``call_info()`` reports them as ``n_dense_streams`` / ``fell_back``.  A call without such a stream runs what it runs
        without the flag.

        ``mode`` (``rt_config.mode``): ``"auto"`` (default) analyses on the fused sparse path and, when an input's noise
        crosses the thresholds, climbs by itself -- chunk-bit pre-filter, exact SNR-aware pre-filter, dense spectrogram; the
        records are the same on every level.  ``"sparse"``, ``"prefilter"``, ``"runfilter"`` and
        ``"dense"`` pin one level (the first three refuse an input they cannot hold with ``RT_E_HOT_OVERFLOW``).

        ``record_pool`` (``rt_config.record_pool``): records the pinned result pool holds at first (0: up to 4 Mi); a
        buffer with more signals grows it -- the reference appends without limit (``analyze.py:449-450``); so does the
        per-stream ``record_capacity`` (where a stream's room STARTS, default 1024): nothing bounds a call but memory.

        ``subtract_first``: apply SciPy's ``detrend='constant'`` in SciPy's order (segment mean subtracted before
        the window) even for hamming / hann / boxcar windows, where the kernels by default subtract ``mean * FFT(window)``
        from the three bins it touches instead (equal within float32 round-off, fewer operations).

        ``group_detect`` (``RT_FLAG_GROUP_DETECT`` / ``RT_FLAG_NO_GROUP_DETECT``): sparse detection with one wave per stream or
        quarter of a stream's sixteen candidate lists instead of one per list -- the same records; ``None`` (default) lets the
        library decide (from 1 024 streams per handle on, where the lists are many and short).

        ``lanes`` > 1 (``rt_config.lanes``) splits the streams into that many contiguous groups, each
        analysed on its own HIP stream: the detection kernels and launch gaps of one group then overlap the
        scan of another (config 2: +14 % whole-path throughput with two lanes).  Streams are independent,
        so the records are the same; ``rt_fetch`` returns them in stream order.  Needs ``hip_stream=None``.
        ``lanes="auto"`` takes what the sweeps of round 5 found best (``default_lanes``: three up to nperseg 512 while the
        batch holds fewer than 16 384 streams, one otherwise and whenever a ``hip_stream`` is given).

        ``calibration_db`` may be a sequence with one value per stream: every SDR of the reference has its own
        analyzer and calibration (``__main__.py:140-141``), and with it its own absolute threshold
        (``analyze.py:115``); the kernels then take the thresholds per stream (``rt_set_stream_params``).

        ``signal_threshold_dbw``, ``snr_threshold_db``, ``signal_min_duration_ms``, ``signal_max_duration_ms`` and
        ``center_freq`` may be sequences as well, one value per device (``analyze.py:113-116``, ``:360``): the attributes
        (``signal_threshold``, ``snr_threshold``, ``signal_min_duration``, ...) are then lists.  The handle is created with the
        envelope of the durations -- the smallest minimum, the largest maximum: look-back depth and pre-filters derive from it
        -- and every stream is gated by its own values (``rt_set_stream_settings``); :meth:`set_stream_settings` changes them
        later, inside that envelope."""
        self.run_devices = [str(d) for d in devices]
        self.chain = int(chain) if chain and int(chain) >= 2 else 0
        self._chain_call = (self.chain, 0)  # links and samples per link of the buffer enqueued last
        if self.chain:
            if precision == "float64":
                raise ValueError("chain is not available with precision='float64'")
            if lanes != "auto" and int(lanes) > 1:
                raise ValueError("chain needs lanes=1: lanes cut the streams into groups that a run may straddle")
            lanes = 1

            def over_run(v):  # a per-device sequence -> one value per stream
                return [x for x in v for _ in range(self.chain)] if np.ndim(v) else v

            devices = over_run(self.run_devices)
            calibration_db, center_freq = over_run(calibration_db), over_run(center_freq)
            signal_threshold_dbw, snr_threshold_db = over_run(signal_threshold_dbw), over_run(snr_threshold_db)
            signal_min_duration_ms, signal_max_duration_ms = over_run(signal_min_duration_ms), over_run(signal_max_duration_ms)
        self.devices = [str(d) for d in devices]
        # (a sequence of the wrong length is refused before anything native is touched)
        per_thr = _per_stream("signal_threshold_dbw", signal_threshold_dbw, self.devices)
        per_snr = _per_stream("snr_threshold_db", snr_threshold_db, self.devices)
        per_min = _per_stream("signal_min_duration_ms", signal_min_duration_ms, self.devices)
        per_max = _per_stream("signal_max_duration_ms", signal_max_duration_ms, self.devices)
        per_center = _per_stream("center_freq", center_freq, self.devices)
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {PRECISIONS}, not {precision!r}")
        self.precision = precision
        f64 = precision == "float64"
        if f64_sparse:
            if not f64:
                raise ValueError("f64_sparse needs precision='float64'")
            if mode != "auto":
                raise ValueError("f64_sparse selects the path by itself: mode must be 'auto'")
            if record_cells:
                raise ValueError("f64_sparse keeps no map: record_cells is not available with it")
        if f64_rescue and not f64_sparse:
            raise ValueError("f64_rescue re-runs the overflowing streams of the map-free path: it needs f64_sparse=True")
        self.f64_sparse = bool(f64_sparse)
        self.f64_rescue = bool(f64_rescue)
        per_stream_cal = None
        if np.ndim(calibration_db):
            per_stream_cal = [float(c) for c in calibration_db]
            if len(per_stream_cal) != len(self.devices):
                raise ValueError(f"calibration values {per_stream_cal} do not match devices {self.devices}")  # __main__.py:219
            calibration_db = per_stream_cal[0]
        self.calibration_db = calibration_db
        self.sample_rate = sample_rate
        self.center_freq = per_center if per_center is not None else center_freq
        if sdr_callback_length is None:  # analyze.py:108-109
            sdr_callback_length = sample_rate
        self.sdr_callback_length = int(sdr_callback_length)
        self.fft_nperseg = fft_nperseg
        self.fft_window = fft_window
        # per-stream values as lists; the handle's own (rt_config) are the envelope of the durations and the first stream's thresholds
        self.signal_min_duration = [v / 1000 for v in per_min] if per_min else signal_min_duration_ms / 1000  # :113
        self.signal_max_duration = [v / 1000 for v in per_max] if per_max else signal_max_duration_ms / 1000  # :114
        self.snr_threshold = [from_dB(v) for v in per_snr] if per_snr else from_dB(snr_threshold_db)  # :116
        self._min_envelope = min(self.signal_min_duration) if per_min else self.signal_min_duration
        self._max_envelope = max(self.signal_max_duration) if per_max else self.signal_max_duration
        snr0 = self.snr_threshold[0] if per_snr else self.snr_threshold
        self.signal_threshold = from_dB((per_thr[0] if per_thr else signal_threshold_dbw) + calibration_db)  # :115

        if f64:
            win32, scale32 = stft_constants_f64(fft_window, fft_nperseg, sample_rate)
        else:
            win32, scale32 = stft_constants(fft_window, fft_nperseg, sample_rate)
        if lanes == "auto":
            lanes = 1 if (hip_stream is not None or f64) else default_lanes(fft_nperseg, len(self.devices))
        if int(lanes) > 1 and hip_stream is not None:
            raise ValueError("lanes > 1 run on their own HIP streams: pass hip_stream=None")
        self._present = None       # the presence mask in force (set_present): None = every stream ...
        self._present_set = False  # ... and whether the native entry has been called at all
        self._native = _native.NativeAnalyzer(
            n_streams=len(self.devices),
            nperseg=fft_nperseg,
            max_samples=self.sdr_callback_length,
            sample_rate=sample_rate,
            window_f32=win32,
            scale=float(scale32),
            # thresholds are compared against float32 data in float32; a float64 handle keeps the Python floats
            threshold=float(self.signal_threshold) if f64 else float(np.float32(self.signal_threshold)),
            snr_threshold=float(snr0) if f64 else float(np.float32(snr0)),
            calibration_db=calibration_db,
            min_duration_s=self._min_envelope,
            max_duration_s=self._max_envelope,
            device=gpu,
            mode={"auto": _native.RT_MODE_AUTO, "dense": _native.RT_MODE_DENSE, "sparse": _native.RT_MODE_SPARSE, "prefilter": _native.RT_MODE_PREFILTER,
                  "runfilter": _native.RT_MODE_RUNFILTER}[mode],
            hot_capacity=hot_capacity,
            record_capacity=record_capacity,
            segs_per_chunk=segs_per_chunk,
            timing=timing,
            hip_stream=hip_stream,
            lanes=max(1, int(lanes)),
            subtract_first=bool(subtract_first),
            record_pool=int(record_pool),
            group_detect=group_detect,
            precision=precision,
            row_means=bool(row_means),
            record_cells=bool(record_cells),
            f64_sparse=self.f64_sparse,
            f64_rescue=self.f64_rescue,
        )
        if per_stream_cal is not None or per_thr is not None:
            n = len(self.devices)
            cals = per_stream_cal if per_stream_cal is not None else [calibration_db] * n
            dbws = per_thr if per_thr is not None else [signal_threshold_dbw] * n
            self.signal_threshold = [from_dB(t + c) for t, c in zip(dbws, cals)]  # :115, per SDR
            if per_stream_cal is not None:
                self.calibration_db = per_stream_cal
            cal_arr = None if per_stream_cal is None else np.array(per_stream_cal, dtype=np.float64 if f64 else np.float32)
            if f64:
                self._native.set_stream_params(np.array(self.signal_threshold, dtype=np.float64), cal_arr)
            else:
                self._native.set_stream_params(np.array(self.signal_threshold, dtype=np.float64).astype(np.float32), cal_arr)
        if per_snr is not None or per_min is not None or per_max is not None:
            self._push_stream_settings()
        if self.chain:
            self._native.set_chain(self.chain)
        self.record_iq = bool(record_iq)
        self.record_iq_margin = int(record_iq_margin)
        if self.record_iq:
            if not 0 <= self.record_iq_margin <= 1024:
                raise ValueError("record_iq_margin must be 0 ... 1024 segments")
            self._native.set_record_iq(self.record_iq_margin)
        self.input_stats = bool(input_stats)
        if self.input_stats:
            self._native.set_input_stats(True)
        self._decoder = _RecordDecoder(fft_nperseg, sample_rate, self.center_freq, self.calibration_db, f64=f64)
        self.decoder = self._decoder  # record -> field conversion, shared with pyradiotracking_amd.match
        self.gpu = gpu
        self._hip_stream = hip_stream

    # -- native plumbing ----------------------------------------------------
    @property
    def native(self) -> "_native.NativeAnalyzer":
        return self._native

    def _hold(self, tensor):
        # two calls may be in flight: keep the device buffers of both alive (torch's caching
        # allocator would otherwise hand the memory to someone else while the scan still reads it)
        held = getattr(self, "_held", [])
        self._held = (held + [tensor])[-2:]

    def reset(self):
        """``_spectrogram_last = None`` for every stream."""
        self._native.reset()

    def reset_stream(self, stream: int):
        """``_spectrogram_last = None`` for one stream: its SDR was restarted, i.e. the reference would have
        replaced its analyzer by a fresh one (``__main__.py:185-190``)."""
        self._native.reset_stream(stream)

    def set_present(self, present=None):
        """Which streams take part in the buffers enqueued from now on (``rt_set_present``): one bool per device, or ``None`` =
        all of them.  In the reference every SDR is a ``SignalAnalyzer`` of its own, whose callback comes when *its* radio
        delivers; a stream that is absent from a call is not read, finds nothing and keeps its state -- its next present buffer
        looks back into its own last present one, exactly as a reference analyzer that was not called in between, after any
        number of absent calls; a pending :meth:`reset_stream` or changed setting takes effect then.  Sticky; may be called
        with buffers in flight (each keeps the mask it was enqueued with); returns at once when the mask equals the one in
        force.  An all-true mask on an analyzer that never had another one is such a case: the native entry is not called and the
        handle stays on its one-count path (``native.set_present`` calls it regardless).  ``extract_signals`` and the spectrogram
        entries ignore it."""
        n = len(self.devices)
        if present is not None:
            present = tuple(bool(p) for p in present)
            if len(present) != n:
                raise ValueError(f"present {list(present)} does not match devices {list(self.devices)}.")
            if all(present) and not self._present_set:
                return  # (never masked, and every stream stays: the handle is left on its one-count path)
        if self._present_set and present == self._present:
            return
        self._native.set_present(None if present is None else np.array(present, dtype=bool))
        self._present = present
        self._present_set = True

    def _push_stream_settings(self):
        """The per-stream attributes -> ``rt_set_stream_settings`` (scalars stay the handle's own: null arrays).  The SNR
        threshold is rounded as the handle compares it: float32 on a float32 handle, like the scalar path; Python floats on a
        float64 handle."""
        f64 = self.precision == "float64"
        snr = lo = hi = None
        if np.ndim(self.snr_threshold):
            snr = np.array(self.snr_threshold, dtype=np.float64)
            if not f64:
                snr = snr.astype(np.float32)
        if np.ndim(self.signal_min_duration):
            lo = np.array(self.signal_min_duration, dtype=np.float64)
        if np.ndim(self.signal_max_duration):
            hi = np.array(self.signal_max_duration, dtype=np.float64)
        self._native.set_stream_settings(snr, lo, hi)

    def set_stream_settings(self, snr_threshold_db=None, signal_min_duration_ms=None, signal_max_duration_ms=None):
        """Change the streams' SNR thresholds and duration gates (``rt_set_stream_settings``): each argument one value for
        every stream, one per device, or ``None`` = as it is.  The durations must stay inside the envelope the analyzer was
        built with (smallest minimum, largest maximum); no call may be pending.  A stream whose settings change starts its
        next buffer without look-back -- in the reference new settings mean a new analyzer (``analyze.py:113-116, 128``) --,
        the others keep theirs.  A refused call (``ValueError`` for a wrong length, ``NativeError`` otherwise) changes nothing."""
        n = len(self.devices)

        def values(name, v, conv):
            if self.chain and np.ndim(v) and len(v) == len(self.run_devices):
                v = [x for x in v for _ in range(self.chain)]  # one value per recording: the same for every link of its run
            per = _per_stream(name, v, self.devices)
            return [conv(x) for x in (per if per is not None else [v] * n)]

        old = (self.snr_threshold, self.signal_min_duration, self.signal_max_duration)
        if snr_threshold_db is not None:
            self.snr_threshold = values("snr_threshold_db", snr_threshold_db, from_dB)
        if signal_min_duration_ms is not None:
            self.signal_min_duration = values("signal_min_duration_ms", signal_min_duration_ms, lambda x: x / 1000)
        if signal_max_duration_ms is not None:
            self.signal_max_duration = values("signal_max_duration_ms", signal_max_duration_ms, lambda x: x / 1000)
        try:
            self._push_stream_settings()
        except Exception:
            self.snr_threshold, self.signal_min_duration, self.signal_max_duration = old
            raise

    # -- chain=L: consecutive buffers of a recording as the streams of a call ------------------------------------------
    def run_of(self, stream):
        """The recording (index into ``run_devices``) stream ``stream`` belongs to; arrays as well (``rec["stream"]``)."""
        return stream // self.chain if self.chain else stream

    def link_of(self, stream):
        """The buffer number of ``stream`` inside its call (0 = the earliest); arrays as well."""
        return stream % self.chain if self.chain else stream * 0

    def _chain_rows(self, x, per_sample: int, links: Optional[int], n_samples: Optional[int] = None):
        """``[R, l * B]`` (``per_sample`` array elements a sample) -> the handle's ``[R * L, B]`` rows, link ``j`` of device ``r`` at
        row ``r * L + j``; ``l < L`` sets the suffix mask.  A raw device pointer is the caller's ``[R * L, stride]`` already."""
        L, R = self.chain, len(self.run_devices)
        if isinstance(x, int):
            l = L if links is None else int(links)
            if not 0 <= l <= L:
                raise ValueError(f"links must be 0 ... {L}")
            self._set_links(l, n_samples)
            return x
        is_np = isinstance(x, np.ndarray)
        if (x.ndim if is_np else x.dim()) == 1:
            x = x[None, :]
        if x.shape[0] != R or x.shape[1] % per_sample:
            raise ValueError(f"expected [{R}, links * B] samples: one row per recording")
        n, b0 = x.shape[1] // per_sample, self.sdr_callback_length
        if links is None:
            if n > b0 and n % b0:
                raise ValueError(f"{n} samples are no whole number of buffers of sdr_callback_length {b0}: pass links=")
            l = 1 if n <= b0 else n // b0
        else:
            l = int(links)
            if l < 1 or n % l:
                raise ValueError(f"{n} samples do not divide into links={links} buffers")
        if l > L:
            raise ValueError(f"{l} buffers per recording, the analyzer chains {L}")
        width = n // l * per_sample
        self._set_links(l, n // l)
        x = np.ascontiguousarray(x) if is_np else x.contiguous()
        if l == L:
            return x.reshape(R * L, width)
        if is_np:
            rows = np.zeros((R, L, width), dtype=x.dtype)
        else:
            import torch

            rows = torch.zeros((R, L, width), dtype=x.dtype, device=x.device)
        rows[:, :l] = x.reshape(R, l, width)
        return rows.reshape(R * L, width)

    def _set_links(self, l: int, n_samples: Optional[int]):
        self._chain_call = (l, n_samples)
        self.set_present([j < l for _ in self.run_devices for j in range(self.chain)])

    def close(self):
        """Destroy the native handle (waits for everything in flight), then let go of the device tensors the
        calls in flight may have been reading."""
        self._native.close()
        self._held = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def call_info(self):
        """Figures of the last fetched call (with lanes: counts and times summed over the lanes' launches)."""
        return self._native.call_info()

    def _process_device(self, ptr: int, n_samples: int, stride: Optional[int], bytes_per_sample: int, u8: bool, i16: bool = False, i8: bool = False):
        if i8:
            self._native.process_device_i8(ptr, n_samples, stride)
        elif i16:
            self._native.process_device_i16(ptr, n_samples, stride)
        elif u8:
            self._native.process_device_u8(ptr, n_samples, stride)
        else:
            self._native.process_device(ptr, n_samples, stride)

    def enqueue(self, iq, n_samples: Optional[int] = None, stream_stride: Optional[int] = None, links: Optional[int] = None):
        """Start analysing one buffer per stream (asynchronous).

        ``iq``: a CUDA/HIP torch tensor ``[S, B]`` complex64, a raw device
        pointer (int, with ``n_samples``), or a host ndarray ``[S, B]``.
        With ``chain=L``: ``[R, links * B]``, one row per recording (a device pointer: ``[R * L, stream_stride]`` with
        ``n_samples = B`` and ``links``); so for the other formats below.
        """
        if self.chain:
            if isinstance(iq, np.ndarray) and iq.dtype == np.uint8:
                self.enqueue_bytes(iq, links=links)
                return
            iq = self._chain_rows(iq, 1, links, n_samples)
        if isinstance(iq, int):
            if n_samples is None:
                raise ValueError("n_samples is required with a raw device pointer")
            self._process_device(iq, n_samples, stream_stride, 16 if self.precision == "float64" else 8, False)
            return
        if isinstance(iq, np.ndarray) and iq.dtype == np.uint8:
            self.enqueue_bytes(iq)
            return
        if isinstance(iq, np.ndarray):
            self._native.process_host(iq)
            return
        # torch tensor
        if iq.dim() == 1:
            iq = iq[None, :]
        if not iq.is_cuda:
            self.enqueue(iq.numpy())
            return
        want = "torch.complex128" if self.precision == "float64" else "torch.complex64"
        if str(iq.dtype) != want:
            raise TypeError(f"device IQ must be {want[6:]}" + (" on a float64 analyzer" if self.precision == "float64" else ""))
        if iq.shape[0] != len(self.devices) or iq.stride(1) != 1:
            raise ValueError("device IQ must be [S, B] with unit sample stride")
        self._hold(iq)
        if self._hip_stream is None:
            # the handle launches on its own stream: whatever torch still has in flight on
            # the producing stream must have landed before the scan kernel reads the IQ
            import torch

            torch.cuda.current_stream(iq.device).synchronize()
        self._process_device(iq.data_ptr(), iq.shape[1], iq.stride(0) if iq.shape[0] > 1 else iq.shape[1], iq.element_size(), False)

    def enqueue_bytes(self, raw, n_samples: Optional[int] = None, stream_stride: Optional[int] = None, links: Optional[int] = None):
        """Same as :meth:`enqueue` for the RTL-SDR wire format: interleaved uint8 I, Q (what
        librtlsdr delivers; pyrtlsdr's ``packed_bytes_to_iq`` turns it into the complex buffer
        the reference's callback sees).  ``raw``: host ndarray / CUDA torch tensor of uint8 shaped
        ``[S, 2*B]`` (or ``[2*B]`` for one stream), or a raw device pointer with ``n_samples``.
        The byte -> float conversion is fused into the scan kernel's load."""
        if self.chain:
            raw = self._chain_rows(raw, 2, links, n_samples)
        if isinstance(raw, int):
            if n_samples is None:
                raise ValueError("n_samples is required with a raw device pointer")
            self._process_device(raw, n_samples, stream_stride, 2, True)
            return
        if isinstance(raw, np.ndarray):
            a = np.ascontiguousarray(raw, dtype=np.uint8)
            if a.ndim == 1:
                a = a[None, :]
            if a.shape[0] != len(self.devices) or a.shape[1] % 2:
                raise ValueError("expected uint8 [S, 2*B]")
            if a.shape[1] // 2 > self.sdr_callback_length:
                raise ValueError("buffer longer than sdr_callback_length")
            # staged by the library: one device buffer per call in flight, kept until the call is fetched
            self._native.process_host_u8(a)
            return
        if raw.dim() == 1:
            raw = raw[None, :]
        if str(raw.dtype) != "torch.uint8" or not raw.is_cuda or raw.stride(1) != 1 or raw.shape[1] % 2:
            raise TypeError("device bytes must be a CUDA uint8 tensor [S, 2*B] with unit stride")
        self._hold(raw)
        if self._hip_stream is None:
            import torch

            torch.cuda.current_stream(raw.device).synchronize()
        stride = (raw.stride(0) if raw.shape[0] > 1 else raw.shape[1]) // 2
        self._process_device(raw.data_ptr(), raw.shape[1] // 2, stride, 2, True)

    def enqueue_int16(self, raw, n_samples: Optional[int] = None, stream_stride: Optional[int] = None, links: Optional[int] = None):
        """Same as :meth:`enqueue` for 16-bit signed IQ (SoapySDR ``CS16``, UHD ``sc16``, SigMF ``ci16_le``): interleaved
        little-endian int16 I, Q, a component's value ``i * 2**-15``.  ``raw``: host ndarray / CUDA torch tensor of int16 shaped
        ``[S, 2*B]`` (or ``[2*B]`` for one stream), or a raw device pointer (4-byte aligned) with ``n_samples``.  The conversion
        is exact and fused into the scan kernel's load: the results are those of :meth:`enqueue` on
        ``synth.i16_to_complex64(raw)`` (``i16_to_complex128`` on a float64 analyzer), byte for byte."""
        if self.chain:
            raw = self._chain_rows(raw, 2, links, n_samples)
        if isinstance(raw, int):
            if n_samples is None:
                raise ValueError("n_samples is required with a raw device pointer")
            self._process_device(raw, n_samples, stream_stride, 4, False, True)
            return
        if isinstance(raw, np.ndarray):
            if raw.dtype != np.int16:
                raise TypeError("expected an int16 array (interleaved I, Q)")
            a = np.ascontiguousarray(raw)
            if a.ndim == 1:
                a = a[None, :]
            if a.ndim != 2 or a.shape[0] != len(self.devices) or a.shape[1] % 2:
                raise ValueError("expected int16 [S, 2*B]")
            if a.shape[1] // 2 > self.sdr_callback_length:
                raise ValueError("buffer longer than sdr_callback_length")
            # staged by the library: one device buffer per call in flight, kept until the call is fetched
            self._native.process_host_i16(a)
            return
        if raw.dim() == 1:
            raw = raw[None, :]
        if str(raw.dtype) != "torch.int16" or not raw.is_cuda or raw.dim() != 2 or raw.stride(1) != 1 or raw.shape[1] % 2:
            raise TypeError("device samples must be a CUDA int16 tensor [S, 2*B] with unit stride")
        if raw.shape[0] != len(self.devices) or (raw.shape[0] > 1 and raw.stride(0) % 2):
            raise ValueError("device samples must be int16 [S, 2*B], a whole number of samples from stream to stream")
        if raw.shape[1] // 2 > self.sdr_callback_length:
            raise ValueError("buffer longer than sdr_callback_length")
        self._hold(raw)
        if self._hip_stream is None:
            import torch

            torch.cuda.current_stream(raw.device).synchronize()
        stride = (raw.stride(0) if raw.shape[0] > 1 else raw.shape[1]) // 2
        self._process_device(raw.data_ptr(), raw.shape[1] // 2, stride, 4, False, True)

    def enqueue_int8(self, raw, n_samples: Optional[int] = None, stream_stride: Optional[int] = None, links: Optional[int] = None):
        """Same as :meth:`enqueue` for 8-bit signed IQ (HackRF's native format, SoapySDR ``CS8``, UHD ``sc8``, SigMF ``ci8``):
        interleaved two's-complement int8 I, Q, a component's value ``i * 2**-7``.  ``raw``: host ndarray / CUDA torch tensor of int8
        shaped ``[S, 2*B]`` (or ``[2*B]`` for one stream), or a raw device pointer (2-byte aligned) with ``n_samples``.  The conversion
        is exact and fused into the scan kernel's load: the results are those of :meth:`enqueue` on
        ``synth.i8_to_complex64(raw)`` (``i8_to_complex128`` on a float64 analyzer), byte for byte."""
        if self.chain:
            raw = self._chain_rows(raw, 2, links, n_samples)
        if isinstance(raw, int):
            if n_samples is None:
                raise ValueError("n_samples is required with a raw device pointer")
            self._process_device(raw, n_samples, stream_stride, 2, False, False, True)
            return
        if isinstance(raw, np.ndarray):
            if raw.dtype != np.int8:
                raise TypeError("expected an int8 array (interleaved I, Q)")
            a = np.ascontiguousarray(raw)
            if a.ndim == 1:
                a = a[None, :]
            if a.ndim != 2 or a.shape[0] != len(self.devices) or a.shape[1] % 2:
                raise ValueError("expected int8 [S, 2*B]")
            if a.shape[1] // 2 > self.sdr_callback_length:
                raise ValueError("buffer longer than sdr_callback_length")
            # staged by the library: one device buffer per call in flight, kept until the call is fetched
            self._native.process_host_i8(a)
            return
        if raw.dim() == 1:
            raw = raw[None, :]
        if str(raw.dtype) != "torch.int8" or not raw.is_cuda or raw.dim() != 2 or raw.stride(1) != 1 or raw.shape[1] % 2:
            raise TypeError("device samples must be a CUDA int8 tensor [S, 2*B] with unit stride")
        if raw.shape[0] != len(self.devices) or (raw.shape[0] > 1 and raw.stride(0) % 2):
            raise ValueError("device samples must be int8 [S, 2*B], a whole number of samples from stream to stream")
        if raw.shape[1] // 2 > self.sdr_callback_length:
            raise ValueError("buffer longer than sdr_callback_length")
        self._hold(raw)
        if self._hip_stream is None:
            import torch

            torch.cuda.current_stream(raw.device).synchronize()
        stride = (raw.stride(0) if raw.shape[0] > 1 else raw.shape[1]) // 2
        self._process_device(raw.data_ptr(), raw.shape[1] // 2, stride, 2, False, False, True)

    def fetch_records(self, allow_truncated: bool = False) -> np.ndarray:
        """Wait for the oldest enqueued call; structured array of ``rt_record`` ordered by stream.  The reference
        has no limit on signals per buffer, and neither has an analysed buffer here (a stream that outgrows
        ``record_capacity`` grows it; the call is analysed again inside the fetch).  Only ``extract_signals`` on a caller's
        spectrogram can be cut off: that raises unless ``allow_truncated`` (then ``native.last_truncated`` tells)."""
        return self._native.fetch(allow_truncated)

    def fetch_record_cells(self):
        """``(offsets, cells)``: the spectrogram cells behind every record of the call :meth:`fetch_records` (or
        :meth:`process_batch`) returned last -- all records, shadowed ones included, in the order they were returned.
        ``cells[offsets[i]:offsets[i + 1]]`` (float32, float64 with ``precision="float64"``) is the reference's ``data`` of
        record ``i`` (analyze.py:437-440): bin ``fi`` at segments ``start .. end - 1``, negative segments from the end of the
        stream's previous buffer; linear power, uncalibrated, bit for bit what the detection used (``max(data) == max_p``).
        Needs ``record_cells=True``; raises ``NativeError`` (``RT_E_INVALID``) once another buffer was enqueued or the analyzer
        reset, after an ``extract_signals`` call and after a truncated fetch."""
        return self._native.fetch_record_cells()

    def fetch_record_iq(self, convert: bool = False):
        """``(offsets, first_segment, samples)``: the IQ samples behind every record of the call :meth:`fetch_records` (or
        :meth:`process_batch`) returned last -- all records, shadowed ones included, in the order they were returned.
        ``samples[offsets[i]:offsets[i + 1]]`` are the whole segments ``first_segment[i] ... min(end + margin, T) - 1`` of record
        ``i``'s stream, ``first_segment[i] = max(start - margin, -D)``: a negative segment counts back from the last whole
        segment of the buffer the detection looked back into, of which the analyzer holds ``D = min(T_before, K + margin)``
        segments (``D = 0`` on a first buffer, after a reset or changed settings, and when that buffer came in another format).
        ``samples`` is in the format the buffer was fed in, bit for bit the caller's bytes: complex64 (complex128 with
        ``precision="float64"``), or ``[n, 2]`` uint8 / int8 / int16 (I, Q).  ``convert=True``: complex64 (complex128) through the
        conversions of :mod:`pyradiotracking_amd.synth`, the ones the kernels apply.
        Needs ``record_iq=True``; raises ``NativeError`` (``RT_E_INVALID``) once another buffer was enqueued or the analyzer
        reset, after an ``extract_signals`` call and after a truncated fetch."""
        from . import synth

        offsets, first, payload, bps = self._native.fetch_record_iq()
        fed = self._native.fetched_format
        f64 = self.precision == "float64"
        if fed == "c":
            samples = payload.view(np.complex128 if f64 else np.complex64)
        else:
            samples = payload.view({"u8": np.uint8, "i8": np.int8, "i16": np.int16}[fed]).reshape(-1, 2)
            if convert:
                flat = samples.reshape(-1)
                samples = {"u8": synth.u8_to_complex128_like_pyrtlsdr if f64 else synth.u8_to_complex64_like_kernel,
                           "i8": synth.i8_to_complex128 if f64 else synth.i8_to_complex64,
                           "i16": synth.i16_to_complex128 if f64 else synth.i16_to_complex64}[fed](flat)
        assert len(samples) == offsets[-1]
        return offsets, first, samples

    def fetch_record_stft(self, hop_div: int = 1):
        """``(offsets, first_segment, values)``: one complex STFT value per delivered segment of every record of the call
        :meth:`fetch_records` (or :meth:`process_batch`) returned last -- the value of the RECORD'S bin, complex64 (complex128 with
        ``precision="float64"``).  ``values[offsets[i]:offsets[i + 1]]`` belong to the whole segments ``first_segment[i] ...`` that
        :meth:`fetch_record_iq` delivers for record ``i`` (margin included), so ``offsets`` is that method's divided by
        ``fft_nperseg``.  A value is ``scipy.signal.spectrogram(..., noverlap=0, return_onesided=False, mode='complex')`` at that
        bin and segment: ``sqrt(scale) * sum w[n] (x[n] - mean(x)) exp(-2 pi i fi n / N)``; ``abs(value) ** 2`` is the cell
        :meth:`fetch_record_cells` returns, the phase is what the detection drops.  Computed on the device from the gathered
        snippets, at the first call after a fetch; ``fft_nperseg`` times fewer bytes than the samples.
        Needs ``record_iq=True``; valid exactly as long as :meth:`fetch_record_iq` is.

        ``hop_div`` k > 1 (``rt_fetch_record_stft_hop``; 2 ... 16, a divisor of ``fft_nperseg``): the same value for FRAMES every
        ``fft_nperseg / k`` samples, ``offsets`` counting frames.  The delivered segments below 0 (the predecessor part) and those
        from 0 on (the record's own part) are framed separately -- a part of ``L`` segments has ``(L - 1) k + 1`` frames, none
        straddles the two -- and :func:`stft_frame_positions` gives every frame's first sample.  Every k-th frame of a part is a
        delivered segment, with the bytes the default returns for it; the phase reference is the frame's own start."""
        return self._native.fetch_record_stft(hop_div)

    def fetch_record_band(self, hop_div: int = 1, half_width: int = 2):
        """``(offsets, first_segment, values)``: for every frame of ``fetch_record_stft(hop_div)`` the complex STFT values of the
        ``2 * half_width + 1`` bins around the record's bin (``rt_fetch_record_band``) -- ``values`` is ``[n_frames, 2 w + 1]``,
        complex64 (complex128 with ``precision="float64"``), column ``j`` the bin ``(fi + j - w) mod fft_nperseg``
        (:func:`band_bins`; circular, fftfreq order).  ``offsets`` and ``first_segment`` are that method's, column ``w`` its
        bytes; every column is that method's value at the column's bin, operation for operation, so a record ``d`` bins away in
        the same stream holds this record's column ``w + d`` in its own centre column.  ``half_width`` 0 ... 8, ``hop_div``
        1 ... 16, a divisor of ``fft_nperseg``.  :func:`record_band_spectrum` reduces the frames to the pulse's spectrum.
        Needs ``record_iq=True``; valid exactly as long as :meth:`fetch_record_iq` is."""
        return self._native.fetch_record_band(hop_div, half_width)

    def fetch_record_spectrum(self, hop_div: int = 4, half_width: int = 2):
        """``(rows, mean, peak)``: the band of ``fetch_record_band(hop_div, half_width)`` reduced on the device to one
        ``SPECTRUM_DTYPE`` row per record of the call returned last (``rt_fetch_record_spectrum``) -- the frames themselves are
        not copied to the host.  ``mean`` and ``peak`` are float64 ``[n_records, 2 w + 1]``: per column the mean and the largest
        ``|value| ** 2`` over the ``n_inside`` frames wholly inside the record's own cells; ``rows`` holds ``total``,
        ``centre_share``, ``centroid``, ``width``, ``peak_bins`` (bins off the record's bin; :func:`spectrum_hz` scales them to
        Hz) and ``peak_col``.  :func:`record_band_rows` defines the result; the same frames give the same bytes on every handle
        kind.  Needs ``record_iq=True``; valid exactly as long as :meth:`fetch_record_iq` is."""
        return self._native.fetch_record_spectrum(hop_div, half_width)

    def fetch_record_edges(self, hop_div: int = 4) -> np.ndarray:
        """float64 ``[n_records, 2]``: ``(rise, fall)`` of every record's pulse in samples relative to sample 0 of the buffer of
        the call returned last, to a fraction of ``fft_nperseg / hop_div`` where the pulse is switched and the delivered margin
        holds the edge (``record_iq_margin >= 1``); NaN otherwise (:func:`record_edges`).  Needs ``record_iq=True``."""
        offsets, first, values = self._native.fetch_record_stft(hop_div)
        rec = self._native._last_fetched
        return record_edges(offsets, first, values, rec["start"], rec["end"], self.fft_nperseg, hop_div)

    def fetch_record_estimates(self, hop_div: int = 4) -> np.ndarray:
        """One ``ESTIMATES_DTYPE`` row per record of the call returned last, reduced on the device from the frames of
        ``fetch_record_stft(hop_div)`` (``rt_fetch_record_estimates``) -- the frames themselves are not copied to the host:
        ``offset_hz``, ``coherence``, ``n_pairs`` as :func:`record_fine` gives them for ``hop_div``, ``rise`` and ``fall`` as
        :func:`record_edges` does, ``level`` (the median of ``|c|`` over the ``n_inside`` frames wholly inside the record's own
        cells, whose half the edges are read at), and the raw sums ``r`` (turned back by the bin's own rotation) and ``pair_mag``
        (``coherence = |r| / pair_mag``).  The two host functions define the result; the rows are float64 on every handle kind and
        the same frames give the same bytes.  ``hop_div`` 1 ... 16, a divisor of ``fft_nperseg``; 1: the frames are the segments.
        Needs ``record_iq=True``; valid exactly as long as :meth:`fetch_record_iq` is."""
        rows = self._native.fetch_record_estimates(hop_div)
        out = np.zeros(len(rows), dtype=ESTIMATES_DTYPE)
        out["offset_hz"] = rows["offset_bins"] * float(self.sample_rate) / int(self.fft_nperseg)
        for name in ("coherence", "n_pairs", "level", "rise", "fall", "n_inside", "pair_mag"):
            out[name] = rows[name]
        out["r"].real = rows["r_re"]  # (the parts as they are: 1j * r_im would turn an infinite r_im into a NaN real part)
        out["r"].imag = rows["r_im"]
        return out

    def fetch_record_fine(self, hop_div: int = 1) -> np.ndarray:
        """One row per record of the call returned last (``FINE_DTYPE``: ``offset_hz``, ``coherence``, ``n_pairs``): the
        pulse-pair estimate of the tone's offset from its bin centre, from the values of the record's own cells (``[start, end)``
        clipped to what was delivered; :func:`record_fine`).  ``frequency + offset_hz`` refines a signal's frequency;
        ``coherence`` is 1 for a pure tone and falls with noise or modulation.  The estimate is unambiguous within half a bin
        either side (``|offset_hz| <= sample_rate / (2 fft_nperseg)``): a tone further off shows in the neighbouring bin's record
        too, so it is meaningful for the record the shadow filter keeps, the one whose bin the tone is nearest to.  The pair
        across a buffer boundary (segments -1 and 0) is left out; a record with fewer than two usable cells has NaN.
        ``hop_div`` k > 1: from the frames of ``fetch_record_stft(hop_div=k)``, unambiguous within ``k / 2`` bins either side.
        Needs ``record_iq=True``."""
        offsets, first, values = self._native.fetch_record_stft(hop_div)
        rec = self._native._last_fetched
        return record_fine(offsets, first, values, rec["start"], rec["end"], self.sample_rate, self.fft_nperseg, hop_div, rec["fi"])

    def set_input_stats(self, on: bool) -> None:
        """Turn the per-stream input statistics on or off (``rt_set_input_stats``) between calls: ``NativeError``
        (``RT_E_INVALID``) while enqueued buffers are unfetched.  A buffer enqueued while they were off has none."""
        self._native.set_input_stats(bool(on))
        self.input_stats = bool(on)

    def fetch_input_stats(self) -> np.ndarray:
        """``[S]`` rows of ``_native.INPUT_STATS_DTYPE`` for the buffer of the call :meth:`fetch_records` (or
        :meth:`process_batch`) returned last, computed on the device from ALL its samples when it was enqueued: ``n_samples``,
        ``n_rail`` (components at full scale), ``n_nonfinite``, the sums ``sum_i``, ``sum_q``, ``sum_sq`` of the raw components
        and their squares, ``peak``, and the ``format`` / ``unit`` that turn raw into values (:func:`input_levels` does).  Exact
        for the integer formats; for complex input the same samples give the same bytes however they are laid out or split into
        lanes.  A stream that sat the call out (:meth:`set_present`) has ``n_samples == 0``.  Needs ``input_stats=True``; raises
        ``NativeError`` (``RT_E_INVALID``) once another buffer was enqueued or the analyzer reset, and after ``extract_signals``."""
        return self._native.fetch_input_stats()

    def fetch_row_means(self, dbw: bool = False) -> np.ndarray:
        """``[S, fft_nperseg]`` (float32, float64 with ``precision="float64"``): every bin's row mean -- ``freq_avg``, the
        reference's noise figure (analyze.py:373-375) -- over the buffer of the call :meth:`fetch_records` (or
        :meth:`process_batch`) returned last, bins in fftfreq order; NaN for a buffer shorter than ``fft_nperseg`` and for the rows
        of a stream that sat the call out (:meth:`set_present`).  A record's
        ``row_mean`` equals its bin's entry bit for bit.  ``dbw=True``: in dBW as ``Signal.noise`` (uncalibrated, analyze.py:446).
        Needs ``row_means=True``; raises ``NativeError`` (``RT_E_INVALID``) once another buffer was enqueued or the analyzer
        reset, and after an ``extract_signals`` call."""
        out = self._native.fetch_row_means()
        return self._decoder.noise_dbw(out) if dbw else out

    def process_batch(self, iq, ts_starts: Union[datetime.datetime, Sequence[datetime.datetime]], filtered: bool = True, lazy: bool = True,
                      links: Optional[int] = None):
        """One buffer per stream -> per stream a sequence of ``Signal``.

        ``filtered=True`` returns what the reference puts on its queue
        (after ``filter_shadow_signals``); ``False`` returns the list
        ``extract_signals`` would have produced.

        ``lazy`` (default): every stream's sequence is a :class:`SignalBatch` -- the nine field columns of the whole call are built
        at once, a ``Signal`` object only when an element is asked for (it compares equal to the list of those objects; 2.6 x the
        rate of building every object up front, and a consumer that hands columns on -- CSV rows, the matcher -- never needs
        them).  ``lazy=False``: plain lists of ``Signal`` objects.

        With ``chain=L``: ``iq`` is ``[R, l * B]`` and ``ts_starts`` holds one time per recording, the start of its first
        buffer of this call; the result is per RECORDING, the signals of its ``l`` buffers in time order -- what ``l``
        consecutive ``SignalAnalyzer.process_samples`` callbacks put on the queue.  Buffer ``j`` starts at ``ts_start + j *
        timedelta(seconds=B / sample_rate)``: the reference's running clock adds that ``timedelta`` once per callback
        (analyze.py:205, 221, 231), and ``timedelta`` arithmetic is exact."""
        self.enqueue(iq, links=links)
        rec = self.fetch_records()
        if self.chain:
            return self._chained_signals(rec, ts_starts, filtered, lazy)
        if isinstance(ts_starts, datetime.datetime):
            ts_starts = [ts_starts] * len(self.devices)
        if filtered:
            rec = rec[rec["shadowed"] == 0]
        # (records come ordered by stream: a stream's signals are one slice)
        bounds = np.searchsorted(rec["stream"], np.arange(len(self.devices) + 1))
        if lazy:
            batch = self._decoder.signal_batch(rec, self.devices, ts_starts)
            return [batch[int(bounds[s]):int(bounds[s + 1])] for s in range(len(self.devices))]
        sigs = self._decoder.signals(rec, self.devices, ts_starts)
        return [sigs[int(bounds[s]):int(bounds[s + 1])] for s in range(len(self.devices))]


    def _chained_signals(self, rec, ts_starts, filtered: bool, lazy: bool):
        """``process_batch`` of a chained analyzer: the fetched records -> per recording its signals, links in time order."""
        L, R = self.chain, len(self.run_devices)
        if isinstance(ts_starts, datetime.datetime):
            ts_starts = [ts_starts] * R
        if len(ts_starts) != R:
            raise ValueError(f"expected {R} start times: one per recording")
        l, n = self._chain_call
        step = datetime.timedelta(seconds=(n or 0) / self.sample_rate)  # analyze.py:205
        ts_streams = [ts_starts[r] + j * step for r in range(R) for j in range(L)]  # :221, :231
        if filtered:
            rec = rec[rec["shadowed"] == 0]
        # (records come ordered by stream, i.e. by recording and inside it by link: a recording's signals are one slice)
        bounds = np.searchsorted(rec["stream"], np.arange(R + 1) * L)
        sigs = self._decoder.signal_batch(rec, self.devices, ts_streams) if lazy else self._decoder.signals(rec, self.devices, ts_streams)
        return [sigs[int(bounds[r]):int(bounds[r + 1])] for r in range(R)]


class SignalAnalyzer:
    """Drop-in for ``radiotracking.analyze.SignalAnalyzer`` on the analysis path.

    Constructor keywords are the reference's (analyze.py:62-83; unknown ones are
    swallowed like its ``**kwargs``) plus ``gpu`` (HIP device ordinal).  The
    object is *not* a ``multiprocessing.Process`` and opens no SDR: feed it
    buffers through :meth:`process_samples` exactly as ``read_samples_async``
    would (analyze.py:157).
    """

    def __init__(
        self,
        device: str,
        calibration_db: float = 0.0,
        sample_rate: int = 300000,
        center_freq: int = 150150000,
        gain: float = 49.6,
        fft_nperseg: int = 256,
        fft_window="hamming",
        signal_min_duration_ms: float = 8,
        signal_max_duration_ms: float = 40,
        signal_threshold_dbw: float = -90.0,
        snr_threshold_db: float = 5.0,
        verbose: int = 0,
        sdr_max_restart: int = 3,
        sdr_timeout_s: int = 2,
        state_update_s: int = 60,
        sdr_callback_length: Optional[int] = None,
        signal_queue=None,
        last_data_ts=None,
        gpu: int = 0,
        mode: str = "auto",
        precision: str = "float32",
        row_means: bool = False,
        record_cells: bool = False,
        f64_sparse: bool = False,
        f64_rescue: bool = False,
        record_iq: bool = False,
        record_iq_margin: int = 0,
        stft_hop_div: int = 1,
        record_estimates: bool = False,
        input_stats: bool = False,
        record_band: Optional[int] = None,
        record_spectrum: bool = False,
        **kwargs,
    ):
        """``input_stats=True``: after every buffer ``input_stats`` holds the row of
        :meth:`BatchSignalAnalyzer.fetch_input_stats` for the buffer just analysed (:func:`input_levels` turns it into levels).

        ``record_iq=True``: after every buffer ``signal_iq`` is the list of the sample arrays of the signals put on the queue
        (unshadowed, queue order, like ``signal_data``) -- the IQ of each pulse in the format the buffer came in, with
        ``record_iq_margin`` whole segments on either side (:meth:`BatchSignalAnalyzer.fetch_record_iq`), and ``signal_stft`` the
        list of their complex STFT values: one per delivered segment, or with ``stft_hop_div=k`` one per frame every
        ``fft_nperseg / k`` samples (:meth:`BatchSignalAnalyzer.fetch_record_stft`).  ``record_estimates=True`` with it:
        ``signal_estimates`` holds one row per such signal (:meth:`BatchSignalAnalyzer.fetch_record_estimates` at ``stft_hop_div``).
        ``record_band=w`` with it: ``signal_band`` is the list of their ``[n_frames, 2 w + 1]`` arrays, the bins beside each
        signal's bin at ``stft_hop_div`` (:meth:`BatchSignalAnalyzer.fetch_record_band`).  ``record_spectrum=True`` with
        ``record_band=w``: ``signal_spectrum`` is ``(rows, mean, peak)`` of those signals, the band reduced on the device
        (:meth:`BatchSignalAnalyzer.fetch_record_spectrum`).

        ``record_cells=True``: after every buffer ``signal_data`` is the list of the cell arrays of the signals put on the
        queue (unshadowed, queue order) -- the reference's ``data`` of each ``Signal`` (analyze.py:437-440): linear power.

        ``precision="float64"``: complex128 buffers are analysed in float64 as the reference does (BatchSignalAnalyzer);
        ``f64_sparse=True`` with it: on the map-free float64 path (same ``Signal``s); ``f64_rescue=True`` with that: a buffer
        that overflows the candidate lists is analysed again from a float64 map instead of raising ``RT_E_HOT_OVERFLOW``.
        ``row_means=True``: after every buffer ``noise_dbw`` holds the noise level of every bin (``[fft_nperseg]``, dBW, fftfreq
        order) -- what the reference prints as the ``noise`` of a Signal (analyze.py:446), for all bins."""
        self.device = device
        self.precision = precision
        self.row_means = bool(row_means)
        self.noise_dbw: Optional[np.ndarray] = None
        self.record_cells = bool(record_cells)
        self.signal_data: Optional[List[np.ndarray]] = None
        self.record_iq = bool(record_iq)
        self.record_iq_margin = int(record_iq_margin)
        self.signal_iq: Optional[List[np.ndarray]] = None
        self.signal_stft: Optional[List[np.ndarray]] = None  # (beside signal_iq: the complex STFT values of each signal's bin)
        self.stft_hop_div = int(stft_hop_div)
        if record_estimates and not record_iq:
            raise ValueError("record_estimates needs record_iq=True")
        self.record_estimates = bool(record_estimates)
        self.signal_estimates: Optional[np.ndarray] = None  # (beside signal_stft: one ESTIMATES_DTYPE row per signal)
        if record_band is not None and not record_iq:
            raise ValueError("record_band needs record_iq=True")
        self.record_band = None if record_band is None else int(record_band)
        self.signal_band: Optional[List[np.ndarray]] = None  # (beside signal_stft: the bins around each signal's bin, frame by frame)
        if record_spectrum and record_band is None:
            raise ValueError("record_spectrum needs record_iq=True and record_band=w")
        self.record_spectrum = bool(record_spectrum)
        self.signal_spectrum = None  # (beside signal_band: (rows, mean, peak), one row per signal)
        self._input_stats_on = bool(input_stats)
        self.input_stats: Optional[np.void] = None  # (the buffer's own level, DC and clipping: one INPUT_STATS_DTYPE row)
        self.calibration_db = calibration_db
        try:
            self.device_index = int(device)  # analyze.py:89-91
        except ValueError:
            self.device_index = None  # serial-number lookup needs pyrtlsdr: out of scope
        self.sample_rate = sample_rate
        self.center_freq = center_freq
        try:
            self.gain = float(gain)
        except ValueError:
            self.gain = gain
        if sdr_callback_length is None:
            sdr_callback_length = sample_rate
        self.fft_nperseg = fft_nperseg
        self.fft_window = fft_window
        self.signal_min_duration = signal_min_duration_ms / 1000
        self.signal_max_duration = signal_max_duration_ms / 1000
        self.signal_threshold = from_dB(signal_threshold_dbw + calibration_db)
        self.snr_threshold = from_dB(snr_threshold_db)
        self.sdr_callback_length = sdr_callback_length
        self.verbose = verbose
        self.sdr_max_restart = sdr_max_restart
        self.sdr_timeout_s = sdr_timeout_s
        self.state_update_s = state_update_s
        self.signal_queue = signal_queue
        # the reference always gets a multiprocessing.Value("d") from its Runner (__main__.py:118); without one the
        # heartbeat lives in a private holder, so that the first buffer reports STARTED and the later ones RUNNING
        self.last_data_ts = last_data_ts if last_data_ts is not None else _Heartbeat()
        self.last_state: Optional[StateMessage] = None
        self.sdr = None  # the caller's SDR handle, if it wants cancel_read_async() on a fatal clock drift

        self._spectrogram_last = None  # only used by extract_signals() called directly
        self._ts = None
        self._replay_batch = None  # (replay: a chained analyzer of its own, made at first use)
        self._replay_kw = dict(
            calibration_db=calibration_db, sample_rate=sample_rate, center_freq=center_freq, fft_nperseg=fft_nperseg, fft_window=fft_window,
            signal_min_duration_ms=signal_min_duration_ms, signal_max_duration_ms=signal_max_duration_ms, signal_threshold_dbw=signal_threshold_dbw,
            snr_threshold_db=snr_threshold_db, sdr_callback_length=sdr_callback_length, gpu=gpu, mode=mode,
            **{k: kwargs[k] for k in ("record_capacity", "record_pool", "hot_capacity", "group_detect") if k in kwargs},
        )
        self._batch = BatchSignalAnalyzer(
            [device],
            calibration_db=calibration_db,
            sample_rate=sample_rate,
            center_freq=center_freq,
            fft_nperseg=fft_nperseg,
            fft_window=fft_window,
            signal_min_duration_ms=signal_min_duration_ms,
            signal_max_duration_ms=signal_max_duration_ms,
            signal_threshold_dbw=signal_threshold_dbw,
            snr_threshold_db=snr_threshold_db,
            sdr_callback_length=sdr_callback_length,
            gpu=gpu,
            mode=mode,
            precision=precision,
            row_means=self.row_means,
            record_cells=self.record_cells,
            record_iq=self.record_iq,
            record_iq_margin=self.record_iq_margin,
            input_stats=self._input_stats_on,
            f64_sparse=bool(f64_sparse),
            f64_rescue=bool(f64_rescue),
            # capacities of the native handle (no counterpart in the reference, whose lists are unbounded)
            **{k: kwargs[k] for k in ("record_capacity", "record_pool", "hot_capacity", "group_detect") if k in kwargs},
        )
        self._decoder = self._batch._decoder

    # -- the callback (analyze.py:192-268) -----------------------------------
    def update_state(self, ts: datetime.datetime, state: "StateMessage.State") -> None:
        """Put a ``StateMessage`` on the queue unless the same state was reported less than
        ``state_update_s`` seconds ago (analyze.py:180-190)."""
        ts = ts.astimezone(pytz.utc)
        last = self.last_state
        if last and last.state == state and last.ts + datetime.timedelta(seconds=self.state_update_s) >= ts:
            return
        self.last_state = StateMessage(self.device, ts, state)
        if self.signal_queue is not None:
            self.signal_queue.put(self.last_state)

    def _clock(self, n_samples: int):
        """Book-keeping at the head of the callback (analyze.py:204-231): liveness, heartbeat value,
        running clock, drift check.  Returns ``ts_start`` of the buffer."""
        ts_recv = datetime.datetime.now()
        buffer_len_dt = datetime.timedelta(seconds=n_samples / self.sample_rate)  # :205
        if not self.last_data_ts.value:  # :210-213
            self.update_state(datetime.datetime.now(), StateMessage.State.STARTED)
        else:
            self.update_state(ts_recv, StateMessage.State.RUNNING)
        self.last_data_ts.value = datetime.datetime.timestamp(ts_recv)  # :214
        if not self._ts:  # :218-221
            self._ts = ts_recv
        else:
            self._ts += buffer_len_dt
        clock_drift = (ts_recv - self._ts).total_seconds()
        if clock_drift > 2 * buffer_len_dt.total_seconds():  # :226-229
            logger.warning(
                f"SDR {self.device} total clock drift ({clock_drift:.5f} s) is larger than two blocks, "
                "signal detection is degraded. Terminating..."
            )
            self.update_state(datetime.datetime.now(), StateMessage.State.STOPPED)
            if self.sdr is not None:
                self.sdr.cancel_read_async()
        return self._ts - buffer_len_dt  # :231

    def process_samples(self, buffer: np.ndarray, context=None):
        """Analyse one buffer; state messages and detected signals go to ``signal_queue`` in the
        reference's order.  complex128 buffers (what pyrtlsdr delivers) are analysed in complex64 --
        unless the analyzer was made with ``precision="float64"``, which analyses them in float64 as the reference
        does.  The SIGALRM watchdog of the reference
        (analyze.py:208) belongs to the process that owns the SDR and is not re-armed here."""
        ts_start = self._clock(len(buffer))
        filtered = self.analyze_buffer(buffer, ts_start)
        [self.consume_signal(s) for s in filtered]  # :251
        return None

    def process_bytes(self, raw: np.ndarray, context=None):
        """The callback for ``RtlSdr.read_bytes_async``: ``raw`` is the interleaved uint8 I/Q
        buffer (2 bytes per sample).  Same bookkeeping and queue contract as
        :meth:`process_samples`; the conversion pyrtlsdr would do on the host happens in the
        scan kernel's load."""
        raw = np.ascontiguousarray(raw, dtype=np.uint8)
        n = raw.size // 2
        ts_start = self._clock(n)
        if n > self._batch.sdr_callback_length:
            raise ValueError("buffer longer than sdr_callback_length")
        self.noise_dbw = self.signal_data = self.signal_iq = self.signal_stft = self.signal_estimates = self.input_stats = None
        self._batch.enqueue_bytes(raw.reshape(1, -1))
        rec = self._batch.fetch_records()
        self._keep_noise()
        self._keep_cells(rec["shadowed"] == 0)
        rec = rec[rec["shadowed"] == 0]
        [self.consume_signal(s) for s in self._decoder.signals(rec, [self.device], [ts_start])]
        return None

    def process_int16(self, raw: np.ndarray, context=None):
        """The callback for a 16-bit source (SoapySDR ``CS16``, UHD ``sc16``, a ``ci16_le`` recording): ``raw`` is the interleaved
        int16 I/Q buffer (4 bytes per sample, value ``i * 2**-15``).  Same bookkeeping and queue contract as
        :meth:`process_samples`, and the signals of ``process_samples(synth.i16_to_complex64(raw))``; the conversion happens
        in the scan kernel's load."""
        raw = np.asarray(raw)
        if raw.dtype != np.int16:
            raise TypeError("expected an int16 array (interleaved I, Q)")
        raw = np.ascontiguousarray(raw).reshape(-1)
        if raw.size % 2:
            raise ValueError("expected int16 [2*B]: an I and a Q for every sample")
        n = raw.size // 2
        if n > self._batch.sdr_callback_length:
            raise ValueError("buffer longer than sdr_callback_length")
        ts_start = self._clock(n)
        self.noise_dbw = self.signal_data = self.signal_iq = self.signal_stft = self.signal_estimates = self.input_stats = None
        self._batch.enqueue_int16(raw.reshape(1, -1))
        rec = self._batch.fetch_records()
        self._keep_noise()
        self._keep_cells(rec["shadowed"] == 0)
        rec = rec[rec["shadowed"] == 0]
        [self.consume_signal(s) for s in self._decoder.signals(rec, [self.device], [ts_start])]
        return None

    def process_int8(self, raw: np.ndarray, context=None):
        """The callback for an 8-bit signed source (a HackRF, SoapySDR ``CS8``, UHD ``sc8``, a ``ci8`` recording): ``raw`` is the interleaved
        int8 I/Q buffer (2 bytes per sample, value ``i * 2**-7``).  Same bookkeeping and queue contract as
        :meth:`process_samples`, and the signals of ``process_samples(synth.i8_to_complex64(raw))``; the conversion happens
        in the scan kernel's load."""
        raw = np.asarray(raw)
        if raw.dtype != np.int8:
            raise TypeError("expected an int8 array (interleaved I, Q)")
        raw = np.ascontiguousarray(raw).reshape(-1)
        if raw.size % 2:
            raise ValueError("expected int8 [2*B]: an I and a Q for every sample")
        n = raw.size // 2
        if n > self._batch.sdr_callback_length:
            raise ValueError("buffer longer than sdr_callback_length")
        ts_start = self._clock(n)
        self.noise_dbw = self.signal_data = self.signal_iq = self.signal_stft = self.signal_estimates = self.input_stats = None
        self._batch.enqueue_int8(raw.reshape(1, -1))
        rec = self._batch.fetch_records()
        self._keep_noise()
        self._keep_cells(rec["shadowed"] == 0)
        rec = rec[rec["shadowed"] == 0]
        [self.consume_signal(s) for s in self._decoder.signals(rec, [self.device], [ts_start])]
        return None

    def analyze_buffer(self, buffer: np.ndarray, ts_start: datetime.datetime, filtered: bool = True) -> List[Signal]:
        """analyze.py:234-248 and :268 with an explicit ``ts_start``."""
        bench_start = time.time()
        buf = np.ascontiguousarray(buffer, dtype=np.complex128 if self.precision == "float64" else np.complex64).reshape(1, -1)
        if buf.shape[1] > self._batch.sdr_callback_length:
            raise ValueError("buffer longer than sdr_callback_length")
        self.noise_dbw = self.signal_data = self.signal_iq = self.signal_stft = self.signal_estimates = self.input_stats = None
        if self.record_cells or self.record_iq:  # (process_batch, with the records kept for the cells' shadow flags)
            self._batch.enqueue(buf)
            rec = self._batch.fetch_records()
            keep = rec["shadowed"] == 0 if filtered else np.ones(len(rec), dtype=bool)
            out = self._decoder.signals(rec[keep], [self.device], [ts_start])
            self._keep_cells(keep)
        else:
            out = self._batch.process_batch(buf, [ts_start], filtered=filtered, lazy=False)[0]  # (one stream: its Signal objects, as the reference returns them)
        self._keep_noise()
        logger.info(
            f"SDR {self.device} recv {len(buffer)}, {len(out)} signals, "
            f"compute: {(time.time() - bench_start) * 1000:.1f} ms"
        )
        return out

    def replay(self, samples: np.ndarray, ts_start: datetime.datetime, *, chain: int = 16, fmt: str = "c64", record_iq: bool = False,
               record_stft: bool = False, stft_hop_div: int = 1, record_estimates: bool = False, record_band: Optional[int] = None,
               record_spectrum: bool = False):
        """Run one long RECORDING through the analysis, ``chain`` buffers of ``sdr_callback_length`` per call (``rt_set_chain``)
        instead of one: the signals -- returned, and put on ``signal_queue`` -- are those of calling the matching callback
        (``process_samples`` / ``process_bytes`` / ``process_int16`` / ``process_int8`` for ``fmt`` ``"c64"`` / ``"u8"`` /
        ``"i16"`` / ``"i8"``) on a fresh analyzer once per buffer, in that order, with a clock that starts at ``ts_start``.
        ``samples``: one array, complex for ``"c64"``, else interleaved I, Q.  The last call has fewer links; a remainder
        shorter than a buffer is one more call if it holds at least two segments, else it is dropped with a log line (nothing
        could be detected in it).  Every replay starts without look-back; the analyzer's own callback state is left alone.
        ``record_iq=True``: returns ``(signals, signal_iq)`` -- beside every signal its samples, as the per-buffer callbacks of an
        analyzer made with ``record_iq=True`` (and this analyzer's ``record_iq_margin``) leave them in ``signal_iq``.
        ``record_stft=True`` (with ``record_iq=True``): returns ``(signals, signal_iq, signal_stft)``, the complex STFT values of
        each signal's bin as well (:meth:`BatchSignalAnalyzer.fetch_record_stft`), with ``stft_hop_div=k`` at frames every
        ``fft_nperseg / k`` samples.  ``record_estimates=True`` (with ``record_iq=True``): one more list at the end of the tuple,
        a row of :meth:`BatchSignalAnalyzer.fetch_record_estimates` (at ``stft_hop_div``) per signal.  ``record_band=w`` (with
        ``record_iq=True``): one more list behind those, per signal the ``[n_frames, 2 w + 1]`` array of
        :meth:`BatchSignalAnalyzer.fetch_record_band` (at ``stft_hop_div``).  ``record_spectrum=True`` (with ``record_band=w``):
        one more list at the very end, per signal the ``SPECTRUM_DTYPE`` row of
        :meth:`BatchSignalAnalyzer.fetch_record_spectrum` (at ``stft_hop_div`` and ``w``)."""
        if record_band is not None and not record_iq:
            raise ValueError("record_band needs record_iq=True")
        if record_spectrum and record_band is None:
            raise ValueError("record_spectrum needs record_iq=True and record_band=w")
        if record_stft and not record_iq:
            raise ValueError("record_stft needs record_iq=True")
        if record_estimates and not record_iq:
            raise ValueError("record_estimates needs record_iq=True")
        per_sample = {"c64": 1, "u8": 2, "i16": 2, "i8": 2}[fmt]
        want = {"c64": np.complex64, "u8": np.uint8, "i16": np.int16, "i8": np.int8}[fmt]
        x = np.asarray(samples).reshape(-1)
        if fmt == "c64":
            x = np.ascontiguousarray(x, dtype=np.complex64)
        elif x.dtype != want or x.size % 2:
            raise TypeError(f"fmt {fmt!r} takes an interleaved {np.dtype(want).name} array [2 * n]")
        if self.precision == "float64":
            raise ValueError("replay is not available with precision='float64'")
        if int(chain) < 2:
            raise ValueError("chain must be >= 2")
        if self._replay_batch is None or self._replay_batch.chain != int(chain) or self._replay_batch.record_iq != bool(record_iq):
            if self._replay_batch is not None:
                self._replay_batch.close()
            self._replay_batch = BatchSignalAnalyzer([self.device], chain=int(chain), record_iq=bool(record_iq), record_iq_margin=self.record_iq_margin,
                                                     **self._replay_kw)
        batch = self._replay_batch
        batch.reset()
        enqueue = {"c64": batch.enqueue, "u8": batch.enqueue_bytes, "i16": batch.enqueue_int16, "i8": batch.enqueue_int8}[fmt]
        B, L = batch.sdr_callback_length, int(chain)
        n = x.size // per_sample
        n_full, rest = divmod(n, B)
        step = datetime.timedelta(seconds=B / self.sample_rate)  # analyze.py:205
        out: List[Signal] = []
        out_iq: List[np.ndarray] = []
        out_stft: List[np.ndarray] = []
        out_est: List[np.void] = []
        out_band: List[np.ndarray] = []
        out_spec: List[np.void] = []

        def call(first: int, links: int, length: int):
            part = x[first * B * per_sample:(first * B + links * length) * per_sample]
            enqueue(part.reshape(1, -1), links=links)
            rec = batch.fetch_records()
            if record_iq:  # (records come by link, i.e. in time order: the kept ones line up with the signals below)
                offsets, _, got = batch.fetch_record_iq()
                out_iq.extend(got[offsets[i]:offsets[i + 1]] for i in np.flatnonzero(rec["shadowed"] == 0))
            if record_stft:
                offsets, _, got = batch.fetch_record_stft(stft_hop_div)
                out_stft.extend(got[offsets[i]:offsets[i + 1]] for i in np.flatnonzero(rec["shadowed"] == 0))
            if record_estimates:
                out_est.extend(batch.fetch_record_estimates(stft_hop_div)[rec["shadowed"] == 0])
            if record_band is not None:
                offsets, _, got = batch.fetch_record_band(stft_hop_div, record_band)
                out_band.extend(got[offsets[i]:offsets[i + 1]] for i in np.flatnonzero(rec["shadowed"] == 0))
                if record_spectrum:
                    out_spec.extend(batch.fetch_record_spectrum(stft_hop_div, record_band)[0][rec["shadowed"] == 0])
            out.extend(batch._chained_signals(rec, [ts_start + first * step], True, False)[0])

        for first in range(0, n_full, L):
            call(first, min(L, n_full - first), B)
        if rest >= 2 * self.fft_nperseg:
            call(n_full, 1, rest)
        elif rest:
            logger.info(f"SDR {self.device} replay: the last {rest} samples hold fewer than two segments and are dropped")
        [self.consume_signal(s) for s in out]
        got = (out, out_iq) + ((out_stft,) if record_stft else ()) + ((out_est,) if record_estimates else ()) + ((out_band,) if record_band is not None else ())
        got = got + ((out_spec,) if record_spectrum else ())
        return got if record_iq else out

    def _keep_noise(self):
        if self.row_means:
            self.noise_dbw = self._batch.fetch_row_means(dbw=True)[0]
        if self._input_stats_on:
            self.input_stats = self._batch.fetch_input_stats()[0]

    def _keep_cells(self, keep):
        """``signal_data``: the cells of the records ``keep`` selects (those whose signals go to the queue), in their order."""
        if self.record_cells:
            offsets, cells = self._batch.fetch_record_cells()
            self.signal_data = [cells[offsets[i]:offsets[i + 1]] for i in np.flatnonzero(keep)]
        if self.record_iq:
            offsets, _, samples = self._batch.fetch_record_iq()
            self.signal_iq = [samples[offsets[i]:offsets[i + 1]] for i in np.flatnonzero(keep)]
            offsets, _, values = self._batch.fetch_record_stft(self.stft_hop_div)
            self.signal_stft = [values[offsets[i]:offsets[i + 1]] for i in np.flatnonzero(keep)]
            if self.record_estimates:
                self.signal_estimates = self._batch.fetch_record_estimates(self.stft_hop_div)[np.flatnonzero(keep)]
            if self.record_band is not None:
                offsets, _, values = self._batch.fetch_record_band(self.stft_hop_div, self.record_band)
                self.signal_band = [values[offsets[i]:offsets[i + 1]] for i in np.flatnonzero(keep)]
                if self.record_spectrum:
                    self.signal_spectrum = tuple(a[np.flatnonzero(keep)] for a in self._batch.fetch_record_spectrum(self.stft_hop_div, self.record_band))

    def reset(self):
        self._batch.reset()
        self._spectrogram_last = None
        self._ts = None
        if isinstance(self.last_data_ts, _Heartbeat):
            self.last_data_ts.value = 0.0

    # -- the reference's public helpers ---------------------------------------
    def consume_signal(self, signal: Signal):
        """analyze.py:270-280."""
        logger.debug(f"SDR {self.device} received {signal}")
        if self.signal_queue is not None:
            self.signal_queue.put(signal)

    def extract_signals(self, freqs: np.ndarray, times: np.ndarray, spectrogram: np.ndarray, ts_start: datetime.datetime) -> List[Signal]:
        """analyze.py:330-452 on an explicit ``[F, T]`` power spectrogram (any
        ``F``), with ``self._spectrogram_last`` as the previous one.  Runs the
        dense detect kernel (``rt_extract``).  The time axis must be the one
        SciPy produces for ``fft_nperseg`` / ``sample_rate`` (hop = nperseg/fs);
        ``freqs`` is used as given."""
        self.noise_dbw = self.signal_data = self.signal_iq = self.signal_stft = self.signal_estimates = self.input_stats = None  # (the caller holds this map: no row means, no cells of it)
        spec = np.asarray(spectrogram)
        n_bins, n_seg = spec.shape
        if n_seg == 0:
            return []
        if n_seg >= 2:
            hop = self._decoder.times(np.array([1]))[0] - self._decoder.times(np.array([0]))[0]
            if not np.isclose(times[1] - times[0], hop, rtol=1e-9, atol=0.0):
                raise ValueError("times does not match fft_nperseg / sample_rate")
        nat = self._batch.native
        sdt = np.float64 if self.precision == "float64" else np.float32  # (a float64 analyzer: rt_extract_f64)
        seg_major = np.ascontiguousarray(spec.T, dtype=sdt)
        d_spec = _native.DeviceBuffer(self._batch.gpu, max(4, seg_major.nbytes))
        d_spec.upload(seg_major)
        d_last = None
        n_last = 0
        if self._spectrogram_last is not None:
            last = np.ascontiguousarray(np.asarray(self._spectrogram_last).T, dtype=sdt)
            n_last = last.shape[0]
            d_last = _native.DeviceBuffer(self._batch.gpu, max(4, last.nbytes))
            d_last.upload(last)
        try:
            nat.extract_device(d_spec.ptr, n_seg, n_bins, d_last.ptr if d_last else None, n_last)
            rec = nat.fetch()
        finally:
            d_spec.free()
            if d_last:
                d_last.free()
        self._last_records = rec
        t_start, duration_s, frequency, max_dbw, avg_dbw, std_db, noise_dbw, snr_db = self._decoder.decode(rec, freqs)
        out = []
        for i in range(len(rec)):
            ts = ts_start + datetime.timedelta(seconds=float(t_start[i]))
            out.append(
                Signal(
                    self.device,
                    ts.astimezone(pytz.utc),
                    frequency[i],
                    datetime.timedelta(seconds=float(duration_s[i])),
                    max_dbw[i],
                    avg_dbw[i],
                    std_db[i],
                    noise_dbw[i],
                    snr_db[i],
                )
            )
        return out

    @staticmethod
    def is_shadow_of(sig: Signal, signals: List[Signal]) -> Union[None, int]:
        """analyze.py:283-313 on ``Signal`` objects (pure datetime/float
        comparisons on the host).  ``process_samples`` does not use this: its
        verdicts come from the detect kernel (``rt_record.shadowed``)."""
        for i, other in enumerate(signals):
            if sig.ts > other.ts + other.duration:
                continue
            if sig.ts + sig.duration < other.ts:
                continue
            if other.max > sig.max:
                return i
        return None

    def filter_shadow_signals(self, signals: List[Signal]) -> List[Signal]:
        """analyze.py:315-328 for a caller-supplied list (see ``is_shadow_of``)."""
        verdict = [SignalAnalyzer.is_shadow_of(s, signals) for s in signals]
        return [s for s, v in zip(signals, verdict) if v is None]
