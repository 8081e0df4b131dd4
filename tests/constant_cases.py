"""Segments that cancel exactly: the inputs of tests/test_constant_contract.py (CPU) and tests/test_gpu_constant.py (GPU).

A front end that clips for one segment next to a strong tag delivers a segment whose samples are all one value.  The reference
subtracts the segment's mean first (``x - mean`` is exactly zero), so every cell of that segment is ``0.0``; its plateau starts ON the
sub-threshold cell before the run (analyze.py:382-398), so a pulse right behind such a segment gives a record whose head cell is 0,
``dB = -inf`` and ``std = NaN``.  Every case here holds exactly that: S = 3 streams at 2.048 MS/s, noise sigma 0.012, a few
consecutive buffers of 24 .. 40 segments, ``signal_min_duration_ms = 0`` (or a few hops where a pre-filter needs them); in the TARGET
stream one segment is constant and a bin-centred tone of amplitude 0.25 starts in the segment behind it (``TONE_SEGS`` segments
long).  The threshold lies 10 dB under the tone's peak, clipped into -70 .. -50 dBW: the noise (-98 dBW) is far below, the tone's bin
and, under hamming / hann / blackman, its neighbours are above.  Stream 0 is noise only; stream 2 carries an ordinary tone, so
that every buffer set has records with a finite ``std`` as well.

Placements (``Case.placement``)
  a        inside buffer 1, constant segment and pulse in one chunk (``segs_per_chunk`` explicit; ``a_x``: the constant segment is
           the last of its chunk, the pulse in the next one)
  b        the LAST segment of buffers 0 and 2, the pulse from segment 0 of buffers 1 and 3 (the 2nd and the 4th call: the head
           cell comes out of the look-back tail, and the three tails rotate)
  c        the same input over six buffers through a chained handle of three links (rt_set_chain): link 0 -> link 1 of call 0, and
           the last link of call 0 -> the first link of call 1
  d        ragged: buffer 0 ends in half a segment of the constant behind its last whole one -- never analysed; the pulse starts
           buffer 1, its head cell is buffer 0's last WHOLE segment (noise): a finite ``std``
  e_zero, e_rail   controls: the whole target stream constant (zeros / a rail) in every buffer -- no record, row means exactly 0
  e_lone   control: a constant segment with no pulse behind it -- no record there

Formats (``Case.fmt``): ``i16``, ``i8``, ``u8`` wire samples; ``c64`` = the int16 samples converted by synth.i16_to_complex64 and
fed through ``enqueue`` (a radio whose driver already converted); ``c64full`` = complex64 with the full-mantissa constant
``FULL_MANTISSA``, for which NumPy's float32 mean is NOT the constant: the reference itself leaves a residue there and its ``std`` is
finite (tests/test_constant_contract.py shows it); its tone sits in bin 1, where that residue is largest."""
import datetime
import functools
import zlib
from collections import namedtuple

import numpy as np

from oracle import analyze_oracle as oracle
from pyradiotracking_amd import synth

TS0 = datetime.datetime(2024, 1, 1, tzinfo=datetime.timezone.utc)
FS = 2048000
S = 3
TARGET, PLAIN = 1, 2
SIGMA = 0.012
TONE_AMP = 0.25
TONE_SEGS = 3
FULL_MANTISSA = complex(np.float32(0.3), np.float32(-0.7))
MARGIN_REL = 2e-4  # tests/test_combo_contract.py, tests/sequence_cases.py: no cell within 2e-4 (relative) of a threshold on the float32 paths

Case = namedtuple("Case", "name nperseg window fmt placement const T spc mode extra precision min_hops",
                  defaults=("sparse", (), "float32", 0.0))


def _c(name, nperseg, window, fmt, placement, const, T=32, spc=8, mode="sparse", precision="float32", min_hops=0.0, **extra):
    return Case(name, nperseg, window, fmt, placement, const, T, spc, mode, tuple(sorted(extra.items())), precision, min_hops)


# Rescue cases (RT_FLAG_F64_RESCUE): CARRIERS bin-centred tones of amplitude CARRIER_AMP through every segment of the target stream, three
# bins apart from bin 8 on (none within three bins of the pulse's): each is over the case's threshold -- 4 dB under a carrier's peak,
# outside the -70 .. -50 dBW of the other cases -- in its own bin only, T cells a buffer, so the stream lists at least CARRIERS x T >
# 1024 = hot_capacity candidate cells and is the one the fetch analyses again; a tone that never ends gives no record (its cells are
# their row's mean), so the records are those of the plain case.  60 x 0.012 + 0.25 < 1: nothing clips.
CARRIERS, CARRIER_AMP = 60, 0.012

RAIL16, NEG16, MID16 = (32767, -32768), (-32768, -32768), (12345, -21845)
RAIL8, MID8 = (127, -128), (45, -85)
RAILU, ZEROU = (255, 0), (0, 0)

CASES = [
    # ---- every family, int16, one placement each (the linearity form runs at 32 .. 4096 under hamming, hann and boxcar)
    _c("fam32", 32, "hamming", "i16", "a", RAIL16, T=40),
    _c("fam64", 64, "hamming", "i16", "b", NEG16, T=40),
    _c("fam128", 128, "hamming", "i16", "a", MID16, T=40),
    _c("fam256box", 256, "boxcar", "i16", "a", RAIL16),
    _c("fam256hann", 256, "hann", "i16", "b", RAIL16),
    _c("fam256blackman", 256, "blackman", "i16", "a", RAIL16),      # no linearity form: subtract-first (a control)
    _c("fam512", 512, "hamming", "i16", "b", RAIL16),
    _c("fam1024", 1024, "hamming", "i16", "a", RAIL16, T=24),
    _c("fam1024b", 1024, "hamming", "i16", "b", MID16, T=24),
    _c("fam2048", 2048, "hamming", "i16", "a", RAIL16, T=24),
    _c("fam2048b", 2048, "hamming", "i16", "b", NEG16, T=24),
    _c("fam4096", 4096, "hamming", "i16", "a", RAIL16, T=24),
    _c("fam4096b", 4096, "hamming", "i16", "b", MID16, T=24),
    _c("fam8192", 8192, "hamming", "i16", "a", RAIL16, T=24),  # stft_wg: always subtract-first (a control)
    _c("fam16", 16, "hamming", "i16", "a", RAIL16, T=40, mode="dense"),   # stft_general
    _c("fam300", 300, "hamming", "i16", "b", RAIL16, mode="dense"),       # Bluestein
    # ---- every (format, placement) at 256, hamming
    _c("i16_a", 256, "hamming", "i16", "a", RAIL16),
    _c("i16_ax", 256, "hamming", "i16", "a_x", NEG16),
    _c("i16_b", 256, "hamming", "i16", "b", MID16),
    _c("i16_c", 256, "hamming", "i16", "c", RAIL16, mode="auto"),
    _c("i16_d", 256, "hamming", "i16", "d", RAIL16),
    _c("i16_ezero", 256, "hamming", "i16", "e_zero", (0, 0), row_means=True),
    _c("i16_erail", 256, "hamming", "i16", "e_rail", RAIL16, row_means=True),
    _c("i16_elone", 256, "hamming", "i16", "e_lone", RAIL16),
    _c("i8_a", 256, "hamming", "i8", "a", RAIL8),
    _c("i8_b", 256, "hamming", "i8", "b", MID8),
    _c("i8_c", 256, "hamming", "i8", "c", RAIL8, mode="auto"),
    _c("i8_d", 256, "hamming", "i8", "d", RAIL8),
    _c("i8_erail", 256, "hamming", "i8", "e_rail", RAIL8, row_means=True),
    _c("i8_elone", 256, "hamming", "i8", "e_lone", MID8),
    _c("u8_a", 256, "hamming", "u8", "a", RAILU),
    _c("u8_b", 256, "hamming", "u8", "b", RAILU),                    # the soak's (81, 132): the record starts in the previous buffer
    _c("u8_b_auto", 256, "hamming", "u8", "b", ZEROU, mode="auto"),
    _c("u8_c", 256, "hamming", "u8", "c", RAILU, mode="auto"),
    _c("u8_d", 256, "hamming", "u8", "d", ZEROU),
    _c("u8_erail", 256, "hamming", "u8", "e_rail", RAILU, row_means=True),
    _c("u8_elone", 256, "hamming", "u8", "e_lone", RAILU),
    _c("c64_a", 256, "hamming", "c64", "a", RAIL16),
    _c("c64_b", 256, "hamming", "c64", "b", NEG16),
    _c("c64_c", 256, "hamming", "c64", "c", MID16, mode="auto"),
    _c("c64_d", 256, "hamming", "c64", "d", RAIL16),
    _c("c64_erail", 256, "hamming", "c64", "e_rail", RAIL16, row_means=True),
    _c("c64_elone", 256, "hamming", "c64", "e_lone", RAIL16),
    _c("c64full_a", 256, "hamming", "c64full", "a", FULL_MANTISSA, record_cells=True),
    _c("c64full_b", 256, "hamming", "c64full", "b", FULL_MANTISSA, record_cells=True),
    # ---- levels and features at 256
    _c("dense", 256, "hamming", "i16", "b", RAIL16, mode="dense"),
    _c("auto", 256, "hamming", "i16", "a", RAIL16, mode="auto"),
    _c("runfilter", 256, "hamming", "i8", "b", RAIL8, mode="runfilter", min_hops=2.0),
    _c("prefilter", 256, "hamming", "i16", "a", MID16, T=40, spc=4, mode="prefilter", min_hops=8.0),  # (needs a minimum of two chunks)
    _c("group", 256, "hamming", "i16", "b", RAIL16, group_detect=True),
    _c("lanes2", 256, "hamming", "i16", "b", NEG16, lanes=2),
    _c("inflight", 256, "hamming", "i8", "b", RAIL8, in_flight=True),
    _c("cells", 256, "hamming", "i16", "b", RAIL16, record_cells=True),
    _c("cells1024", 1024, "hamming", "i8", "a", RAIL8, T=24, record_cells=True),
    _c("means", 256, "hamming", "i16", "a", RAIL16, row_means=True),
    _c("subfirst", 256, "hamming", "i16", "b", RAIL16, subtract_first=True),
    # ---- float64 handles: dense, map-free (f64_sparse), and map-free with the rescue
    _c("f64_i16_256", 256, "hamming", "i16", "b", RAIL16, mode="dense", precision="float64"),
    _c("f64_i8_1024", 1024, "hamming", "i8", "a", RAIL8, T=24, mode="dense", precision="float64"),
    _c("f64_u8_256", 256, "hamming", "u8", "a", RAILU, mode="dense", precision="float64"),
    _c("f64s_i16_1024", 1024, "hamming", "i16", "b", RAIL16, T=24, mode="auto", precision="float64", f64_sparse=True),
    _c("f64s_i8_256", 256, "hamming", "i8", "a", RAIL8, mode="auto", precision="float64", f64_sparse=True),
    _c("f64s_u8_1024", 1024, "hamming", "u8", "b", RAILU, T=24, mode="auto", precision="float64", f64_sparse=True),
    # the rescue: ``carriers`` weak tones over the whole target stream put more candidate cells on its lists than hot_capacity holds
    _c("f64r_i16_256", 256, "hamming", "i16", "b", RAIL16, mode="auto", precision="float64", f64_sparse=True, f64_rescue=True,
       hot_capacity=1024, carriers=CARRIERS),
    _c("f64r_i8_1024", 1024, "hamming", "i8", "a", RAIL8, T=24, mode="auto", precision="float64", f64_sparse=True, f64_rescue=True,
       hot_capacity=1024, carriers=CARRIERS),
]
# (The float64 crossing is deliberately thin, to keep the table small: every format and both sizes occur on every level -- dense,
# map-free, rescue -- but one size per (format, level) pair, not both.)
NOT_HANDLE_KEYWORDS = ("in_flight", "carriers")  # entries of Case.extra that the table reads itself
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def family(nperseg, window="hamming"):
    """the kernel family that serves a size (pyradiotracking_amd/csrc: stft_scan and its lane-group forms, stft_scan64, stft_wg,
    stft_general, Bluestein)"""
    if nperseg in (32, 64, 128):
        return "lane groups"
    if nperseg >= 8192:
        return "stft_wg"
    if nperseg == 4096:
        return "stft_scan64"
    if nperseg == 16:
        return "stft_general"
    if nperseg & (nperseg - 1):
        return "bluestein"
    return f"stft_scan {nperseg}" + ("" if window == "hamming" else f" {window}")


def n_buffers(c):
    return {"b": 4, "c": 6}.get(c.placement, 3)


def tone_segs(c):
    return max(TONE_SEGS, int(c.min_hops) + 1)


def tone_bin(c, stream=TARGET):
    if c.fmt == "c64full" and stream == TARGET:
        return 1
    return c.nperseg // 4 + 3 if stream == TARGET else c.nperseg // 2 + 2


def threshold_dbw(c):
    w = oracle.window_coefficients(c.window, c.nperseg)
    gain = synth.window_gain_db(w, FS)
    if dict(c.extra).get("carriers"):
        return float(20.0 * np.log10(CARRIER_AMP) + gain - 4.0)
    return float(np.clip(20.0 * np.log10(TONE_AMP) + gain - 10.0, -70.0, -50.0))


def carrier_bins(c):
    n = dict(c.extra).get("carriers", 0)
    bins = [b for b in range(8, c.nperseg - 4, 3) if abs(b - tone_bin(c)) > 3]
    assert len(bins) >= n
    return bins[:n]


def settings(c):
    """analysis keywords, oracle and analyzer alike"""
    return dict(sample_rate=FS, fft_nperseg=c.nperseg, fft_window=c.window, signal_threshold_dbw=threshold_dbw(c),
                signal_min_duration_ms=1e3 * c.min_hops * c.nperseg / FS)


def layout(c):
    """(lengths [buffer] in samples, constant segments [(buffer, segment)], pulses [(buffer, first segment)], expected NaN records
    [(buffer, start, end)] of the target stream's tone bin)."""
    N, T, nb, n = c.nperseg, c.T, n_buffers(c), tone_segs(c)
    lengths = [T * N] * nb
    if c.placement in ("a", "a_x"):
        t0 = (2 * c.spc + 1) if c.placement == "a" else (3 * c.spc - 1)  # inside a chunk / the last segment of one
        return lengths, [(1, t0)], [(1, t0 + 1)], [(1, t0, t0 + 1 + n)]
    if c.placement in ("b", "c"):
        at = [0, 2]
        return lengths, [(k, T - 1) for k in at], [(k + 1, 0) for k in at], [(k + 1, -1, n) for k in at]
    if c.placement == "d":
        lengths[0] += N // 2
        return lengths, [], [(1, 0)], []
    if c.placement == "e_lone":
        return lengths, [(1, T // 2)], [], []
    return lengths, [], [], []  # e_zero, e_rail


def _seed(c, s):
    return [zlib.crc32(c.name.encode()) & 0x7FFFFFFF, s]


def _quantise(c, x):
    if c.fmt == "u8":
        return synth.quantize_u8(x)
    if c.fmt == "i8":
        return synth.quantize_i8(x)
    if c.fmt in ("i16", "c64"):
        return synth.quantize_i16(x)
    return x.astype(np.complex64)


@functools.lru_cache(maxsize=None)
def wire(name):
    """[buffer] -> the samples as the handle takes them: uint8 / int8 / int16 [S, 2 n] or complex64 [S, n] (read-only)."""
    c = BY_NAME[name]
    N = c.nperseg
    lengths, consts, pulses, _ = layout(c)
    offs = np.concatenate(([0], np.cumsum(lengths)))
    total = int(offs[-1])
    rows = []
    for s in range(S):
        rng = np.random.default_rng(_seed(c, s))
        x = SIGMA * (rng.standard_normal(total) + 1j * rng.standard_normal(total))
        tones = [(k, t, tone_bin(c)) for k, t in pulses] if s == TARGET else [(1, 5, tone_bin(c, PLAIN))] if s == PLAIN else []
        for k, t, fi in tones:
            a = int(offs[k]) + t * N
            n = np.arange(tone_segs(c) * N)
            x[a: a + len(n)] += TONE_AMP * np.exp(2j * np.pi * fi * n / N)
        if s == TARGET:
            n = np.arange(total)
            for i, fi in enumerate(carrier_bins(c)):
                x += CARRIER_AMP * np.exp(2j * np.pi * (fi * n / N + 0.618 * i))
        q = _quantise(c, x)
        per = 1 if q.dtype == np.complex64 else 2
        if s == TARGET:
            value = np.complex64(c.const) if per == 1 else np.array(c.const).astype(q.dtype)
            spans = [(int(offs[k]) + t * N, N) for k, t in consts]
            if c.placement == "d":
                spans.append((int(offs[0]) + c.T * N, N // 2))
            if c.placement in ("e_zero", "e_rail"):
                spans.append((0, total))
            for a, n in spans:
                if per == 1:
                    q[a: a + n] = value
                else:
                    q[2 * a: 2 * (a + n)] = np.tile(value, n)
        rows.append((q, per))
    out = []
    for k in range(len(lengths)):
        buf = np.stack([q[per * int(offs[k]): per * int(offs[k + 1])] for q, per in rows])
        if c.fmt == "c64":
            buf = synth.i16_to_complex64(buf)
        buf = np.ascontiguousarray(buf)
        buf.setflags(write=False)
        out.append(buf)
    return out


def as_complex(c, buf):
    """what the library makes of a wire buffer: the oracle's input and the complex twin's (complex128 for a float64 handle)"""
    f64 = c.precision == "float64"
    if c.fmt == "u8":
        return synth.u8_to_complex128_like_pyrtlsdr(buf) if f64 else synth.u8_to_complex64_like_kernel(buf)
    if c.fmt == "i8":
        return synth.i8_to_complex128(buf) if f64 else synth.i8_to_complex64(buf)
    if c.fmt == "i16":
        return synth.i16_to_complex128(buf) if f64 else synth.i16_to_complex64(buf)
    return buf.astype(np.complex128) if f64 else buf


Ref = namedtuple("Ref", "records shadowed spec")  # of one buffer and stream: oracle records (OracleRecord), shadow flags, map [F, T]


@functools.lru_cache(maxsize=None)
def reference(name):
    """[buffer][stream] -> Ref, the oracle over the consecutive buffers (analyze.py:231-268)."""
    c = BY_NAME[name]
    kw = settings(c)
    p = oracle.ExtractParams(kw["signal_threshold_dbw"], 5.0, kw["signal_min_duration_ms"], 40, 0.0)
    last = [None] * S
    out = []
    with np.errstate(divide="ignore", invalid="ignore"):
        for buf in wire(name):
            x = as_complex(c, buf)
            row = []
            for s in range(S):
                freqs, times, spec = oracle.stft_power(x[s], FS, c.window, c.nperseg)
                rec = oracle.extract_records(times, spec, last[s], p)
                sig = oracle.records_to_signals(rec, freqs, TS0, str(s), 0.0)
                kept = {id(v) for v in oracle.filter_shadows(sig)}
                row.append(Ref(rec, [id(v) not in kept for v in sig], spec))
                last[s] = spec
            out.append(row)
    return out


def nan_records(name):
    """[(buffer, stream, fi, start, end)] of the oracle records whose std is NaN"""
    return [(k, s, r.fi, r.start, r.end) for k, row in enumerate(reference(name)) for s, ref in enumerate(row) for r in ref.records
            if np.isnan(r.std_db)]
