"""Long call sequences through one handle (tests/test_sequence_contract.py on the CPU, tests/test_gpu_sequences.py on the GPU).

What a handle carries from call to call -- three rotating look-back tails ``[S][K][N]`` that the sparse scans write only in part,
the previous call's segment count, AUTO's level and probe counter, the exact pre-filter's thresholds, two alternating call slots --
only shows after the fourth call: call k writes the tail call k - 3 wrote, so within three calls no tail is written twice and
whatever a scan fails to overwrite is still the zeros of the allocation, which a walk reads as cold.

A schedule is a list of per-call segment counts ``T[k]`` and ragged sample tails ``rag[k] < nperseg``, in units of segments, so that
one schedule serves every nperseg.  At every boundary j (between calls j - 1 and j) every stream s holds up to six bin-centred tones
i at -68 dBW peak over ``synth.NOISE_SIGMA``: tone i is hot on the last ``d`` whole segments of buffer j - 1 (and its ragged tail) and
on the first ``e`` of buffer j,

    d = min(D[(2 j + i + s) % 7], T[j - 1] - 1, T[j] - 2)        e = min(E[(j + i) % 5], T[j] - 1)

each dropped when less than 1.  (T[j] - 2, not T[j] - 1: the walk stops ON the cold cell d + 1 back, and the reference reads its time
from the CURRENT buffer's axis, ``times[d + 1]`` -- with d = T[j] - 1 that is the IndexError DESIGN section 2 pins as a deviation,
which no schedule here may raise.)  A bin-centred tone over whole segments under a hamming window lights its bin and the two beside it
and nothing else, so every reach-back is exactly ``d`` cells deep, whatever nperseg.  The tones of a stream peak half a dB apart
(-68, -68.5 ... -70.5 dBW): records of equal level that overlap in time would leave the shadow filter's ``other.max > sig.max`` to
float32 round-off -- DESIGN section 2 pins that tie as undecidable -- and the verdicts are compared exactly here.

* Schedule A: varying lengths -- calls shorter than K (33, 9, 2), one just over a default chunk (33), an empty one (T = 0), lengths
  that are no multiple of any chunk length, reach-backs over one and two chunk boundaries, and the same bin reaching back by
  different depths at boundaries j and j - 3 (the two that share a tail buffer).  After the empty call two more tones: one from
  sample 0, and one whose first hot segment is segment 1 -- with an empty previous map the reference's walk has ``lo_limit = 1 - 0``
  and stops ON that segment; after a reset (no previous map) it goes on to segment 0.
* Schedule B: ten calls of 96 segments with the same tables.
* Schedule C: equal lengths, the noise level moving quiet -> floor -> higher floor -> floor -> quiet, for AUTO and the pre-filters.
* Schedule P: schedule A's tables on ten short calls (at most 47 segments) for the covering table of tests/combo_cases.py: an empty
  call, one under K / 4 segments (9), one just over a chunk of 32 (33), four shorter than K = 42 (33, 35, 9, 41), so that a walk reads a tail wider
  than the call, and each of the three rotating tails is written at least three times.  The first three calls are no shorter than K
  (a misplaced column of a short call shows at once, not only on a tail written twice), and no T / h, h hot segments of a row, lies
  within 4 % of the SNR thresholds the table uses (2.9 and 8 dB): a tone's cells over their row's mean are T / h.

Also here: a NumPy model of the look-back tail with the two mutations the old three-call tests cannot see (``tail_model_records``),
the float64 restatement the seed guard of schedule C uses (``records_f64``), and the helper that feeds a schedule's calls to a handle
and holds every call and stream to the oracle (``hold_sequence``)."""
import datetime
import functools
from collections import namedtuple

import numpy as np

from oracle import analyze_oracle as oracle
from pyradiotracking_amd import synth
from tests import precision64 as p64
from tests import stream_settings_cases as ssc

TS0 = datetime.datetime(2024, 1, 1, tzinfo=datetime.timezone.utc)
FS = 300000
WINDOW = "hamming"
PEAK_DBW = -68.0
LEVEL_STEP_DB = 0.5  # tone i peaks at -68 - 0.5 i dBW, see the module docstring
D_TAB = (1, 5, 31, 12, 33, 2, 20)
E_TAB = (3, 1, 6, 2, 4)
MIN_HOPS, MAX_HOPS, SNR_DB = 2.5, 40.0, 3.0
WIRE_GAIN = 20.0            # uint8 / int16 cases: the samples times 20 (26 dB) before quantisation ...
WIRE_SHIFT_DB = 26.0        # ... and the threshold raised by as much
WIRE_SIGMA = 0.012 / WIRE_GAIN  # noise well over the uint8 step after the gain (tests/test_gpu_parity.py: test_uint8_wire_format_ingestion)

Schedule = namedtuple("Schedule", "name T rag_base extras e_min sigmas noisy d_max n_tones", defaults=(99, 6))

A_T = (96, 70, 96, 33, 96, 9, 64, 2, 96, 0, 40, 96, 70)
A_RAG = (5, 0, -1, 7, 0, 3, 0, 1, 0, 100, 0, 9, 0)  # -1: nperseg - 1; all mod nperseg
SCHEDULES = {
    "A": Schedule("A", A_T, A_RAG, True, 0, None, None),
    "B": Schedule("B", (96,) * 10, (0,) * 10, False, 0, None, None),
    # B for the chunk-bit pre-filter: every run at least 10 segments long (e stretched), see test_gpu_sequences
    "B10": Schedule("B10", (96,) * 10, (0,) * 10, False, 10, None, None),
    "P": Schedule("P", (47, 47, 47, 33, 35, 9, 47, 0, 41, 47), (5, 0, -1, 7, 0, 3, 0, 100, 0, 9), True, 0, None, None),
}

# Schedule C: noise regimes.  The per-call sigma moves quiet -> floor -> higher floor -> floor -> quiet; stream 1 alone is noisy in
# two calls of the quiet tail.  Floor: 2 dB over the -90 dBW threshold (half of all cells pass it), higher floor: 10 dB over it (the
# constants of test_auto_climbs_from_the_chunk_bit_prefilter_to_the_exact_one_under_a_high_noise_floor and of
# test_exact_run_length_prefilter_equals_dense, tests/test_gpu_parity.py).  Minimum 8 hops, every run at least 10 segments.
# The quiet tail: AUTO stays `sticky_len` calls on a level it climbed to before it probes the level below (rt_analyze.hip: 16 at
# first, doubled by every further climb).  Every size climbs twice here (calls 2 and 3), so the first probe is due 33 calls behind
# the second climb, at call 35, the next 17 calls later, and nperseg 4096, which climbs to the dense level, is back on the sparse one
# at call 69: a descent cannot show within 16 calls, whatever the input; the quiet calls cost next to nothing.
# The pulses are thinned -- three tones per stream, reach-backs of at most 12 segments -- so that the quiet tail is quiet for AUTO
# too: it leaves a pre-filter level upwards (`unselective`, rt_analyze.hip) when more than half of a call's segments hold cells to
# keep, or more than 1 / 32 of all cells are on the lists; six tones of 10 + 33 hot segments in 64 are both, at nperseg 128.
C_D_MAX, C_TONES = 12, 3
C_MIN_HOPS = 8.0
C_CALLS = 72
SIGMA_FLOOR = float(np.sqrt(10.0 ** ((-90.0 + 2.0) / 10.0) * FS / 2.0))
SIGMA_HIGH = float(np.sqrt(10.0 ** ((-90.0 + 10.0) / 10.0) * FS / 2.0))
C_SIGMAS = (ssc.SIGMA_QUIET, ssc.SIGMA_QUIET, SIGMA_FLOOR, SIGMA_HIGH, SIGMA_HIGH, SIGMA_FLOOR) + (ssc.SIGMA_QUIET,) * (C_CALLS - 6)
C_NOISY = (1, (9, 10), SIGMA_FLOOR)
SCHEDULES["C"] = Schedule("C", (64,) * C_CALLS, (0,) * C_CALLS, False, 10, C_SIGMAS, C_NOISY, C_D_MAX, C_TONES)
#: noise seeds of schedule C per nperseg, searched on the CPU from 1 upwards (the first one passed at every size): the float32 oracle
#: and its float64 restatement find the same records on every call and stream (tests/test_sequence_contract.py holds them to that)
C_SEEDS = {128: 1, 256: 1, 1024: 1, 4096: 1}


def n_streams(nperseg):
    """Five streams, so that two or three lanes split unevenly; three from nperseg 8192 on."""
    return 5 if nperseg < 8192 else 3


def rag(sched, nperseg):
    return [(nperseg - 1 if r < 0 else r) % nperseg for r in sched.rag_base]


def hop_s(nperseg, fs=FS):
    return nperseg / float(fs)


def settings(nperseg, fs=FS, min_hops=MIN_HOPS, **over):
    """Analysis keywords (oracle and analyzer alike): 2.5 hops minimum, 40 hops maximum (K = 42 tail columns), 3 dB SNR, the default
    threshold."""
    kw = dict(sample_rate=fs, fft_nperseg=nperseg, fft_window=WINDOW, signal_min_duration_ms=1e3 * min_hops * hop_s(nperseg, fs),
              signal_max_duration_ms=1e3 * MAX_HOPS * hop_s(nperseg, fs), snr_threshold_db=SNR_DB)
    kw.update(over)
    return kw


def tail_cols(nperseg, fs=FS):
    """K as rt_create derives it: floor(max duration / hop) + 2."""
    _, times, _ = oracle.stft_power(np.zeros(2 * nperseg, np.complex64), fs, WINDOW, nperseg)
    return int(np.floor(settings(nperseg, fs)["signal_max_duration_ms"] / 1000 / (times[1] - times[0]))) + 2


def tone_bins(nperseg, s):
    """Six tones at bins round((-0.4 + 0.13 i + 0.004 s) N), in fftfreq order; under 39 bins as many as fit five apart (at least two)."""
    if nperseg >= 39:
        return [int(round((-0.4 + 0.13 * i + 0.004 * s) * nperseg)) % nperseg for i in range(6)]
    n = max(2, min(6, nperseg // 5))
    return [2 + (nperseg // n) * i for i in range(n)]


def extra_bins(nperseg, s):
    """The two tones after schedule A's empty call (none where the bins do not fit: there one of the tones is moved to start at segment 1,
    ``shifted_tone``)."""
    if nperseg < 64:
        return []
    return [int(round((0.35 + 0.002 * s) * nperseg)), int(round((0.45 + 0.002 * s) * nperseg))]


def reach(sched, j, s, i):
    """(d, e) of tone i of stream s at boundary j (0 where dropped)."""
    T = sched.T
    if j < 1 or j >= len(T):
        return 0, 0
    d = min(D_TAB[(2 * j + i + s) % 7], sched.d_max, T[j - 1] - 1, T[j] - 2)
    e = min(max(E_TAB[(j + i) % 5], sched.e_min), T[j] - 1)
    return max(d, 0), max(e, 0)


def empty_call(sched):
    return sched.T.index(0) if 0 in sched.T else None


def shifted_tone(sched, k, s, nperseg):
    """Under 64 bins: the tone that starts at segment 1 behind the empty call -- the one that reaches back least over the next
    boundary, so that its row stays mostly cold and the SNR gate opens."""
    n = len(tone_bins(nperseg, s)[:sched.n_tones])
    return min(range(n), key=lambda i: reach(sched, k + 1, s, i)[0])


def hot_spans(sched, k, s, nperseg):
    """[(bin, first segment, end segment, through the ragged tail)] of call k, stream s."""
    out = []
    T = sched.T[k]
    z = empty_call(sched)
    after_empty = sched.extras and z is not None and k == z + 1
    shifted = shifted_tone(sched, k, s, nperseg) if after_empty and not extra_bins(nperseg, s) else None
    for i, b in enumerate(tone_bins(nperseg, s)[:sched.n_tones]):
        _, e = reach(sched, k, s, i)
        d, _ = reach(sched, k + 1, s, i)
        if i == shifted:
            out.append((b, 1, 5, False))  # under 64 bins there is no room for two more tones: one of the six starts at segment 1
        elif e:
            out.append((b, 0, e, False))
        if d:
            out.append((b, T - d, T, True))
    if after_empty:
        xb = extra_bins(nperseg, s)
        if xb:
            out.append((xb[0], 0, 4, False))
            out.append((xb[1], 1, 5, False))
    return out


def merged_spans(spans):
    """The spans of one bin that touch or overlap become one (a tone is added once per sample)."""
    out = []
    for b, a, e, through in sorted(spans):
        if out and out[-1][0] == b and a <= out[-1][2]:
            out[-1] = (b, out[-1][1], max(out[-1][2], e), out[-1][3] or through)
        else:
            out.append((b, a, e, through))
    return out


def call_sigma(sched, k, s, base):
    if sched.sigmas is None:
        return base
    if sched.noisy and s == sched.noisy[0] and k in sched.noisy[1]:
        return sched.noisy[2]
    return sched.sigmas[k]


def buffer(sched, nperseg, k, S=None, fs=FS, sigma=synth.NOISE_SIGMA, seed=None, peak_dbw=PEAK_DBW):
    """complex64 [S, T[k] nperseg + rag[k]]: call k of every stream.  Noise from (seed, k, s); the tones exp(2 pi j bin n / N), n
    counted from the buffer's first sample, added in float64 and rounded once.  ``peak_dbw``: the level of tone 0."""
    S = n_streams(nperseg) if S is None else S
    if seed is None:
        seed = 2024 if sched.sigmas is None else C_SEEDS.get(nperseg, 1)
    n = sched.T[k] * nperseg + rag(sched, nperseg)[k]
    w = oracle.window_coefficients(WINDOW, nperseg)
    amps = {}
    for s in range(S):
        for i, b in enumerate(tone_bins(nperseg, s) + extra_bins(nperseg, s)):
            amps[(s, b)] = synth.amp_for_peak_dbw(peak_dbw - LEVEL_STEP_DB * i, w, fs)
    out = np.empty((S, n), np.complex64)
    seg_idx = np.arange(nperseg)
    for s in range(S):
        rng = np.random.default_rng([seed, k, s])
        x = rng.standard_normal((n, 2), dtype=np.float32)
        x *= np.float32(call_sigma(sched, k, s, sigma))
        x = x.view(np.complex64)[:, 0]
        for b, a_seg, b_seg, through in merged_spans(hot_spans(sched, k, s, nperseg)):
            a, e = a_seg * nperseg, (n if through else b_seg * nperseg)
            tone = np.resize(amps[(s, b)] * np.exp(2j * np.pi * ((b * seg_idx) % nperseg) / nperseg), e - a)  # (a is a whole segment: one period, tiled)
            x[a:e] = (x[a:e].astype(np.complex128) + tone).astype(np.complex64)
        out[s] = x
    return out


# ---- input formats ---------------------------------------------------------------------------------------------------------------
def wire(x, fmt):
    """(what the handle is fed, what the reference arithmetic sees) for complex64 ``x``:
    ``c64``; ``u8`` / ``i16`` / ``i8`` (the kernels' conversion to complex64); ``c128`` (widened exactly); ``u8f64`` (bytes into a
    float64 handle: pyrtlsdr's conversion); ``i16f64`` / ``i8f64`` (integers into a float64 handle: the exact widening)."""
    if fmt == "c64":
        return x, x
    if fmt == "c128":
        y = x.astype(np.complex128)
        return y, y
    if fmt in ("u8", "u8f64"):
        raw = synth.quantize_u8(x, gain=WIRE_GAIN)
        return raw, (synth.u8_to_complex64_like_kernel(raw) if fmt == "u8" else synth.u8_to_complex128_like_pyrtlsdr(raw))
    if fmt in ("i16", "i16f64"):
        raw = synth.quantize_i16(x, gain=WIRE_GAIN)
        return raw, (synth.i16_to_complex64(raw) if fmt == "i16" else synth.i16_to_complex128(raw))
    if fmt in ("i8", "i8f64"):
        raw = synth.quantize_i8(x, gain=WIRE_GAIN)
        return raw, (synth.i8_to_complex64(raw) if fmt == "i8" else synth.i8_to_complex128(raw))
    raise ValueError(fmt)


WIRE_FORMATS = ("u8", "u8f64", "i16", "i16f64", "i8", "i8f64")
F64_FORMATS = ("c128", "u8f64", "i16f64", "i8f64")


def is_wire(fmt):
    return fmt in WIRE_FORMATS


def case_settings(nperseg, fmt="c64", **over):
    kw = settings(nperseg, **over)
    if is_wire(fmt):
        kw["signal_threshold_dbw"] = kw.get("signal_threshold_dbw", -90.0) + WIRE_SHIFT_DB
    return kw


def case_sigma(fmt):
    return WIRE_SIGMA if is_wire(fmt) else synth.NOISE_SIGMA


# ---- the oracle over a schedule --------------------------------------------------------------------------------------------------
def extract(times, spec, spec_last, params):
    """``oracle.extract_records`` on the rows that hold a cell not under the threshold (a row without one yields nothing: every
    probe fails analyze.py:370), bins mapped back.  Rows are independent, so the records are those of the whole map; at 16 384 bins
    the Python loop over quiet rows would take minutes."""
    if spec.shape[1] == 0:
        return []
    rows = np.flatnonzero(~(spec < params.signal_threshold).all(axis=1))
    if len(rows) == 0:
        return []
    last = None if spec_last is None else spec_last[rows]
    return [r._replace(fi=int(rows[r.fi])) for r in oracle.extract_records(times, spec[rows], last, params)]


def shadow_flags(records, freqs):
    sigs = oracle.records_to_signals(records, freqs, TS0, "0", 0)
    return [oracle.shadow_index(x, sigs) is not None for x in sigs]


def params_of(kw):
    return oracle.ExtractParams(kw.get("signal_threshold_dbw", -90.0), kw.get("snr_threshold_db", 5.0), kw.get("signal_min_duration_ms", 8),
                                kw.get("signal_max_duration_ms", 40), 0.0)


Call = namedtuple("Call", "records shadowed")


@functools.lru_cache(maxsize=None)
def oracle_run(name, nperseg, fmt="c64", events=(), min_hops=MIN_HOPS, S=None):
    """[call][stream] -> Call(oracle records, shadow verdicts): every call of the schedule through one analyzer state per stream.
    ``events``: ("reset", k, s) -- stream s starts call k without a previous map; ("snr", k, s, dB) -- its SNR threshold changes
    before call k (a new analyzer in the reference: no previous map either)."""
    sched = SCHEDULES[name]
    S = n_streams(nperseg) if S is None else S
    kws = [case_settings(nperseg, fmt, min_hops=min_hops) for _ in range(S)]
    last = [None] * S
    out = []
    for k in range(len(sched.T)):
        for ev in events:
            if ev[1] == k:
                last[ev[2]] = None
                if ev[0] == "snr":
                    kws[ev[2]] = dict(kws[ev[2]], snr_threshold_db=ev[3])
        _, seen = wire(buffer(sched, nperseg, k, S, sigma=case_sigma(fmt)), fmt)
        row = []
        for s in range(S):
            freqs, times, spec = oracle.stft_power(seen[s], FS, WINDOW, nperseg)
            recs = extract(times, spec, last[s], params_of(kws[s]))
            row.append(Call(recs, shadow_flags(recs, freqs)))
            last[s] = spec
        out.append(row)
    return out


def key(records):
    return [(int(r.fi), int(r.start), int(r.end)) for r in records]


def rec_key(rec):
    return list(zip(rec["fi"].tolist(), rec["start"].tolist(), rec["end"].tolist()))


def records_f64(x, nperseg, spec_last64, params, fs=FS):
    """The float64 restatement: ``oracle.extract_records`` on ``precision64.stft_power_f64(...).P`` -> (records, map [F, T])."""
    ref = p64.stft_power_f64(np.asarray(x, np.complex64), fs, WINDOW, nperseg)
    spec = np.ascontiguousarray(ref.P.T)
    T = spec.shape[1]
    times = np.arange(nperseg / 2, len(x) - nperseg / 2 + 1, nperseg) / float(fs)
    return extract(times[:T], spec, spec_last64, params), spec


# ---- the look-back tail, as the sparse scans write it ----------------------------------------------------------------------------
TAIL_RULES = ("correct", "drop_stop", "offset")


def tail_model_records(name, nperseg, s, L, rule="correct", n_calls=None, fs=FS):
    """[call] -> record keys of stream s when the look-back reads a model of the sparse tail instead of the true previous map.

    Three rotating ``[N][K]`` arrays (zeros at first); call k writes array k % 3 and reads the one call k - 1 wrote.  Segment
    ``seg`` of a call of T segments belongs to column ``seg - (T - K)`` (columns under 0 are not kept); within a chunk of ``L``
    segments a cell is written iff the later cells of its chunk all pass the absolute threshold (rt_kernels.h: the sparse tail).
    A walk at look-back index lo < 0 reads column K + lo; beyond K cells back the true map stands in (such a run is longer than
    the maximum duration either way).  ``rule``:
      ``correct``    as above;
      ``drop_stop``  the cold cell a walk stops on is not written (the mask and-ed with the cell's own hot bit);
      ``offset``     the column offset ignores T < K (column ``seg - max(0, T - K)``)."""
    assert rule in TAIL_RULES
    sched = SCHEDULES[name]
    K = tail_cols(nperseg, fs)
    params = params_of(settings(nperseg, fs))
    thr = params.signal_threshold
    tails = [np.zeros((nperseg, K), np.float32) for _ in range(3)]
    prev_true = None
    out = []
    for k in range(len(sched.T) if n_calls is None else n_calls):
        x = buffer(sched, nperseg, k, s + 1, fs)[s]
        _, times, spec = oracle.stft_power(x, fs, WINDOW, nperseg)
        T = spec.shape[1]
        if prev_true is None:
            prev = None
        else:
            prev = np.array(prev_true)
            Kp = min(K, prev.shape[1])
            if Kp:
                prev[:, prev.shape[1] - Kp:] = tails[(k - 1) % 3][:, K - Kp:]
        out.append(key(extract(times, spec, prev, params)))
        dst = tails[k % 3]
        off = max(0, T - K) if rule == "offset" else T - K
        for c0 in range(0, T, L):
            allhot = np.ones(nperseg, bool)
            for seg in range(min(c0 + L, T) - 1, c0 - 1, -1):
                hot = ~(spec[:, seg] < thr)
                col = seg - off
                if 0 <= col < K:
                    m = allhot & hot if rule == "drop_stop" else allhot
                    dst[m, col] = spec[m, seg]
                allhot &= hot
        prev_true = spec
    return out


# ---- feeding a handle ------------------------------------------------------------------------------------------------------------
def enqueue(b, feed, fmt):
    if fmt in ("u8", "u8f64"):
        b.enqueue_bytes(np.ascontiguousarray(feed))
    elif fmt in ("i16", "i16f64"):
        b.enqueue_int16(np.ascontiguousarray(feed))
    elif fmt in ("i8", "i8f64"):
        b.enqueue_int8(np.ascontiguousarray(feed))
    else:
        b.enqueue(np.ascontiguousarray(feed))


def max_samples(sched, nperseg):
    return max(t * nperseg + r for t, r in zip(sched.T, rag(sched, nperseg)))


def run_handle(b, sched, nperseg, fmt="c64", pipelined=False, before_call=None, after_fetch=None, S=None):
    """Every call of the schedule through handle ``b`` -> [(records, call_info)].  ``pipelined``: call k + 1 is enqueued before call
    k is fetched.  ``before_call(k)`` runs ahead of call k's enqueue (serial runs only), ``after_fetch(k, rec)`` behind its fetch."""
    n = len(sched.T)
    feeds = (lambda k: wire(buffer(sched, nperseg, k, S, sigma=case_sigma(fmt)), fmt)[0])
    out = []
    if pipelined:
        enqueue(b, feeds(0), fmt)
    for k in range(n):
        if pipelined:
            if k + 1 < n:
                enqueue(b, feeds(k + 1), fmt)
        else:
            if before_call:
                before_call(k)
            enqueue(b, feeds(k), fmt)
        rec = b.fetch_records()
        out.append((rec, b.native.call_info()))
        if after_fetch:
            after_fetch(k, rec)
    return out


def hold_sequence(runs, name, nperseg, fmt="c64", events=(), min_hops=MIN_HOPS, form="lin", f64_tol=None, note=None, what="", S=None):
    """``runs`` = ``run_handle``'s result.  After every call, per stream: (fi, start, end) and the shadow verdicts equal the oracle's;
    the float fields lie within the precision64 model of the float64 transform of the same input (look-back cells from the previous
    call's reference, L from call_info) -- on a float64 handle within ``f64_tol`` = (dB, std) of the oracle's own float64 figures.
    ``note(field, ratio)`` collects worst ratios.  Returns (records, negative starts) counted over the schedule."""
    sched = SCHEDULES[name]
    S = n_streams(nperseg) if S is None else S
    want = oracle_run(name, nperseg, fmt, events, min_hops, S)
    prev = [None] * S
    n_rec = n_neg = 0
    for k, (rec, info) in enumerate(runs):
        L = max(1, int(info.segs_per_chunk))
        _, seen = wire(buffer(sched, nperseg, k, S, sigma=case_sigma(fmt)), fmt)
        for ev in events:
            if ev[1] == k:
                prev[ev[2]] = None
        for s in range(S):
            mine = rec[rec["stream"] == s]
            w = want[k][s]
            tag = f"{what} call {k} (T {sched.T[k]}) stream {s}"
            assert rec_key(mine) == key(w.records), f"{tag}: records differ from the oracle's\n got  {rec_key(mine)}\n want {key(w.records)}"
            assert [bool(v) for v in mine["shadowed"]] == w.shadowed, f"{tag}: shadow verdicts"
            if f64_tol is not None:
                check_f64(mine, w.records)  # max / avg / noise / snr within DB_TOL, std within STD_TOL
            elif sched.T[k] > 0:
                ref = p64.stft_power_f64(seen[s], FS, WINDOW, nperseg)
                bd = p64.cell_bounds(ref, form)
                if len(mine):
                    pr = prev[s]
                    chk = p64.check_records(mine, ref, bd, L, pr[0] if pr else None, pr[1] if pr else None, what=tag)
                    assert not chk.failures, "\n".join(chk.failures[:8])
                    if note:
                        for f, v in chk.worst.items():
                            note(f"{f} ({form})", v)
                prev[s] = (ref, bd)
            else:
                prev[s] = None
            n_rec += len(mine)
            n_neg += int((mine["start"] < 0).sum())
    return n_rec, n_neg


def check_f64(rec, want):
    from tests.test_gpu_float64_path import _check

    _check(rec, want)


def trace(runs):
    """One line per call: mode_used / fell_back / dense streams / records."""
    return " ".join(f"{k}:{i.mode_used}/{i.fell_back}/{i.n_dense_streams}/{len(r)}" for k, (r, i) in enumerate(runs))
