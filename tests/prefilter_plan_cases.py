"""What the two run-length pre-filter levels KEEP, cell for cell, at their edges (tests/test_prefilter_plan_contract.py on the CPU,
tests/test_gpu_prefilter_plan.py on the GPU).

Both levels scan a buffer twice: a first scan leaves threshold bits, a planning kernel decides which cells the detection needs, a
second, selective scan emits those cells into the candidate lists.  The records say nothing about the selection -- a superset of
the needed cells gives the same records -- but ``call_info().n_hot`` counts the emitted cells, and with PLANNED inputs that count is
an exact function of the plan:

RT_MODE_RUNFILTER (rt_kernels.h: MODE 6, ``plan_runs<4|8|16>``, MODE 7; nperseg 4096: rt_scan64.h).  With H the threshold bits,
    C[t]    = cell t lies in a run of >= r hot cells, rows before the buffer counting as hot  (a run through t = 0 is kept whatever
              its length: it may continue a plateau of the previous buffer)
    need[t] = C[t] | C[t + 1]                                                                 (the C[t + 1] term dropped at t = T - 1)
and MODE 7 emits exactly the set ``need`` bits (stft_scan: ``emit = LISTED ? (active ? need_seg : 0u)``): n_hot = their number.
r = min(min_run_cells, T + 1) (rt_analyze.hip, where plan_runs is launched: "a run needs r cells: more than the buffer holds ...").

RT_MODE_PREFILTER (MODE 4, ``plan_pass_b``, MODE 5).  Chunks of L segments, chunk c = segments c L .. c L + L - 1:
    full[c]   = bins hot in every segment of chunk c that lies inside the buffer    (stft_scan: ``allhot &= hot``, stored to ``p.full``)
    needed[c] = full[c - 1] | full[c] | full[c + 1]                                  (stft_scan, MODE 5: ``need = f[0] | f[-LG] | f[LG]``)
    first[t]  = bins hot in every segment 0 .. t, for t in chunk 0                   (plan_pass_b: ``m &= f[t * lg]``)
A cell is emitted if it is hot or directly precedes a hot cell, and its bin is needed (chunk 0: or in ``first[t]``) -- in ITS OWN
chunk, with one exception: the cold cell under a chunk's lowest segment is the UPPER chunk's to emit.  Where a lowest cell of a needed
bin is hot, the wave takes one more step on segment c0 - 1 and emits ``next_hot & ~hot`` there under its own ``need`` (stft_scan:
``halo ? (BELOW ? (next_hot & ~hot) : 0u)``, and the block ``if (i == L) { const bool below = ...``).  The comment above
``constexpr bool BELOW`` has nperseg 4096 hand that cell to the LOWER chunk (``BELOW = R3 <= 8``); that holds for ``stft_scan<16>``
only, which a product build does not run: nperseg 4096 is served by ``stft_scan64`` (rt_kernels.h: ``#define RT_WAVE64_4096 1``,
``scan_wave64``), and that kernel takes the step below as well (rt_scan64.h: ``halo ? (next_hot & ~hot)`` in ``emit``, and
``seg = c0 - 1; halo = true;`` behind "a lowest cell of the chunk is a candidate").  So the one convention, the upper chunk's, is
planned at every nperseg -- and the table plants the cell whose count differs between the two conventions at 256, 1024 and 4096
(``convention`` below).

The inputs are those of tests/detect_order_cases.py: a boxcar window, bin-centred tones switched at segment borders, each with a
level of its own, over noise around -180 dBW, the threshold more than 40 dB from either; a bin is hot in at most an eighth of the
segments.  So every cell's threshold bit is planned: hot exactly where a tone is on.  A stream carries ONE tone at a time, the cell
before it included: the cold cell a record starts on then holds noise alone, on which every float32 transform agrees to 1e-3 dB
(beside a tone 100 dB above it that cell is the transform's own round-off, and the std over a short plateau hangs on it).

MODE 6 takes its bits with per-bin thresholds theta as well (``make_bin_thresholds``): theta = snr x margin x (the smallest sum of
P over a complete group of ``minsum_group`` chunks of the source buffer) / (segments of a group), 0 where that buffer holds no
complete group.  The source is the buffer of the call before, on a handle's first call on the level the buffer itself
(rt_analyze.hip, enqueue_analysis, ``if (!on_hand) launch_scan<6>``: "a scan of this buffer provides them"; 0 only where that buffer holds no complete group).  ``theta_table`` computes these
for every (case, call, stream, bin) from the fed samples; the contract test fails loudly where one comes near a tone's level or
near snr x this buffer's row mean (``after_bit_scan``'s check, which would re-analyse the call: ``fell_back``).

Nothing here needs a GPU, and nothing imports torch.  The edges come from the library through the host build (rt_hostcheck.cpp:
hc_plan_tile_rows, hc_min_run_cells, hc_choose_chunk, hc_scan_family, hc_minsum_group, hc_minsum_margin); the expected counts
come from the rules above alone, never from a run of the library."""
import collections
import ctypes
import functools

import numpy as np

from oracle import analyze_oracle as oracle
from tests import detect_order_cases as dc

FS = dc.FS
WINDOW = dc.WINDOW
SNR_DB = dc.SNR_DB
MAX_HOPS = dc.MAX_HOPS
DUTY = dc.DUTY
SCAN_BLOCK = 256            # threads of a scan workgroup (rt_kernels.h: scan_block)
ROWS_PER_WAVE = 16384       # rt_core.h: kPlanRowsPerWave (its effect is checked through hc_plan_tile_rows, test_prefilter_plan_contract.py)
#: per sample format: threshold, the quietest tone's cells, noise per component.  int16 and uint8 carry half a quantisation step of
#: noise (a dither: the rounding error of a bin-centred tone is periodic, spurs instead of a floor, without it)
FORMATS = {"c64": (dc.THRESHOLD_DBW, dc.TONE_DBW, dc.SIGMA), "i16": (dc.THRESHOLD_DBW, dc.TONE_DBW, 0.5 * 2.0 ** -15), "u8": (-76.0, -46.0, 0.5 / 127.5)}

Tone = dc.Tone
Call = collections.namedtuple("Call", "T tail streams present expect")  # streams: per stream its tones; expect: count | overflow | climb
Case = collections.namedtuple("Case", "name level nperseg r L calls kw fmt edge")  # edge: what the case is there for, in words


# ---- the library's own edges -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _hc():
    lib = dc._hostcheck()
    i, d, p = ctypes.c_int, ctypes.c_double, ctypes.c_void_p
    lib.hc_plan_tile_rows.argtypes = [i, i, i]
    lib.hc_plan_runs.argtypes = [p, p, i, i, i, i]
    lib.hc_min_run_cells.argtypes = [i, d, d]
    lib.hc_min_run_cells.restype = ctypes.c_longlong
    lib.hc_choose_chunk.argtypes = [i, i, d, d, i, i, i]
    lib.hc_scan_family.argtypes = [i, p]
    lib.hc_minsum_group.argtypes = [i, i]
    lib.hc_minsum_margin.argtypes = [i]
    lib.hc_minsum_margin.restype = d
    return lib


@functools.lru_cache(maxsize=None)
def lane_group(nperseg):
    """Lanes of a lane group (rt_analyze.hip, rt_create: ``h->LG = QS ? QS : 16 * R3``): a row of threshold bits is LG 16-bit words."""
    out = np.zeros(6, np.int32)
    _hc().hc_scan_family(int(nperseg), out.ctypes.data)
    r3, qs, big, general = (int(v) for v in out[:4])
    assert r3 and not big and not general, nperseg
    return qs if qs else 16 * r3


def words(nperseg):
    """64-bit planner words per row (plan_runs: ``w = lg / 4``)."""
    return lane_group(nperseg) // 4


def tiles_per_wave(nperseg):
    return 64 // words(nperseg)


def planner_of(r):
    """rt_analyze.hip, ``kern = r <= 16 ? plan_runs<4> : r <= 256 ? plan_runs<8> : plan_runs<16>``: the counter planes of the instantiation that plans runs of r cells."""
    return 4 if r <= 16 else 8 if r <= 256 else 16


def hop_ms(nperseg):
    return 1e3 * nperseg / FS


def min_ms(r, nperseg):
    """A duration gate that a run of r cells passes and one of r - 1 fails: (r + 0.5) hops."""
    return (r + 0.5) * hop_ms(nperseg)


def run_cells(c, T):
    """r of a call of T segments (rt_analyze.hip: ``min(h->run_cells, n_seg + 1)`` ahead of plan_runs), the handle's ``min_run_cells`` from the library."""
    r = int(_hc().hc_min_run_cells(c.nperseg, float(FS), min_ms(c.r, c.nperseg) / 1e3))
    assert r == c.r, (c.name, r, c.r)
    return min(r, T + 1)


def tile_rows(c, T):
    return int(_hc().hc_plan_tile_rows(T, lane_group(c.nperseg), run_cells(c, T)))


def max_samples(c):
    return max(k.T * c.nperseg + k.tail for k in c.calls)


def chunk_len(c):
    """Segments per chunk of the case's handle (rt_core.h: choose_chunk, asked as rt_create asks it)."""
    return int(_hc().hc_choose_chunk(c.nperseg, SCAN_BLOCK, float(FS), min_ms(c.r, c.nperseg) / 1e3, c.L, n_streams(c), max_samples(c) // c.nperseg))


def prefilter_ok(c):
    """rt_analyze.hip, rt_create, ``h->ap.lv.prefilter_ok``: may the handle run the chunk-bit level?  (it needs a run of r cells to cover an aligned chunk)"""
    L = chunk_len(c)
    return L >= 4 and 2 * L - 1 <= c.r and max_samples(c) // c.nperseg >= 2 * L


@functools.lru_cache(maxsize=None)
def bin_slot(nperseg):
    """(word column, bit) of every bin in a row of threshold bits -> two int arrays [nperseg].  Lane ``lt`` of a group holds the
    bins ``bin_of<R3, LG>(lt, reg)`` in bit ``reg`` of its 16-bit word (rt_kernels.h: ``bin_of``), four lanes make a planner word;
    stft_scan64 holds 64 bins per lane, bin = lane + 64 reg (rt_kernels.h: ``lane_order_bin``'s comment), a lane's 64 bits are one planner word."""
    lg = lane_group(nperseg)
    col, bit = np.full(nperseg, -1), np.full(nperseg, -1)
    if nperseg == 4096:
        b = np.arange(nperseg)
        return b % 64, b // 64
    r3 = max(1, nperseg // 256)
    for lt in range(lg):
        for reg in range(16):
            if r3 == 1:
                b = lt + lg * reg
            else:
                g = 16 // r3
                k1, qg = lt // r3, lt % r3
                u = (reg // r3 - ((k1 * r3 // 8) & (g - 1))) & (g - 1)
                b = k1 + 16 * (qg * g + u) + 256 * (reg % r3)
            assert col[b] < 0
            col[b], bit[b] = lt // 4, 16 * (lt % 4) + reg
    assert (col >= 0).all()
    return col, bit


# ---- planting --------------------------------------------------------------------------------------------------------------------
def n_streams(c):
    return len(c.calls[0].streams)


def settings(c):
    thr = FORMATS[c.fmt][0]
    return dict(sample_rate=FS, fft_nperseg=c.nperseg, fft_window=WINDOW, signal_threshold_dbw=thr, snr_threshold_db=SNR_DB,
                signal_min_duration_ms=min_ms(c.r, c.nperseg), signal_max_duration_ms=MAX_HOPS * hop_ms(c.nperseg))


def handle_kwargs(c):
    """BatchSignalAnalyzer's keywords (without ``devices`` and ``sdr_callback_length``)."""
    kw = dict(settings(c), lanes=1, record_capacity=2048, mode=c.level, segs_per_chunk=c.L)
    kw.update(dict(c.kw))
    return kw


def params(c):
    kw = settings(c)
    return oracle.ExtractParams(kw["signal_threshold_dbw"], kw["snr_threshold_db"], kw["signal_min_duration_ms"], kw["signal_max_duration_ms"])


def raw(c, k, s):
    """Stream s of call k as it is fed: complex64 [B], int16 [2 B] or uint8 [2 B]."""
    from pyradiotracking_amd import synth

    call = c.calls[k]
    _, _, sigma = FORMATS[c.fmt]
    n = call.T * c.nperseg
    rng = np.random.default_rng([1618, k, s])
    x = (sigma * (rng.standard_normal(n + call.tail) + 1j * rng.standard_normal(n + call.tail))).astype(np.complex64)
    seg = x[:n].reshape(call.T, c.nperseg)
    i = np.arange(c.nperseg)
    for f, t0, r, level in call.streams[s]:
        seg[t0:t0 + r] += (dc.tone_amplitude(c.nperseg, level) * np.exp(2j * np.pi * ((f * i) % c.nperseg) / c.nperseg)).astype(np.complex64)
    if c.fmt == "i16":
        return synth.quantize_i16(x)
    if c.fmt == "u8":
        return synth.quantize_u8(x)
    return x


def samples(c, k, s):
    """... and as the kernels convert it: complex64 [B]."""
    from pyradiotracking_amd import synth

    x = raw(c, k, s)
    if c.fmt == "i16":
        return synth.i16_to_complex64(x)
    if c.fmt == "u8":
        return synth.u8_to_complex64_like_kernel(x)
    return x


def batch(c, k):
    return np.stack([raw(c, k, s) for s in range(n_streams(c))])


def present(c, k, s):
    p = c.calls[k].present
    return True if p is None else bool(p[s])


def plan_bits(c, k, s):
    """The planned threshold bits of stream s in call k: bool [nperseg, T], hot exactly where a tone is on."""
    call = c.calls[k]
    hot = np.zeros((c.nperseg, call.T), bool)
    for f, t0, r, _ in call.streams[s]:
        assert 0 < f < c.nperseg and 0 <= t0 and t0 + r <= call.T and r > 0, (c.name, k, s, f, t0, r)
        assert not hot[f, max(t0 - 1, 0):t0 + r + 1].any(), (c.name, k, s, f, t0, "two tones of a bin touch")
        hot[f, t0:t0 + r] = True
    return hot


# ---- the rules -------------------------------------------------------------------------------------------------------------------
def _runs(row):
    d = np.diff(np.concatenate(([0], row.astype(np.int8), [0])))
    return list(zip(np.flatnonzero(d == 1), np.flatnonzero(d == -1)))  # [start, end)


def kept_runs(hot, r, before_hot=True):
    """C: bool like ``hot`` [F, T]."""
    C = np.zeros_like(hot)
    for f in np.flatnonzero(hot.any(axis=1)):
        for a, b in _runs(hot[f]):
            if b - a >= r or (a == 0 and before_hot):
                C[f, a:b] = True
    return C


def runfilter_need(hot, r, before_hot=True):
    """need[t] = C[t] | C[t + 1]: the cells MODE 7 emits."""
    C = kept_runs(hot, r, before_hot)
    need = C.copy()
    need[:, :-1] |= C[:, 1:]
    return need


def tile_walk(hot, r, B, fault=None):
    """``need`` as the planner's tiles compute it -- a restatement of ``plan_tile_column`` (rt_core.h) in whole rows: tile
    a .. a + B - 1 sees rows a - r + 1 .. a + B + r - 1, rows before the buffer as set, rows past it as clear, and knows nothing
    beyond.  Without a fault it equals ``runfilter_need`` (the contract test holds both to hc_plan_runs); the planted faults:
    ``halo_short`` the upper halo one row short, ``before_clear`` rows before the buffer counted clear, ``drop_at_tile_end`` the
    C[t + 1] term dropped at a tile's last row, ``keep_all`` no run length asked (r = 1: every threshold cell and the cell before)."""
    F, T = hot.shape
    need = np.zeros_like(hot)
    if fault == "keep_all":
        r = 1
    for a in range(0, T, B):
        lo, hi = a - r + 1, a + B + r - 1 - (1 if fault == "halo_short" else 0)  # rows seen, inclusive
        win = np.zeros((F, hi - lo + 1), bool)
        if lo < 0 and fault != "before_clear":
            win[:, :-lo] = True
        u0, u1 = max(lo, 0), min(hi, T - 1)
        if u1 >= u0:
            win[:, u0 - lo:u1 - lo + 1] = hot[:, u0:u1 + 1]
        C = np.zeros_like(win)
        for f in np.flatnonzero(win.any(axis=1)):
            for x, y in _runs(win[f]):
                if y - x >= r:
                    C[f, x:y] = True
        for t in range(a, min(a + B, T)):
            v = C[:, t - lo].copy()
            if t + 1 < T and t + 1 <= hi and not (fault == "drop_at_tile_end" and t == a + B - 1):
                v |= C[:, t + 1 - lo]
            need[:, t] = v
    return need


def prefilter_emit(hot, L, spread=1, lower_emits=False):
    """The cells MODE 5 emits: bool like ``hot``.  ``spread``: chunks either side that a chunk bit reaches (the rule: 1);
    ``lower_emits``: the other border convention (stft_scan<16>: the LOWER chunk emits the cold cell under a chunk's lowest)."""
    F, T = hot.shape
    chunks = -(-T // L)
    full = np.zeros((F, chunks), bool)
    for ch in range(chunks):
        full[:, ch] = hot[:, ch * L:min((ch + 1) * L, T)].all(axis=1)
    needed = np.zeros_like(full)
    for d in range(-spread, spread + 1):
        lo, hi = max(0, -d), min(chunks, chunks - d)
        needed[:, lo:hi] |= full[:, lo + d:hi + d]
    first = np.logical_and.accumulate(hot[:, :min(L, T)], axis=1)
    own = np.repeat(needed, L, axis=1)[:, :T]  # the need of every cell's own chunk
    own[:, :first.shape[1]] |= first
    nxt = np.zeros_like(hot)
    nxt[:, :-1] = hot[:, 1:]
    emit = (hot | nxt) & own
    if not lower_emits:
        # the cold cell under a chunk's lowest segment: the upper chunk's need decides (and ``first`` never holds a cold cell)
        for ch in range(1, chunks):
            t = ch * L - 1
            cold = ~hot[:, t] & hot[:, t + 1]
            emit[cold, t] = needed[cold, ch]
    return emit


def planned_cells(c, k, s, fault=None, carried=None):
    """The cells stream s emits in call k on the case's level: bool [nperseg, T].  ``carried``: the cells of the call before
    (fault ``stale_need``: a need word the listed scan did not put back to zero is emitted again, where the buffer reaches it)."""
    hot = plan_bits(c, k, s)
    T = c.calls[k].T
    if not present(c, k, s):
        return np.zeros_like(hot)
    if c.level == "prefilter":
        return prefilter_emit(hot, chunk_len(c), spread=2 if fault == "spread_two" else 1)
    if fault in ("halo_short", "before_clear", "drop_at_tile_end", "keep_all"):
        out = tile_walk(hot, run_cells(c, T), tile_rows(c, T), fault)
    else:
        out = runfilter_need(hot, run_cells(c, T))
    if fault == "stale_need" and carried is not None:
        n = min(T, carried.shape[1])
        out[:, :n] |= carried[:, :n]
    return out


FAULTS = ("halo_short", "before_clear", "drop_at_tile_end", "spread_two", "stale_need", "keep_all")


def planned_counts(c, fault=None):
    """n_hot of every call: the emitted cells of the streams that take part."""
    out, carried = [], [None] * n_streams(c)
    for k in range(len(c.calls)):
        n = 0
        for s in range(n_streams(c)):
            cells = planned_cells(c, k, s, fault, carried[s])
            if present(c, k, s):
                carried[s] = cells
            n += int(cells.sum())
        out.append(n)
    return out


def bucket_fill(c, k):
    """The fullest candidate list of call k: (cells, stream)."""
    best = (0, 0)
    for s in range(n_streams(c)):
        cells = planned_cells(c, k, s)
        per = [int(cells[b::16].sum()) for b in range(16)]
        best = max(best, (max(per), s))
    return best


def sparse_fill(c, k):
    """... and of the SPARSE level on the same input (every hot cell and the cell before it): what an AUTO handle tries first."""
    best = 0
    for s in range(n_streams(c)):
        hot = plan_bits(c, k, s)
        listed = hot.copy()
        listed[:, :-1] |= hot[:, 1:]
        best = max(best, max(int(listed[b::16].sum()) for b in range(16)))
    return best


def hot_cap(c):
    cap = dict(c.kw).get("hot_capacity", 0)
    return cap if cap else dc.default_hot_cap(c.nperseg, max_samples(c) // c.nperseg)


# ---- the per-bin thresholds of MODE 6 --------------------------------------------------------------------------------------------
def theta_groups(c, T):
    """[(first segment, segments)] of the complete groups whose sums make_bin_thresholds takes the minimum of, for a buffer of T
    segments (stft_scan's epilogue, ``if (p.chunk_min ...)``: groups of ``minsum_group(L, min(GPW, 16))`` chunks, chunk index a multiple of it, every chunk
    inside the buffer; stft_scan64, ``whole = c_len == L && (c0 + L <= T)``: every complete chunk of full length, the earliest chunks being half as long where the
    handle has no chunk bits -- ``chunk_geometry``, rt_kernels.h)."""
    L = chunk_len(c)
    if c.nperseg == 4096:
        long0 = -(-T // L)
        n_short, short_len = (0, L) if (prefilter_ok(c) or long0 < 4 or L < 8) else (2 * (long0 // 4), (L + 1) // 2)
        at = n_short * short_len
        return [(a, L) for a in range(at, T - L + 1, L)]
    g = int(_hc().hc_minsum_group(L, min(SCAN_BLOCK // lane_group(c.nperseg), 16)))
    return [(a, g * L) for a in range(0, T - g * L + 1, g * L)]


def theta_table(c, k, s, spec_of):
    """theta of every bin of stream s in call k (float64 [nperseg]) and the call it comes from: call k - 1, on a handle's first call
    call k itself.  Zeros where that buffer holds no complete group -- and where the stream sat that call out, which no case with
    more than one call has (an absent stream's rows of minima are not restated here).  ``spec_of(k, s)``: the power map
    [nperseg, T] of the fed samples."""
    src = k - 1 if k > 0 else k
    T = c.calls[src].T
    groups = theta_groups(c, T)
    if not groups or not present(c, src, s):
        return np.zeros(c.nperseg), src
    spec = spec_of(src, s).astype(np.float64)
    m = groups[0][1]
    sums = np.stack([spec[:, a:a + n].sum(axis=1) for a, n in groups])
    return oracle.db_to_linear(SNR_DB) * float(_hc().hc_minsum_margin(m)) * sums.min(axis=0) / m, src


# Bin 0 under a boxcar window is the segment's mean, which the detrend removes: its cells are the transform's round-off, 1e-32 where
# only noise stands and 1e-24 in a segment that holds a tone -- and differ from one implementation to the next.  after_bit_scan holds
# theta (the quietest group of the buffer BEFORE) against this buffer's row mean for that bin too; so that the check cannot hang on
# round-off, every stream of a later call holds a tone (its row mean of bin 0 is then a million times a quiet group's), which the
# contract test asserts with a factor of 100 in hand.


# ---- the table -------------------------------------------------------------------------------------------------------------------
class _Layout:
    """Tones dealt to streams so that a stream carries one at a time (the cell before a tone included), to
    bins that walk through the word columns and bit positions."""

    def __init__(self, nperseg, T, n_str, first_bin=1, grow_to=None):
        self.nperseg, self.T = nperseg, T
        self.grow_to = grow_to if grow_to is not None else n_str  # streams are added while a tone finds no room, up to this many
        self.busy = [np.zeros(T + 2, bool) for _ in range(n_str)]
        self.tones = [[] for _ in range(n_str)]
        self.per_bin = collections.Counter()
        w = words(nperseg)
        # the j-th tone: column j mod w, the bit moving on by 5 per tone and by one per round of the columns (5 and 64 are coprime)
        col, bit = bin_slot(nperseg)
        at = {(int(a), int(b)): f for f, (a, b) in enumerate(zip(col, bit))}
        self.order = [at[(j % w, (5 * j + j // w) % 64)] for j in range(64 * w)]
        self.j = first_bin

    def n_tones(self):
        return sum(len(t) for t in self.tones)

    def room(self, t0, n):
        lo, hi = max(t0 - 1, 0), t0 + n
        return len(self.busy) < self.grow_to or any(not b[lo:hi].any() for b in self.busy)

    def _next_bin(self, s, n):
        for _ in range(64 * words(self.nperseg)):
            f = self.order[self.j % len(self.order)]
            self.j += 1
            if f != 0 and (self.per_bin[(s, f)] + n) * DUTY <= self.T:  # (bin 0: a constant, which the detrend removes)
                return f
        raise AssertionError("no bin left")

    def add(self, kind, t0, n, stream=None, bin=None):
        assert 0 <= t0 and t0 + n <= self.T and n > 0, (kind, t0, n, self.T)
        lo, hi = max(t0 - 1, 0), t0 + n  # the cell before and the tone: a cold cell lies between any two tones of a stream
        for s in ([stream] if stream is not None else range(len(self.busy))):
            if not self.busy[s][lo:hi].any():
                break
        else:
            if stream is not None or len(self.busy) >= self.grow_to:
                raise AssertionError(f"{kind}: no stream free for segments {lo} .. {hi - 1} of {self.T}")
            s = len(self.busy)
            self.busy.append(np.zeros(self.T + 2, bool))
            self.tones.append([])
        self.busy[s][lo:hi] = True
        f = bin if bin is not None else self._next_bin(s, n)
        self.per_bin[(s, f)] += n
        assert self.per_bin[(s, f)] * DUTY <= self.T, (kind, s, f)
        self.tones[s].append((f, t0, n))
        return s, f

    def streams(self, fmt, first_level=0):
        tone0 = FORMATS[fmt][1]
        out, i = [], first_level
        for ts in self.tones:
            row = []
            for f, t0, n in ts:
                i += 1
                row.append(Tone(f, t0, n, tone0 + dc.LEVEL_SPREAD_DB * ((dc.GOLDEN * i) % 1.0)))
            out.append(tuple(row))
        return tuple(out)


def edge_kinds(r, splits=None):
    """The run-length edges of the border between rows b - 1 and b as (kind, first row - b, cells).  The tile below reads r rows
    above its own (b .. b + r - 1), the tile above r - 1 rows below (b - r + 1 .. b - 1)."""
    out = [("end-last", -r, r),         # a run of r ending on the tile's last row
           ("start-first", 0, r)]       # ... starting on the next tile's first: the cell before it is the lower tile's, which needs all r rows above
    out += [(f"split-{k}", -k, r) for k in (range(1, r) if splits is None else splits)]  # k cells below the border, r - k above
    if r > 2:
        out.append(("short-split", -1, r - 1))  # one cell short, across the border: dropped
    out += [("halo-last", -1, r + 1),   # ends on the last row of the lower tile's halo
            ("halo-past", -1, r + 2)]   # ... and one row past it
    return out


def border_edges(lay, borders, r, where, splits=None, turn=0):
    """Every edge kind at a border of ``borders`` (``where``: tile | wave), the borders taking turns: the edges of one border all
    hold rows b - 1 or b, and a stream carries one tone at a time."""
    ok = [b for b in borders if b - r - 2 >= 0 and b + r + 3 <= lay.T]
    assert ok, (borders, r, lay.T)
    for i, (kind, off, n) in enumerate(edge_kinds(r, splits)):
        lay.add(f"{where}:{kind}", ok[(i + turn) % len(ok)] + off, n)


def borders(nperseg, T, r):
    """(tile rows, rows of a wave, [tile borders that are no wave borders], [wave borders]) of a call: border b lies between rows
    b - 1 and b."""
    B = int(_hc().hc_plan_tile_rows(T, lane_group(nperseg), min(r, T + 1)))
    wave = tiles_per_wave(nperseg) * B
    return B, wave, [b for b in range(B, T, B) if b % wave], list(range(wave, T, wave))


def _case(name, level, nperseg, r, calls, edge, L=0, fmt="c64", **kw):
    return Case(name, level, nperseg, r, L, tuple(calls), tuple(sorted(kw.items())), fmt, edge)


def _one_call(name, level, nperseg, r, T, lay, edge, tail=0, present=None, L=0, fmt="c64", **kw):
    return _case(name, level, nperseg, r, [Call(T, tail, lay.streams(fmt), present, "count")], edge, L=L, fmt=fmt, **kw)


def _fill(lay, r, upto):
    """Plain runs of r (kept, with the cell before) and of r - 1 (dropped) until ``upto`` tones stand: one per word column at least."""
    i = 0
    while lay.n_tones() < upto:
        t0 = 3 + (i * (2 * r + 5)) % (lay.T - 2 * r - 8)
        n = r if i % 2 == 0 else max(r - 1, 1)
        if lay.room(t0, n):
            lay.add("inside:run-r" if n == r else "inside:run-short", t0, n)
        i += 1
        assert i < 4000, "no room left"


def _geometry_case(nperseg, T, r, grow_to):
    """Every border edge at a tile border and at a wave border of one planner geometry, the tones walking through the word columns."""
    B, wave, tile_b, wave_b = borders(nperseg, T, r)
    assert wave_b, (nperseg, T, r)
    lay = _Layout(nperseg, T, 1, grow_to=grow_to)
    if tile_b:
        border_edges(lay, tile_b, r, "tile", turn=len(tile_b) // 2)
    border_edges(lay, wave_b, r, "wave")
    _fill(lay, r, words(nperseg) + 2)
    return _one_call(f"run-{nperseg}-T{T}-r{r}", "runfilter", nperseg, r, T, lay,
                     f"every border edge at a tile and a wave border, w = {words(nperseg)}, {tiles_per_wave(nperseg)} tiles a wave, tiles of {B} rows")


def _run_length_case(nperseg, T, r, grow_to):
    """Runs of r - 1, r and r + 1 inside a tile, and the border edges for this r -- every split of a run of r -- at whatever
    borders the geometry has."""
    B, wave, tile_b, wave_b = borders(nperseg, T, r)
    lay = _Layout(nperseg, T, 1, grow_to=grow_to)
    at = 2
    for n in (r - 1, r, r + 1):
        if n > 0:
            lay.add(f"inside:run-{'r' if n == r else 'short' if n < r else 'long'}", at, n, stream=0)
            at += n + 3
    border_edges(lay, sorted(tile_b + wave_b), r, "border", turn=2 + (2 * r + 8) // B)
    return _one_call(f"run-{nperseg}-T{T}-r{r}", "runfilter", nperseg, r, T, lay,
                     f"runs of r - 1, r, r + 1 and every split of a run of r = {r} over a border (plan_runs<{planner_of(r)}>), tiles of {B} rows")


def _wide_counter_case(nperseg, T, r):
    """Two streams for a long r: a run of r split in the middle over a border, a run of r - 1 across one (dropped), a short run
    through t = 0 and a run of r through T - 1."""
    B, wave, tile_b, wave_b = borders(nperseg, T, r)
    ok = [b for b in sorted(tile_b + wave_b) if b - r >= 8 and b + 2 * r + 8 <= T]
    b = ok[len(ok) // 2]
    lay = _Layout(nperseg, T, 2)
    lay.add("start:short-from-0", 0, 3, stream=0)
    lay.add(f"border:split-{r // 2}", b - r // 2, r, stream=0)
    lay.add("border:short-split", b - 1, r - 1, stream=1)
    lay.add("end:run-r-to-last", T - r, r, stream=1)
    return _one_call(f"run-{nperseg}-T{T}-r{r}", "runfilter", nperseg, r, T, lay,
                     f"plan_runs<{planner_of(r)}> at w = {words(nperseg)}: a run of r = {r} split over a border of tiles of {B} rows, r - 1 across it, t = 0, T - 1")


def _ends_case(name, nperseg, T, r, tail=0, **kw):
    """The buffer's ends: four streams."""
    lay = _Layout(nperseg, T, 4)
    lay.add("start:single-at-0", 0, 1, stream=0)                     # kept: it may continue a plateau of the buffer before
    lay.add("start:short-from-0", 0, max(r - 1, 1), stream=1)        # kept, for the same reason
    lay.add("start:short-from-1", 1, max(r - 1, 1), stream=2)        # dropped: one row into the buffer a short run is a short run
    lay.add("end:run-r-to-last", T - r, r, stream=0)                 # kept (listed; no record: it may go on in the next buffer)
    lay.add("end:short-to-last", T - max(r - 1, 1), max(r - 1, 1), stream=1)  # dropped
    lay.add("end:run-r-to-last-but-one", T - r - 1, r, stream=2)     # the last record a buffer can hold
    lay.add("inside:run-r", T // 2, r, stream=3)
    return _one_call(name, "runfilter", nperseg, r, T, lay, "a single cell at t = 0, runs of r - 1 from t = 0 and from t = 1, runs of r and r - 1 through T - 1", tail=tail, **kw)


class _TinyLayout(_Layout):
    """A buffer of a few segments: neither the duty rule of the table nor a cell's distance between tones fits it.  (A bin that is
    hot in a third of a ten-segment buffer still stands 4 dB over its row's mean against an SNR threshold of 1 dB: the contract
    test holds every decision of these cases 3 dB clear like the others'.)"""

    def add(self, kind, t0, n, stream=None, bin=None):
        assert stream is not None and 0 <= t0 and t0 + n <= self.T
        f = 0
        while f == 0:
            f = self.order[self.j % len(self.order)]
            self.j += 1
        self.tones[stream].append((f, t0, n))


def _chunk_edges(lay, L, r, c0, s0=0):
    """The chunk-bit edges around chunk c0 in streams s0 .. s0 + 4 (chunks c0 - 2 .. c0 + 3 hold nothing else there)."""
    a = c0 * L
    s, f = lay.add("chunk:cover", a, L, stream=s0)                                  # exactly one aligned chunk: L cells and the cell under it
    lay.add("chunk:near-1", a - L + 1, 2, stream=s0, bin=f)                        # a burst in the chunk below: needed, emitted
    lay.add("chunk:near+1", a + L + 1, 2, stream=s0, bin=f)                        # ... and above
    lay.add("chunk:far-2", a - 2 * L + 1, 2, stream=s0, bin=f)                     # two chunks away: not needed, nothing
    lay.add("chunk:far+2", a + 2 * L + 1, 2, stream=s0, bin=f)
    lay.add("chunk:short-low", a + 1, L - 1, stream=s0 + 1)                        # one cell short at the low end: no bit, nothing
    lay.add("chunk:short-high", a, L - 1, stream=s0 + 2)                           # ... at the high end
    lay.add("chunk:long-no-chunk", a + 1, 2 * L - 2, stream=s0 + 3)                # the longest run that covers no aligned chunk
    # the cold cell under a chunk's lowest segment, where the two chunks differ in need: chunk c0 full makes c0 - 1 and c0 + 1 needed
    s, f = lay.add("chunk:cover", a, L, stream=s0 + 4)
    lay.add("convention:upper-needed", a - L, 2, stream=s0 + 4, bin=f)             # lowest cell of c0 - 1 hot; the cell under it lies in c0 - 2 (not needed): emitted
    lay.add("convention:lower-needed", a + 2 * L, 2, stream=s0 + 4, bin=f)         # lowest cell of c0 + 2 hot (not needed); the cell under it lies in c0 + 1 (needed): nothing
    # (once more for the first: the two would cancel in a count)
    s, f = lay.add("chunk:cover", a + 8 * L, L, stream=s0 + 2)
    lay.add("convention:upper-needed", a + 7 * L, 2, stream=s0 + 2, bin=f)
    lay.add("inside:run-r", a + 4 * L + 1, r + 1, stream=s0 + 1)                   # a record: 2 L cells cover an aligned chunk wherever they start


def _relevel(streams, fmt):
    tone0 = FORMATS[fmt][1]
    return tuple(tuple(Tone(t.bin, t.t0, t.r, t.level_db - dc.TONE_DBW + tone0) for t in ts) for ts in streams)


def _sequence_case():
    """One handle on the exact level through nine calls: T larger, smaller, larger; the bins moving between word columns; a call
    that keeps nothing; a call that overflows ``hot_capacity`` in one stream; what an earlier call left in ``need``, in the segment
    list or in a counter would be counted by a later one.
    The handle is an AUTO one that its first call takes to the exact level (as in ``_auto_case``), not one pinned to
    ``runfilter``: a pinned handle REFUSES a call whose lists overflow (rt_core.h, overflow_step: kOverflowFail unless the handle
    is AUTO), where an AUTO handle analyses the one overflowing stream of four again on its own -- and stays on its level for the
    sixteen calls that follow a climb, so every later call here runs MODE 6, plan_runs and MODE 7 as well.  The GPU test runs a
    pinned handle through the same calls but the overflowing one and asks it for the same counts."""
    nperseg, r, n_str, cap = 256, 9, 4, 128
    calls, lvl = [], 0
    plan = ((1400, "climb"), (700, "edges"), (2100, "edges"), (420, "edges"), (1500, "nothing"), (1400, "overflow"), (2100, "edges"), (900, "edges"), (300, "ends"))
    for k, (T, what) in enumerate(plan):
        lay = _Layout(nperseg, T, n_str, first_bin=1 + 29 * k)
        B, wave, tile_b, wave_b = borders(nperseg, T, r)
        if what == "climb":
            for i in range(45):  # bucket 7 of stream 2: 45 bursts of 3 cells list 180 cells on the sparse level, none on the exact one
                lay.add("inside:run-short", 4 + 30 * i, 3, stream=2, bin=7 + 16 * (i % 15))
            lay.add("inside:run-r", 600, r, stream=1)
        elif what == "nothing":
            for i in range(12):  # runs of r - 1 and bursts, none through t = 0: the planner keeps no cell
                lay.add("inside:run-short", 5 + 40 * i, r - 1 if i % 2 else 3, stream=i % n_str)
        elif what == "overflow":
            for i in range(10):  # bucket 9 of stream 3: ten runs of 14 cells keep 150 cells
                lay.add("inside:run-long", 20 + 130 * i, 14, stream=3, bin=9 + 16 * (i % 15))
            lay.add("start:short-from-0", 0, 4, stream=0)
            lay.add("inside:run-r", 700, r, stream=1)
        else:
            lay.add("start:short-from-0", 0, 2 + k % 3, stream=k % n_str)
            lay.add("end:run-r-to-last", T - r - (k % 2), r + (k % 2), stream=(k + 1) % n_str)  # through T - 1: the next call's run through t = 0 may continue it
            lay.add("inside:run-r", T // 2 + 1, r, stream=(k + 2) % n_str)
            lay.add("inside:run-short", T // 3, 3, stream=(k + 3) % n_str)
            if what == "edges":
                border_edges(lay, sorted(tile_b + wave_b), r, "border", splits=(1, r // 2, r - 1), turn=k)
        for s in range(n_str):  # (every stream holds a tone in every call: see theta_table on bin 0)
            if not lay.tones[s]:
                lay.add("inside:run-short", 300 + 7 * s, 3, stream=s)
        calls.append(Call(T, 0, lay.streams("c64", lvl), None, what if what in ("climb", "overflow") else "count"))
        lvl += lay.n_tones()
    return _case("sequence-256", "auto", nperseg, r, calls,
                 "nine calls on one handle: T 1400 (climbs), 700, 2100, 420, 1500 (keeps nothing), 1400 (one stream overflows), 2100, 900, 300", L=32, hot_capacity=cap)


def _auto_case():
    """An AUTO handle whose sparse lists a planted input overflows (bursts that the exact level drops): the call is finished on the
    exact level and the handle stays there; a later call overflows ``hot_capacity`` on THAT level in one stream of four, which is
    analysed again on its own (dense).  Chunks of 32 (forced): with r = 9 the chunk-bit level does not exist, the exact one is next."""
    nperseg, r, n_str, cap = 256, 9, 4, 128
    calls, lvl = [], 0
    for k, (T, what) in enumerate(((1400, "climb"), (1100, "count"), (1400, "overflow"), (900, "count"))):
        lay = _Layout(nperseg, T, n_str, first_bin=1 + 11 * k)
        B, wave, tile_b, wave_b = borders(nperseg, T, r)
        if what == "climb":
            for i in range(45):  # bucket 3 of stream 1: 45 bursts of 3 cells list 180 cells on the sparse level, none on the exact one
                lay.add("inside:run-short", 4 + 30 * i, 3, stream=1, bin=3 + 16 * (i % 15))
            lay.add("inside:run-r", 700, r, stream=0)
        elif what == "overflow":
            for i in range(10):  # bucket 5 of stream 2: ten runs of 14 cells keep 150 cells
                lay.add("inside:run-long", 20 + 130 * i, 14, stream=2, bin=5 + 16 * (i % 15))
            lay.add("inside:run-r", 700, r, stream=0)
        else:
            border_edges(lay, sorted(tile_b + wave_b), r, "border", splits=(1, r - 1), turn=k)
            lay.add("start:short-from-0", 0, 3)
        for s in range(n_str):  # (every stream holds a tone in every call: see theta_table on bin 0)
            if not lay.tones[s]:
                lay.add("inside:run-short", 300 + 7 * s, 3, stream=s)
        calls.append(Call(T, 0, lay.streams("c64", lvl), None, what))
        lvl += lay.n_tones()
    return _case("auto-256", "auto", nperseg, r, calls, "AUTO: the sparse lists overflow, the exact level finishes the call and serves the next; one stream overflows there",
                 L=32, hot_capacity=cap)


def _table():
    out = []
    # 1. RUNFILTER, the planner's geometry: w words a row, 64 / w tiles a wave; the border edges at a tile and at a wave border
    out.append(_geometry_case(64, 16700, 9, 6))
    out.append(_geometry_case(128, 8400, 9, 6))
    out.append(_geometry_case(256, 4200, 9, 6))
    out.append(_geometry_case(1024, 1500, 9, 6))
    out.append(_geometry_case(2048, 750, 9, 6))
    out.append(_geometry_case(4096, 330, 9, 8))   # stft_scan64's MODE 6 / 7; every border is a wave's (one tile a wave)
    # 2. run lengths: the three planner instantiations and both switches between them
    out.append(_run_length_case(256, 2100, 2, 4))
    out.append(_run_length_case(256, 2100, 16, 6))
    out.append(_run_length_case(256, 2100, 17, 6))
    out.append(_run_length_case(64, 16384, 256, 16))
    out.append(_run_length_case(64, 16384, 257, 16))
    out.append(_run_length_case(1024, 600, 17, 8))
    out.append(_run_length_case(128, 2100, 17, 6))
    out.append(_run_length_case(2048, 600, 16, 8))
    out.append(_run_length_case(4096, 200, 2, 6))  # three waves of one tile
    out.append(_run_length_case(2048, 600, 17, 8))
    out.append(_run_length_case(4096, 330, 17, 8))
    # plan_runs<16> at the wider rows: a run of 257 needs 2 056 segments for the table's duty rule, so these stay with two streams
    for nperseg in (256, 1024, 2048, 4096):
        out.append(_wide_counter_case(nperseg, 2100, 257))
    # 3. kPlanRowsPerWave sets the wave count (r = 100: tiles of 400 rows, 64 to a wave, would make one wave of 25 600)
    T = 20000
    B, wave, tile_b, wave_b = borders(64, T, 100)
    assert -(-T // wave) == -(-T // ROWS_PER_WAVE) == 2 and T // (64 * 400) < 2
    lay = _Layout(64, T, 1, grow_to=9)
    border_edges(lay, wave_b, 100, "wave", splits=(1, 50, 99))
    border_edges(lay, tile_b, 100, "tile", splits=(1, 50, 99), turn=70)
    out.append(_one_call("run-64-T20000-r100", "runfilter", 64, 100, T, lay, f"the wave count comes from kPlanRowsPerWave: two waves of 64 tiles of {B} rows"))
    # 4. T against the tiling
    for T in (8320, 8319):  # tiles x rows exactly, and one less
        B, wave, tile_b, wave_b = borders(64, T, 9)
        assert B == 65 and T in (128 * B, 128 * B - 1)
        lay = _Layout(64, T, 3)
        lay.add("end:run-r-to-last", T - 9, 9, stream=0)
        lay.add("end:run-r-to-last-but-one", T - 10, 9, stream=1)
        lay.add("end:short-to-last", T - 8, 8, stream=2)
        border_edges(lay, tile_b[-3:], 9, "tile", splits=(1, 8))  # the last tiles' borders
        out.append(_one_call(f"run-64-T{T}-r9", "runfilter", 64, 9, T, lay, "T = tiles x rows: the last tile full" if T == 8320 else "T = tiles x rows - 1: the last tile one row short"))
    lay = _TinyLayout(64, 10, 3)  # most of the 64 tiles of the one wave start beyond the buffer
    lay.add("start:short-from-0", 0, 1, stream=0)
    lay.add("inside:run-r", 3, 2, stream=0)
    lay.add("inside:run-short", 2, 1, stream=1)
    lay.add("end:run-r-to-last", 8, 2, stream=1)
    lay.add("end:short-to-last", 9, 1, stream=2)
    lay.add("inside:run-long", 4, 3, stream=2)
    out.append(_one_call("run-64-T10-r2", "runfilter", 64, 2, 10, lay, "ten rows, tiles of one row: 54 of the wave's 64 tiles start beyond the buffer"))
    # 5. r > T
    lay = _TinyLayout(256, 2, 3)
    lay.add("start:short-from-0", 0, 1, stream=0)
    lay.add("end:short-to-last", 1, 1, stream=1)
    lay.add("start:short-from-0", 0, 2, stream=2)  # the whole buffer: a run through t = 0
    out.append(_one_call("run-256-T2-r9", "runfilter", 256, 9, 2, lay, "r = 9 > T = 2 (r becomes 3): only runs through t = 0 remain"))
    lay = _TinyLayout(256, 16, 3)
    lay.add("start:short-from-0", 0, 5, stream=0)
    lay.add("start:short-from-1", 1, 5, stream=1)  # off t = 0 and off T - 1: dropped
    lay.add("end:short-to-last", 11, 5, stream=2)
    out.append(_one_call("run-256-T16-r17", "runfilter", 256, 17, 16, lay, "T = r - 1 = 16 (r stays 17 = T + 1, plan_runs<8>): only runs through t = 0 remain"))
    # 6. the buffer's ends
    out.append(_ends_case("ends-256-r9", 256, 700, 9))
    out.append(_ends_case("ends-256-r9-ragged", 256, 700, 9, tail=131))
    out.append(_ends_case("ends-4096-r2", 4096, 130, 2, tail=1000))
    out.append(_ends_case("ends-64-r17", 64, 2100, 17))
    out.append(_ends_case("ends-1024-r9", 1024, 300, 9, tail=7))
    out.append(_ends_case("ends-128-r257", 128, 8400, 257))
    # 7. handle features
    g = _geometry_case(256, 4200, 9, 6)
    out.append(g._replace(name="lanes2-256", kw=(("lanes", 2),), edge="two lanes: " + g.edge))
    lay = _Layout(256, 2100, 3)
    B, wave, tile_b, wave_b = borders(256, 2100, 9)
    for s in (0, 2):
        lay.add("wave:start-first", wave_b[0], 9, stream=s)
        lay.add("tile:end-last", tile_b[3] - 9, 9, stream=s)
        lay.add("start:short-from-0", 0, 3, stream=s)
    lay.add("inside:run-r", 500, 30, stream=1)  # in the absent stream: never read
    out.append(_one_call("absent-between-256", "runfilter", 256, 9, 2100, lay, "a presence mask: an absent stream between two edge streams", present=(True, False, True)))
    for fmt, what in (("i16", "int16"), ("u8", "uint8")):
        out.append(g._replace(name=f"{what}-256", fmt=fmt, calls=tuple(k._replace(streams=_relevel(k.streams, fmt)) for k in g.calls), edge=f"{what} input: " + g.edge))
    out.append(_sequence_case())
    out.append(_auto_case())
    # 8. PREFILTER: chunk bits
    for nperseg, L, forced, r, n_chunks in ((256, 4, 4, 7, 24), (1024, 4, 4, 7, 24), (4096, 4, 4, 7, 24), (256, 32, 0, 63, 24), (1024, 8, 8, 15, 24)):
        T = n_chunks * L + L // 2  # the last chunk partly beyond T
        lay = _Layout(nperseg, T, 7)
        _chunk_edges(lay, L, r, 4)
        lay.add("start:short-from-0", 0, L - 1, stream=5)                            # through t = 0, shorter than a chunk: its cells, by ``first``
        lay.add("end:partial-last-chunk", n_chunks * L, T - n_chunks * L, stream=5)  # the cells of the last chunk inside the buffer: its bit is set
        lay.add("start:long-from-0", 0, L + 2, stream=6)                             # through t = 0 and over chunk 0
        out.append(_one_call(f"pre-{nperseg}-L{L}", "prefilter", nperseg, r, T, lay,
                             f"chunk bits, chunks of {L}: cover, one short, neighbours, t = 0, the cell under a chunk, a partial last chunk", L=forced))
    # more than 256 chunks a stream: plan_pass_b's tiles of 256 chunks and its count of needed chunks carried from tile to tile
    L, r, n_chunks = 4, 7, 300
    T = n_chunks * L
    lay = _Layout(256, T, 4)
    for s, ch in enumerate((255, 256, 257)):
        lay.add(f"chunk:cover-{ch}", ch * L, L, stream=s)
        for early in range(10 + s, 250, 40):  # needed chunks below, so that the tile's base is not zero
            lay.add("chunk:cover", early * L, L, stream=s)
    lay.add("chunk:cover-255-256", 255 * L, 2 * L, stream=3)  # 255 and 256 full: needed 254 .. 257, across the tiles' border
    lay.add("chunk:cover", 298 * L, L, stream=3)
    out.append(_one_call("pre-256-L4-chunks300", "prefilter", 256, r, T, lay, "300 chunks a stream: needed chunks at 255, 256 and 257 (plan_pass_b's second tile)", L=4))
    # two calls with different T on one handle
    calls, lvl = [], 0
    for k, n_chunks in enumerate((28, 24)):
        T = n_chunks * 4 + (2 if k == 0 else 0)
        lay = _Layout(256, T, 7, first_bin=1 + 37 * k)
        _chunk_edges(lay, 4, 7, 4 if k == 0 else 5)
        lay.add("start:short-from-0", 0, 3, stream=5 + k)
        calls.append(Call(T, 0, lay.streams("c64", lvl), None, "count"))
        lvl += lay.n_tones()
    out.append(_case("pre-256-L4-two-calls", "prefilter", 256, 7, calls, "two calls of 114 and 96 segments on one handle, the edges at other chunks and bins", L=4))
    return out




CASES = _table()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ---- the oracle's view of a case -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=32)
def spec(name, k, s):
    """(freqs, times, power map [nperseg, T]) of the samples as the kernels convert them."""
    c = BY_NAME[name]
    return oracle.stft_power(samples(c, k, s), FS, WINDOW, c.nperseg)


def last_present(c, k, s):
    """The latest call before k that stream s took part in (its look-back), or None."""
    for j in range(k - 1, -1, -1):
        if present(c, j, s):
            return j
    return None


Analysis = collections.namedtuple("Analysis", "records shadowed")


@functools.lru_cache(maxsize=256)
def analyse(name, k, s):
    """The oracle's records of stream s in call k (its look-back: the stream's buffer before) and their shadow verdicts."""
    c = BY_NAME[name]
    if not present(c, k, s):
        return Analysis([], [])
    freqs, times, sp = spec(name, k, s)
    j = last_present(c, k, s)
    last = spec(name, j, s)[2] if j is not None else None
    records = oracle.extract_records(times, sp, last, params(c))
    signals = oracle.records_to_signals(records, freqs, dc.TS0, str(s), 0)
    kept = {id(v) for v in oracle.filter_shadows(signals)}
    return Analysis(records, [id(v) not in kept for v in signals])


def records_from_cells(c, k, s, cells):
    """The records a detection finds that is given only ``cells`` (bool [nperseg, T]) of call k: (fi, start, end), the planned
    bits standing for the thresholds, the look-back as the reference walks it (analyze.py:382-398)."""
    hot = plan_bits(c, k, s) & cells
    T = c.calls[k].T
    j = last_present(c, k, s)
    back = plan_bits(c, j, s) if j is not None else None
    _, times, _ = spec(c.name, k, s)
    p = params(c)
    out = []
    for f in np.flatnonzero(hot.any(axis=1)):
        for a, b in _runs(hot[f]):
            if b == T:
                continue
            lo = a - 1
            if a == 0:
                lo = 0
                if back is not None:
                    n = 0
                    while n < back.shape[1] - 1 and back[f, back.shape[1] - 1 - n]:
                        n += 1
                    lo = -(n + 1)
            elif not cells[f, a - 1]:
                continue  # (a run without the cell before it: the library reports an internal error)
            d = times[b] - (-times[-lo] if lo < 0 else times[lo])
            if p.signal_min_duration <= d <= p.signal_max_duration:
                out.append((int(f), int(lo), int(b)))
    return sorted(out)
