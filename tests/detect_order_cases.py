"""Every ordering routine of the sparse detection at its size edges (tests/test_detect_order_contract.py on the CPU,
tests/test_gpu_detect_order.py on the GPU).

The sparse scan emits candidate cells as 32-bit keys (``bin << tbits | t``) into 16 lists per stream (bucket = bin & 15), in the
order the waves get there; one of many routines then puts each list into (bin, t) order before ``detect_runs`` walks it.  Which one
is chosen at run time from the bin count, the bits of the call's segment count and the list's length (``bucket_routine``,
``group_routine``, ``f64_routine`` below restate the three switches).  The suite's other files reach these routines with random
pulses only; here every list's length is PLANNED, cell for cell.

The inputs: a boxcar window and bin-centred tones switched on and off at segment borders, over very quiet noise.  A tone in bin
``b`` over segments ``t0 .. t0 + r - 1`` puts exactly those ``r`` cells above the threshold and nothing else; the scan lists a cell
if it is hot or directly precedes a hot one (rt_kernels.h, ``emit = hot | next_hot``), so such a tone adds ``r + 1`` cells to the
list of bucket ``b & 15`` (``r`` where it starts on segment 0).  One stream carries 16 independent lists, so one stream holds up to
16 different edges.  A plateau of ``PLATEAU_MIN`` cells and more yields a record, a burst of up to ``BURST_MAX`` cells adds cells
but no record (it fails the duration gate), which trims a fill to any number.  The plateaus of a bucket are dealt to its bins in
turn and spread over the whole buffer, so they overlap in time and cross chunk borders: the emitted list is thoroughly out of
(bin, t) order.  A bin is hot in at most an eighth of the segments and the tones of a stream lie within ``LEVEL_SPREAD_DB`` of each
other, so a hot cell is at least 6 dB over its row's mean against an SNR threshold of ``SNR_DB`` = 1 dB; every tone has a level
of its own (a golden-ratio sequence), so that no shadow verdict hangs on the last bits of two maxima.

Nothing here needs a GPU, and nothing imports torch.  The edges (``K``) come from the library itself: rt_core.h's constants
through the host build (rt_hostcheck.cpp: hc_detect_order_constants, hc_key_tbits, hc_next_pow2)."""
import collections
import ctypes
import datetime
import functools
import math

import numpy as np

from oracle import analyze_oracle as oracle

FS = 2048000
WINDOW = "boxcar"
SIGMA = 1e-6                # noise: cells around -180 dBW
TONE_DBW = -79.0            # the quietest tone's cells
LEVEL_SPREAD_DB = 3.0       # every tone of a stream has its own level in [TONE_DBW, TONE_DBW + LEVEL_SPREAD_DB)
THRESHOLD_DBW = -125.0      # > 40 dB under the tones, > 40 dB over the noise
SNR_DB = 1.0
MAX_HOPS = 600.5            # the duration gate's upper end in STFT hops; the lower end: half a hop under the shortest plateau
PLATEAU_MIN = 8             # hot cells of the shortest plateau planted for a record: (8 + 1) hops against a gate of 7.5 (or of 1 ms)
BURST_MAX = 3               # hot cells of the longest burst: (3 + 1) hops, clear of it on the other side
DUTY = 8                    # a bin is hot in at most T / DUTY segments
NOISE_BLOCK = 1 << 20       # samples of noise generated; longer buffers repeat them
GOLDEN = 0.6180339887498949
TS0 = datetime.datetime(2024, 1, 1)

Tone = collections.namedtuple("Tone", "bin t0 r level_db")
Bucket = collections.namedtuple("Bucket", "fill plateaus head tail", defaults=(None, None, False, None))
Stream = collections.namedtuple("Stream", "tones fills plateaus")  # planned: cells and records of each of the 16 buckets
Case = collections.namedtuple("Case", "name family nperseg T streams kw expect min_ms rec_min")
Consts = collections.namedtuple("Consts", "buckets small_bucket group_cells group_bins quarters cand_cap_max")


# ---- the library's own edges -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _hostcheck():
    from pyradiotracking_amd import build

    lib = ctypes.CDLL(build.build_hostcheck())
    lib.hc_detect_order_constants.argtypes = [ctypes.c_void_p]
    lib.hc_detect_order_constants.restype = None
    return lib


@functools.lru_cache(maxsize=None)
def constants():
    out = np.zeros(6, np.int32)
    _hostcheck().hc_detect_order_constants(out.ctypes.data)
    return Consts(*(int(v) for v in out))


def key_tbits(n_seg):
    return int(_hostcheck().hc_key_tbits(int(n_seg)))


def next_pow2(v):
    return int(_hostcheck().hc_next_pow2(int(v)))


def _bits(n):
    b = 0
    while (1 << b) < n:
        b += 1
    return b


# ---- the three switches, restated ------------------------------------------------------------------------------------------------
def default_hot_cap(nperseg, max_seg):
    """rt_analyze.hip, rt_create (near line 1970): candidate cells per (stream, bucket) where rt_config.hot_capacity is 0."""
    K = constants()
    return min(8192, max(K.small_bucket, next_pow2(max(max_seg, 1)) * max(1, nperseg // 1024)))


def bucket_routine(nperseg, n_seg, n, hot_cap):
    """rt_kernels.h, detect_bucket_one (the switch near line 2900; the overflow and LARGE tests near line 2860): what orders a
    bucket list of ``n`` cells -> (routine, instantiation).  ``large``: the workgroup's bitonic sort in LDS over n2 cells."""
    K = constants()
    if n == 0:
        return None
    if n > hot_cap:
        return ("overflow", 0)
    n2 = 64
    while n2 < n:
        n2 <<= 1
    if n > K.small_bucket:
        assert n2 <= next_pow2(max(hot_cap, 64))  # (DetectArgs::lds_cells)
        return ("large", n2)
    hb = _bits(nperseg // K.buckets)
    tbits = key_tbits(n_seg)
    if hb + tbits <= 15 and n2 >= 128:
        return ("bitmap", n2 // 64)
    if hb + tbits + 10 <= 32:
        return ("packed", n2 // 64)
    return ("regs", n2 // 64)


def group_can(nperseg, max_seg):
    """rt_analyze.hip, rt_create (near line 1994): may the handle run detect_group at all?"""
    return nperseg <= constants().group_bins and _bits(nperseg) + key_tbits(max(max_seg, 1)) + 10 <= 32


def group_routine(nperseg, max_seg, n_seg, counts, hot_cap):
    """rt_kernels.h, detect_group (``whole`` near line 3070, the switch near line 3107) on a handle with RT_FLAG_GROUP_DETECT: the
    stream's 16 lists together -> [("group_packed", M)], or -- the stream goes to the work list, or the handle cannot group --
    the per-bucket routines of detect_bucket_one."""
    K = constants()
    total = int(sum(counts))
    if group_can(nperseg, max_seg) and total <= K.group_cells and all(c <= hot_cap for c in counts):
        if total == 0:
            return []
        n2 = 64
        while n2 < total:
            n2 <<= 1
        return [("group_packed", n2 // 64)]
    return [bucket_routine(nperseg, n_seg, int(c), hot_cap) for c in counts if c]


def f64_routine(n, hot_cap):
    """rt_f64_sparse.h, detect_sparse_f64 (near line 313): a map-free float64 handle sorts a stream's ONE list in LDS over the
    next power of two (the arrays hold next_pow2(hot_cap) = ``sort_cap`` cells)."""
    if n == 0:
        return None
    if n > hot_cap:
        return ("overflow", 0)
    M = next_pow2(n)
    assert M <= next_pow2(hot_cap)
    return ("f64_lds", M)


#: every routine x instantiation the switches can reach (the table of DESIGN section 4.3)
ALL_ROUTINES = ([("bitmap", m) for m in (2, 4, 8, 16)] + [("packed", m) for m in (1, 2, 4, 8, 16)] + [("regs", m) for m in (1, 2, 4, 8, 16)]
                + [("large", n2) for n2 in (2048, 4096, 8192)] + [("group_packed", m) for m in (1, 2, 4, 8, 16)]
                + [("f64_lds", m) for m in (1024, 2048)])


def sort_word(routine, nperseg, key, tbits, pos):
    """The 32-bit word a routine COMPARES for the cell ``key`` that stands at ``pos`` in the unordered list (rt_kernels.h:
    sort_bucket_packed, sort_group_packed: (bin, t) above a 10-bit position; the others: the key itself)."""
    key = np.asarray(key, np.uint64)
    if routine == "packed":
        hi = (key >> np.uint64(tbits)) // np.uint64(constants().buckets)
        return ((((hi << np.uint64(tbits)) | (key & np.uint64((1 << tbits) - 1))) << np.uint64(10)) | np.asarray(pos, np.uint64)) & np.uint64(0xFFFFFFFF)
    if routine == "group_packed":
        return ((key << np.uint64(10)) | np.asarray(pos, np.uint64)) & np.uint64(0xFFFFFFFF)
    return key


# ---- planting --------------------------------------------------------------------------------------------------------------------
def _pieces(b, T, rec_min, q_cells):
    """A bucket's fill as hot-cell counts: [(kind, r)], bursts first.  kind: burst | plateau | head (starts on segment 0) | end
    (runs through segment T - 1: listed, no record) | end-1 (through T - 2: a record that ends on the last segment).
    ``rec_min``: hot cells of the shortest plateau (a record), ``q_cells``: list cells of the longest."""
    left = b.fill if b.fill is not None else b.plateaus * (rec_min + 2)
    fill = left
    special = []
    n_rec = 0
    if b.tail:
        assert b.tail[0] == "end" or b.tail[1] >= rec_min
        special.append(b.tail)
        left -= b.tail[1] + 1
        n_rec += b.tail[0] == "end-1"
    if b.head:
        special.append(("head", rec_min + 4))
        left -= rec_min + 4
        n_rec += 1
    bursts = []
    if b.plateaus is None:
        if left >= rec_min + 6:
            bursts = [2, 1]
            left -= 5
        q_max = max(rec_min + 1, min(q_cells, T // DUTY - 2))
        p = -(-left // q_max)
    else:
        p = b.plateaus - n_rec
    out = [("burst", r) for r in bursts]
    if p:
        q, extra = divmod(left, p)
        assert q >= rec_min + 1, (b, T)
        out += [("plateau", q - 1 + (1 if i < extra else 0)) for i in range(p)]
    else:
        assert left == 0, (b, T)
    return out + special, fill, n_rec + p


def plan_stream(nperseg, T, buckets, first_level=0, rec_min=PLATEAU_MIN, q_cells=48, one_at_a_time=False):
    """``buckets``: {bucket: Bucket} -> Stream.  The pieces of a bucket go to its bins in turn (the head to the lowest, a tail to the
    highest, which is bin nperseg - 1 in bucket 15; where the bucket has bins to spare these two stay on their own); a bin's
    pieces are spread evenly over the buffer.  ``one_at_a_time``: the stream's tones one after the other instead, the buckets
    and bins taking turns -- no segment holds a tone and the cell before another bin's plateau, so that cell is noise that
    float32 transforms agree on (beside a tone 90 dB above it, it is the round-off of whichever transform computes it)."""
    K = constants()
    tones, fills, plateaus = [], [0] * K.buckets, [0] * K.buckets
    queues, lo_all, hi_all = [], 1, T - 2
    for bk in sorted(buckets):
        bins = [f for f in range(bk, nperseg, K.buckets) if f != 0]  # (bin 0: a constant, which the detrend removes)
        pieces, fills[bk], plateaus[bk] = _pieces(buckets[bk], T, rec_min, q_cells)
        per_bin = collections.defaultdict(list)
        head = tail = None
        for kind, r in pieces:
            if kind == "head":
                head = r
            elif kind in ("end", "end-1"):
                tail = (kind, r)
        free = bins[(1 if head is not None and len(bins) > 2 else 0):(len(bins) - 1 if tail is not None and len(bins) > 1 else len(bins))]
        step = 1 if len(free) <= 16 else len(free) // 8  # (many bins: pieces all over the bucket, both halves of the bin range)
        while math.gcd(step, len(free)) != 1:
            step += 1
        i = 0
        for kind, r in pieces:
            if kind in ("burst", "plateau"):
                per_bin[free[-1 - (i * step) % len(free)]].append(r)  # (from the top bin down: the list's last cell is a plateau's)
                i += 1
        for j, f in enumerate(bins):
            mine = per_bin.get(f, [])
            lo, hi = 1 + (3 * j) % 7, T - 2
            if f == bins[0] and head is not None:
                tones.append((f, 0, head))
                lo = head + 2
            if f == bins[-1] and tail is not None:
                t0 = T - tail[1] - (1 if tail[0] == "end-1" else 0)
                tones.append((f, t0, tail[1]))
                hi = t0 - 2
            hot = sum(mine) + (head or 0) * (f == bins[0]) + (tail[1] if tail and f == bins[-1] else 0)
            assert hot * DUTY <= T, (nperseg, T, bk, f, hot)
            if one_at_a_time:
                lo_all, hi_all = max(lo_all, lo if f == bins[0] and head is not None else 1), min(hi_all, hi)
                continue
            if not mine:
                continue
            need = sum(r + 2 for r in mine)
            assert lo + need <= hi, (nperseg, T, bk, f, need)
            gap = (hi - lo - need) // len(mine)
            t = lo
            for r in mine:
                tones.append((f, t, r))
                t += r + 2 + gap
        if one_at_a_time:
            queues.append([(f, r) for k in range(max(map(len, per_bin.values()), default=0)) for f, rs in sorted(per_bin.items(), reverse=True) if k < len(rs) for r in rs[k:k + 1]])
    if one_at_a_time:
        turn = [q[k] for k in range(max(map(len, queues), default=0)) for q in queues if k < len(q)]
        need = sum(r + 2 for _, r in turn)
        assert turn and lo_all + need <= hi_all, (nperseg, T, need)
        gap = (hi_all - lo_all - need) // len(turn)
        t = lo_all
        for f, r in turn:
            tones.append((f, t, r))
            t += r + 2 + gap
    out = [Tone(f, t0, r, TONE_DBW + LEVEL_SPREAD_DB * ((GOLDEN * (first_level + i + 1)) % 1.0)) for i, (f, t0, r) in enumerate(tones)]
    return Stream(tuple(out), tuple(fills), tuple(plateaus))


def split_total(total, nperseg):
    """A stream total dealt to its buckets (detect_group sees the sum): {bucket: Bucket}, every fill one or two plateaus."""
    K = constants()
    n_b = max(1, min(K.buckets - 1, total // 12))
    q, extra = divmod(total, n_b)
    return {K.buckets - 1 - i: Bucket(fill=q + (1 if i < extra else 0)) for i in range(n_b)}  # (from bucket 15 down: bucket 0 lacks bin 0)


def tone_amplitude(nperseg, level_db):
    """A bin-centred tone of this amplitude fills its cells with ``level_db`` (boxcar: |X|^2 = A^2 N^2, scale 1 / (fs N))."""
    return math.sqrt(10.0 ** (level_db / 10.0) * FS / nperseg)


def plant(nperseg, T, tones, seed):
    """complex64 [T * nperseg]: the tones over (repeated) noise."""
    n = T * nperseg
    rng = np.random.default_rng([2718, seed])
    blk = min(n, NOISE_BLOCK)
    z = (SIGMA * (rng.standard_normal(blk) + 1j * rng.standard_normal(blk))).astype(np.complex64)
    x = np.empty(n, np.complex64)
    for a in range(0, n, blk):
        x[a:a + blk] = z[:min(blk, n - a)]
    seg = x.reshape(T, nperseg)
    k = np.arange(nperseg)
    for f, t0, r, level in tones:
        seg[t0:t0 + r] += (tone_amplitude(nperseg, level) * np.exp(2j * np.pi * ((f * k) % nperseg) / nperseg)).astype(np.complex64)
    return x


# ---- the case table --------------------------------------------------------------------------------------------------------------
EDGE_FILLS = (64, 65, 128, 129, 256, 257, 512, 513, 1023, 1024)
BORDER_FILLS = (64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025)
GROUP_TOTALS = (64, 65, 128, 129, 256, 257, 512, 513, 896, 897)
PLATEAU_COUNTS = (32, 33, 64, 65, 129)


def _edges(fills, head=5, tail=None, tail_fill=100):
    b = {1 + i: Bucket(fill=f, head=(1 + i == head)) for i, f in enumerate(fills)}
    if tail:
        b[15] = Bucket(fill=tail_fill, tail=tail)
    return b


def _case(name, family, nperseg, T, bucket_maps, expect="records", min_ms=None, rec_min=PLATEAU_MIN, q_cells=48, one_at_a_time=False, **kw):
    streams, at = [], 0
    for m in bucket_maps:
        streams.append(plan_stream(nperseg, T, m, first_level=at, rec_min=rec_min, q_cells=q_cells, one_at_a_time=one_at_a_time))
        at += len(streams[-1].tones)
    kw.setdefault("mode", "sparse")
    return Case(name, family, nperseg, T, tuple(streams), tuple(sorted(kw.items())), expect, min_ms, rec_min)


def _table():
    K = constants()
    out = []
    # 1. the bitmap: hb + tbits = 15 at T = 2048, a power of two exactly; bin 255 with segment 2047 listed (every key bit set)
    out.append(_case("bitmap-256-T2048", "bitmap", 256, 2048, [_edges(EDGE_FILLS, tail=("end", 150), tail_fill=200)]))
    out.append(_case("bitmap-256-T2049", "bitmap", 256, 2049, [_edges(EDGE_FILLS, tail=("end", 150), tail_fill=200)]))  # tbits 12: packed
    out.append(_case("bitmap-32-T4400", "bitmap", 32, 4400, [_edges(EDGE_FILLS, tail=("end", 150), tail_fill=200)]))
    # 2. the packed network at every scan family; T just large enough for hb + tbits > 15, never a power of two
    for n, T in ((32, 16390), (64, 8200), (128, 4100), (1024, 600), (4096, 230), (8192, 230)):
        out.append(_case(f"packed-{n}-T{T}", "packed", n, T, [_edges(EDGE_FILLS, tail=("end-1", 20), tail_fill=60)]))
    # 3. the 2^26 border: the packed word uses all 32 bits / the first call that takes sort_bucket_regs
    for n in (256, 1024):
        for T in ((1 << 26) // n, (1 << 26) // n + 1):
            # (plateaus of 40 cells and more against a gate of 39.5 hops: the oracle probes every 39th segment of 2^26 / n; one tone at
            # a time: these cases' figures are held to the oracle's own float32 figures, 0.01 dB, where the others have the model's bounds)
            out.append(_case(f"border-{n}-T{T}", "border", n, T, [_edges(BORDER_FILLS, tail=("end-1", 60), tail_fill=160)], rec_min=40, q_cells=100, one_at_a_time=True))
    # 4. LARGE and the capacity edge
    out.append(_case("large-cap1500", "large", 256, 2048, [{3: Bucket(fill=1025), 7: Bucket(fill=1500, head=True), 12: Bucket(fill=300)}], hot_capacity=1500))
    out.append(_case("large-cap4096", "large", 256, 2400, [{2: Bucket(fill=2048), 6: Bucket(fill=2049), 9: Bucket(fill=4096), 15: Bucket(fill=64)}], hot_capacity=4096))
    out.append(_case("large-cap8192", "large", 256, 4200, [{4: Bucket(fill=4097), 11: Bucket(fill=8192)}], hot_capacity=8192))
    over = [{3: Bucket(fill=1025), 7: Bucket(fill=1501), 12: Bucket(fill=300)}]
    out.append(_case("large-cap1500-over-sparse", "large", 256, 2048, over, expect="overflow", hot_capacity=1500))
    out.append(_case("large-cap1500-over-auto", "large", 256, 2048, over, expect="fell_back", hot_capacity=1500, mode="auto"))
    # 5. detection by groups of lists (forced): stream totals up to kGroupCells by the group wave, one more by the work list
    assert GROUP_TOTALS[-2:] == (K.group_cells, K.group_cells + 1)
    for n in (32, 64, 128, 256):
        out.append(_case(f"group-{n}", "group", n, 700, [split_total(t, n) for t in GROUP_TOTALS], group_detect=True))
    out.append(_case("group-256-overflowed-bucket", "group", 256, 700, [{**split_total(100, 256), 3: Bucket(fill=129)}, split_total(200, 256)],
                     expect="fell_back", group_detect=True, hot_capacity=128, mode="auto"))
    for T in (16384, 16385):  # fbits + tbits + 10 == 32 with bin 255 through segment T - 2 listed; one more: the bucket waves, quietly
        out.append(_case(f"group-256-T{T}", "group", 256, T, [{**split_total(300, 256), 15: Bucket(fill=60, tail=("end-1", 30))}, split_total(K.group_cells, 256)],
                         group_detect=True))
    # 6. plateaus per bucket against the staging area (cand_cap 32 at nperseg 256, 64 at 1024)
    for n in (256, 1024):
        out.append(_case(f"plateaus-{n}", "plateaus", n, 700, [{1 + i: Bucket(plateaus=p) for i, p in enumerate(PLATEAU_COUNTS)}], min_ms=1.0, hot_capacity=2048))  # (129 plateaus: 1 290 cells)
    # 7. map-free float64: ONE list per stream, hot_capacity counts its cells
    f64 = dict(precision="float64", f64_sparse=True, mode="auto")
    out.append(_case("f64-cap1024", "f64", 256, 700, [split_total(1023, 256), split_total(1024, 256)], hot_capacity=1024, **f64))
    out.append(_case("f64-cap1024-over", "f64", 256, 700, [split_total(1025, 256), split_total(200, 256)], expect="overflow", hot_capacity=1024, **f64))
    out.append(_case("f64-cap1024-rescue", "f64", 256, 700, [split_total(1025, 256), split_total(200, 256)], expect="rescued", hot_capacity=1024, f64_rescue=True, **f64))
    out.append(_case("f64-cap1500", "f64", 256, 700, [split_total(1025, 256), split_total(1500, 256)], hot_capacity=1500, **f64))
    out.append(_case("f64-4096-top-bin", "f64", 4096, 230, [{15: Bucket(fill=60, tail=("end-1", 20)), 3: Bucket(fill=400), 9: Bucket(fill=240)}], hot_capacity=1024, **f64))
    return out


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
BIG = tuple(c.name for c in CASES if c.family == "border")  # the buffers of 2^26 samples


def kw_of(c):
    return dict(c.kw)


def is_f64(c):
    return kw_of(c).get("precision") == "float64"


def hop_ms(nperseg):
    return 1e3 * nperseg / FS


def settings(c):
    """The analysis keywords of the case (oracle and analyzer alike)."""
    return dict(sample_rate=FS, fft_nperseg=c.nperseg, fft_window=WINDOW, signal_threshold_dbw=THRESHOLD_DBW, snr_threshold_db=SNR_DB,
                signal_min_duration_ms=c.min_ms if c.min_ms is not None else (c.rec_min - 0.5) * hop_ms(c.nperseg),
                signal_max_duration_ms=MAX_HOPS * hop_ms(c.nperseg))


def handle_kwargs(c):
    """BatchSignalAnalyzer's keywords (without ``devices`` and ``sdr_callback_length``)."""
    kw = dict(settings(c), lanes=1, record_capacity=2048)
    kw.update(kw_of(c))
    return kw


def hot_cap(c):
    """Cells a list of the case's handle holds (a map-free float64 handle: per stream)."""
    cap = kw_of(c).get("hot_capacity", 0)
    return cap if cap else default_hot_cap(c.nperseg, c.T)


def buffer(c, s):
    """Stream s of the case: complex64 [T * nperseg] (a float64 handle widens it exactly)."""
    return plant(c.nperseg, c.T, c.streams[s].tones, seed=s)


def routines(c, fills):
    """[stream] -> the (routine, instantiation) pairs that order the stream's lists of ``fills[s]`` cells."""
    kw = kw_of(c)
    out = []
    for f in fills:
        if is_f64(c):
            r = f64_routine(int(sum(f)), hot_cap(c))
            out.append([r] if r else [])
        elif kw.get("group_detect"):
            out.append(group_routine(c.nperseg, c.T, c.T, f, hot_cap(c)))
        else:
            out.append([bucket_routine(c.nperseg, c.T, int(n), hot_cap(c)) for n in f if n])
    return out


# ---- the oracle's view of a case -------------------------------------------------------------------------------------------------
Analysis = collections.namedtuple("Analysis", "fills runs records shadowed cells row_means times loudest_cold_db quietest_hot_db snr_margin_db")


def analyse_stream(c, s):
    """Everything the tests need of stream s, from the oracle's own ``stft_power`` and the threshold: the length of each of the 16
    lists (hot cells and the cells directly before one), the records and shadow verdicts, the listed cells themselves (bins,
    segments, powers; time-major, the order a scan roughly emits in) and how far every decision is from its threshold."""
    K = constants()
    x = buffer(c, s)
    if is_f64(c):
        x = x.astype(np.complex128)
    kw = settings(c)
    p = oracle.ExtractParams(kw["signal_threshold_dbw"], kw["snr_threshold_db"], kw["signal_min_duration_ms"], kw["signal_max_duration_ms"])
    freqs, times, spec = oracle.stft_power(x, FS, WINDOW, c.nperseg)
    del x
    hot = spec >= p.signal_threshold
    listed = hot.copy()
    listed[:, :-1] |= hot[:, 1:]
    fills = tuple(int(listed[b::K.buckets].sum()) for b in range(K.buckets))
    records = oracle.extract_records(times, spec, None, p)
    signals = oracle.records_to_signals(records, freqs, TS0, str(s), 0)
    kept = {id(v) for v in oracle.filter_shadows(signals)}
    shadowed = [id(v) not in kept for v in signals]
    runs = [0] * K.buckets
    for r in records:
        runs[r.fi % K.buckets] += 1
    t_idx, f_idx = np.nonzero(listed.T)  # time-major
    vals = spec[f_idx, t_idx]
    means = spec.mean(axis=1)
    with np.errstate(divide="ignore"):
        loudest_cold = float(oracle.to_db(spec[~hot].max())) if (~hot).any() else -np.inf
        quietest_hot = float(oracle.to_db(spec[hot].min())) if hot.any() else np.inf
        ratio_db = oracle.to_db(spec[hot] / np.broadcast_to(means[:, None], spec.shape)[hot]) if hot.any() else np.array([np.inf])
    snr_margin = float(np.min(np.abs(ratio_db - kw["snr_threshold_db"])))
    return Analysis(fills, tuple(runs), records, shadowed, (f_idx.astype(np.int64), t_idx.astype(np.int64), vals), means, times, loudest_cold, quietest_hot,
                    snr_margin)


@functools.lru_cache(maxsize=64)
def _analyse_small(name, s):
    return analyse_stream(BY_NAME[name], s)


@functools.lru_cache(maxsize=1)
def _analyse_big(name, s):
    return analyse_stream(BY_NAME[name], s)


def analyse(c, s):
    """Cached (the contract's tests share it; of the 2^26 cases only the latest is kept)."""
    return (_analyse_big if c.name in BIG else _analyse_small)(c.name, s)


def rec_key(records):
    return [(int(r.fi), int(r.start), int(r.end)) for r in records]


# ---- a walker over the ordered list ----------------------------------------------------------------------------------------------
FAULTS = (None, "drop_last_of_full", "signed_compare", "tbits_short")


def order_list(c, routine, inst, keys, tbits, fault=None):
    """The list a routine hands detect_runs: ``keys`` (uint64 array, in emission order) padded with 0xFFFFFFFF to the routine's
    length, ordered by the word the routine compares, the first ``n`` taken.  -> indices into ``keys`` (-1: a padding word)."""
    n = len(keys)
    length = inst if routine in ("large", "f64_lds") else 64 * inst
    if fault == "drop_last_of_full" and n == length and routine not in ("large", "f64_lds"):
        keys = keys[:-1]  # the cell at position 64 M - 1 never arrives
    words = np.full(length, 0xFFFFFFFF, np.uint64)
    words[:len(keys)] = sort_word(routine, c.nperseg, keys, tbits, np.arange(len(keys)))
    idx = np.full(length, -1, np.int64)
    idx[:len(keys)] = np.arange(len(keys))
    cmp_ = words.astype(np.uint32).view(np.int32) if fault == "signed_compare" else words
    order = np.argsort(cmp_, kind="stable")
    return idx[order][:len(keys)]


def walk(c, s, fault=None):
    """The records of stream s from its ordered lists alone (no look-back: every case is one call): maximal runs of listed hot
    cells of one bin at consecutive segments, the duration gate on (cell before the run .. first cell after it), a run that
    reaches the last segment dropped (analyze.py:415-417).  Under a fault the lists are built as the faulty routine would."""
    K = constants()
    a = analyse(c, s)
    f_idx, t_idx, vals = a.cells
    kw = settings(c)
    p = oracle.ExtractParams(kw["signal_threshold_dbw"], kw["snr_threshold_db"], kw["signal_min_duration_ms"], kw["signal_max_duration_ms"])
    f64 = is_f64(c)
    tbits_true = 20 if f64 else key_tbits(c.T)  # (rt_core.h: kF64KeySegBits)
    tbits = tbits_true - 1 if fault == "tbits_short" else tbits_true
    keys_all = (f_idx.astype(np.uint64) << np.uint64(tbits)) | t_idx.astype(np.uint64)
    lists = []  # (routine, instantiation, member indices)
    per = routines(c, [a.fills])[0]
    assert ("overflow", 0) not in per, "an overflowing case has no lists to walk: the handle refuses the call or analyses it densely"
    if f64 or (per and per[0][0] == "group_packed"):
        if per:
            lists.append((per[0][0], per[0][1], np.arange(len(keys_all))))
    else:
        for b in range(K.buckets):
            members = np.flatnonzero(f_idx % K.buckets == b)
            r = bucket_routine(c.nperseg, c.T, len(members), hot_cap(c))
            if r and r[0] != "overflow":
                lists.append((r[0], r[1], members))
    out = []
    for routine, inst, members in lists:
        order = order_list(c, routine, inst, keys_all[members], tbits, fault)
        order = order[order >= 0]
        k = keys_all[members][order]
        v = vals[members][order]
        fi = (k >> np.uint64(tbits)).astype(np.int64)
        t = (k & np.uint64((1 << tbits) - 1)).astype(np.int64)
        ok = fi < c.nperseg
        above = np.zeros(len(k), bool)
        above[ok] = (v[ok] >= p.signal_threshold) & (v[ok] / a.row_means[fi[ok]] >= p.snr_threshold)
        i = 0
        while i < len(k):
            if not above[i]:
                i += 1
                continue
            j = i
            while j + 1 < len(k) and above[j + 1] and k[j + 1] == k[j] + np.uint64(1) and t[j] + 1 < c.T:
                j += 1
            b, e = int(t[i]), int(t[j]) + 1
            i = j + 1
            if e >= c.T:
                continue
            start = b - 1 if b > 0 else 0
            d = a.times[e] - a.times[start]
            if d < p.signal_min_duration or d > p.signal_max_duration:
                continue
            out.append((int(fi[j]), start, e))
    return sorted(out)
