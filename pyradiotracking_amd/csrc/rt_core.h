// rt_core.h -- scalar decision logic of the analysis path, shared by the HIP
// kernels (device) and by the host-side unit-test harness (rt_hostcheck.cpp).
//
// Everything here is a restatement of reference arithmetic that must be
// decided bit-identically on the GPU:
//   * segment-centre times            scipy/signal/_spectral_py.py:2136-2137
//   * the "above" predicate            radiotracking/analyze.py:370, 378 (T10)
//   * start-of-plateau walk incl. look-back into the previous buffer
//                                      analyze.py:382-398 (T11-T13)
//   * duration gate in float64         analyze.py:420-433 (T14)
//   * plateau statistics               analyze.py:442-447 (T15)
//   * timedelta microsecond rounding   CPython Modules/_datetimemodule.c
//                                      (delta_new / accum), used by the shadow
//                                      filter analyze.py:300-311 (T16)
// and the geometry a handle derives from its configuration on the host (look-back columns, chunk length, kernel family),
// RT_MODE_AUTO's choice of level from call to call (AutoPolicy),
// and the per-stream bookkeeping of a handle whose streams may sit out a call (rt_set_present: PresenceBook).
#ifndef RT_CORE_H
#define RT_CORE_H

#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <initializer_list>
#include <type_traits>
#include <utility>
#include <vector>

#if defined(__HIP__)  // HIP translation units only (hipcc also compiles the plain C++ ones)
#define RT_HD __host__ __device__ __forceinline__
#else
#define RT_HD inline
#endif

namespace rt {

// A complex value as two floats / two doubles: the element type of the kernels' tables and registers (arithmetic on them:
// rt_fft.h, rt_f64.h) and of the host's table builders (rt_tables.h).
struct cf {
    float x, y;
};
struct cd {
    double x, y;
};

// Geometry/thresholds of one detect pass (one spectrogram of T columns).  P is the power type of the map: float for
// the complex64 path, double for a float64 handle (rt_create_f64), whose thresholds are the reference's Python floats.
template <class P>
struct DetectParamsT {
    int32_t n_seg;        // T: columns of the current spectrogram
    int32_t n_seg_last;   // columns of the previous one, or -1 if there is none
    int32_t tail_cols;    // K: how many trailing columns of the previous one are readable
    int32_t stride;       // probe stride max(1, int(min_d / hop))         (analyze.py:354, 364)
    int32_t nperseg;      // N (for the time axis only)
    P thr;                // signal_threshold (linear)
    P snr;                // snr_threshold (linear)
    P cal_db;             // calibration (only to order maxima in the shadow filter)
    double fs;
    double min_d;         // seconds
    double max_d;         // seconds
};
using DetectParams = DetectParamsT<float>;
using DetectParams64 = DetectParamsT<double>;

// One stream's own detection settings (rt_set_stream_settings): what the reference fixes per SignalAnalyzer besides the
// absolute threshold (analyze.py:113-116).  `stride` is probe_stride of the stream's min_d, computed where the entry is built.
template <class P>
struct StreamSettingsT {
    double min_d;    // seconds
    double max_d;    // seconds
    P snr;           // snr_threshold (linear)
    int32_t stride;  // max(1, int(min_d / hop))
};
using StreamSettings = StreamSettingsT<float>;
using StreamSettings64 = StreamSettingsT<double>;
template <class P>
RT_HD void apply_stream_settings(DetectParamsT<P> &dp, const StreamSettingsT<P> &q) {
    dp.snr = q.snr;
    dp.min_d = q.min_d;
    dp.max_d = q.max_d;
    dp.stride = q.stride;
}
template <class T>
struct same_t {  // (keeps an argument out of template deduction: the power type comes from the parameters)
    using type = T;
};

// ---- RT_MODE_AUTO's levels (host-side bookkeeping of rt_analyze.hip; here so that the CPU suite can test it) ----
// Order: sparse < chunk-bit pre-filter (where the geometry allows it) < exact pre-filter (where its scratch exists) < dense.
// The mode numbers are rt_mode's (include/rt_analyze.h).
enum : int { kAutoAuto = 0, kAutoDense = 1, kAutoSparse = 2, kAutoPrefilter = 3, kAutoRunfilter = 4 };
struct AutoLevels {
    bool prefilter_ok;  // the chunk-bit pre-filter exists at this geometry
    bool runfilter_ok;  // the exact pre-filter exists (and its scratch is allocated)
};
RT_HD int level_rank(int mode) { return mode == kAutoSparse ? 0 : mode == kAutoPrefilter ? 1 : mode == kAutoRunfilter ? 2 : 3; }
RT_HD int level_up(AutoLevels a, int mode) {
    if (mode == kAutoSparse && a.prefilter_ok) return kAutoPrefilter;
    if (level_rank(mode) < 2 && a.runfilter_ok) return kAutoRunfilter;
    return kAutoDense;
}
RT_HD int level_down(AutoLevels a, int mode) {
    if (mode == kAutoDense && a.runfilter_ok) return kAutoRunfilter;
    if (level_rank(mode) > 1 && a.prefilter_ok) return kAutoPrefilter;
    return kAutoSparse;
}
// Is a probe of `target` (= level_down of the handle's level) pointless?  `abs_hot` = the most cells at or above the
// absolute threshold any stream had in the last call a pre-filter level analysed (valid: there was one):
//   * the sparse lists hold `list_cells` (16 buckets x hot_capacity) cells per stream -- more than that cannot fit;
//   * the chunk-bit level needs chunks of L cells that do NOT all pass the absolute threshold: with a share q of the cells
//     over it a chunk bit is set with probability q^L in each of nperseg bins (q = 3/4, L = 32, 256 bins: 2.6 % of the
//     chunks), beyond that every chunk is kept.
RT_HD bool probe_ruled_out(int target, int level, bool valid, uint64_t abs_hot, uint64_t list_cells, uint64_t cells_per_stream) {
    if (!valid || target == level) return false;
    if (target == kAutoSparse) return abs_hot > list_cells;
    if (target == kAutoPrefilter && level == kAutoRunfilter) return cells_per_stream > 0 && abs_hot * 4u > 3u * cells_per_stream;
    return false;
}

constexpr int kSlots = 2;        // calls a handle keeps in flight (rt_analyze.hip: one slot each)
constexpr int kMaxPartial = 32;  // AUTO: up to this many overflowing streams of a batch are re-run dense on their own

// What rt_fetch does with a call whose candidate lists overflowed (not rt_extract, not on the dense level): analyse it again on
// the same level with thresholds from its own row means, fail with RT_E_HOT_OVERFLOW, re-run the overflowing streams dense on
// their own, or re-run the whole call one level up (AutoPolicy::climb).
enum AutoOverflow : int { kOverflowOwnMeans = 0, kOverflowFail = 1, kOverflowPartialDense = 2, kOverflowLevelUp = 3 };
// `mode`: the level the call ran on; `thr_rerun`: it has been analysed on its own means already (once per call); `thr_stale`: its
// kFlagThrStale bit; `n_bad` of `n_streams` streams overflowed; `cfg_mode`: rt_config.mode.
//   * Stale: the per-bin thresholds of the exact pre-filter were too high for some streams (their noise floor fell from the buffer
//     before to this one) -- not a matter of capacity.  A few streams of many go dense on their own (AUTO); otherwise the call is
//     analysed again on the same level, its thresholds now taken from its own row means: the handle's level does not change, and
//     an explicit RT_MODE_RUNFILTER handle does not fail.
//   * Few: at most kMaxPartial streams and a quarter of the batch -- only they go dense, the handle stays on its level.  (Where a
//     pre-filter level is still ahead of the sparse one, the whole batch goes there first: its second pass costs less than the fixed
//     ~1 ms of a dense re-run of a few streams -- one workgroup per stream in detect_dense.)
inline AutoOverflow overflow_step(int mode, bool thr_rerun, bool thr_stale, int n_bad, int n_streams, int cfg_mode, AutoLevels lv) {
    const bool is_auto = cfg_mode == kAutoAuto;
    const bool stale = thr_stale && mode == kAutoRunfilter && !thr_rerun;
    const bool few = n_bad > 0 && n_bad <= kMaxPartial && 4 * n_bad <= n_streams && !(mode == kAutoSparse && level_up(lv, kAutoSparse) != kAutoDense);
    if (stale && !(is_auto && few)) return kOverflowOwnMeans;
    if (!is_auto) return kOverflowFail;
    return few ? kOverflowPartialDense : kOverflowLevelUp;
}

// RT_MODE_AUTO's state machine: the one place its rules live.  Three ways to analyse a buffer and a fourth between
// them, cheapest first -- RT_MODE_SPARSE (candidates emitted by the scan itself), RT_MODE_PREFILTER (two scan passes, rt_kernels.h;
// only where lv.prefilter_ok), RT_MODE_RUNFILTER (where lv.runfilter_ok), RT_MODE_DENSE.  A call whose candidate lists overflow is
// re-run one level up when it is fetched (overflow_step, climb); the handle then stays on that level for `dense_sticky` calls
// before it probes the level below again (a failed probe costs a wasted scan: the interval doubles, 16 .. 1024).  Plain integers
// in, plain integers out: rt_analyze.hip feeds it from a call's counters, the CPU suite from literal traces (hc_auto_*).
struct AutoPolicy {
    AutoLevels lv{false, false};
    int level = kAutoSparse;  // the level the input last needed
    int dense_sticky = 0;     // calls left on `level` before the next probe
    int sticky_len = 16;      // ... and how many there will be after the next climb
    // the most cells at or above the absolute threshold any stream had in the last call a pre-filter level analysed: more
    // than the sparse lists hold (kBuckets x hot_capacity per stream) means a probe of the sparse level cannot succeed
    uint32_t abs_hot_seen = 0;
    bool abs_hot_valid = false;

    // The mode a new call is enqueued with: the level the input last needed, for `dense_sticky` more calls; then a probe of the level
    // below.  `list_cells` = kBuckets x hot_capacity, `cells_per_stream` = T x N (probe_ruled_out).  A handle pinned to a mode runs it.
    int begin_call(int cfg_mode, uint64_t list_cells, uint64_t cells_per_stream) {
        if (cfg_mode != kAutoAuto) return cfg_mode;
        if (dense_sticky > 0) {
            --dense_sticky;
            return level;
        }
        int mode = level_down(lv, level);
        // (no probe, no back-off where the last count rules the level below out: the next call looks again)
        if (probe_ruled_out(mode, level, abs_hot_valid, abs_hot_seen, list_cells, cells_per_stream)) mode = level;
        // one probe at a time: the calls enqueued before this one's verdict is in (the caller may keep a slot's
        // worth of calls in flight) stay on the handle's level instead of each paying for a failed probe
        if (mode != level) dense_sticky = kSlots;
        return mode;
    }
    // What a call whose enqueue fails or that is rolled back puts back: taken before begin_call, nothing else of the policy has moved by then.
    int restore_point() const { return dense_sticky; }
    void restore(int point) { dense_sticky = point; }

    // A call that ran on `from` is analysed again one level up (returned), and the handle goes there.  It stays for a while; every
    // further failed probe doubles the while (a probe costs a wasted scan; `first`: a call that climbs two levels counts once).
    int climb(int from, bool first) {
        level = level_up(lv, from);
        if (first) back_off();
        return level;
    }

    // A call's analysis stands (every re-run is behind it): what it says about the handle's level.  `settled`: this call has been
    // here before (rt_fetch passes over a call twice: size query / peek, then delivery) -- the probe interval doubles once per call,
    // not once per pass.  `counts`: not an rt_extract, and it had segments.  `n_hot`: cells on the candidate lists; `seg_total`:
    // segments the exact pre-filter's second scan took (< 0: no such count); `n_took_part`: streams present.
    void settle(bool settled, int cfg_mode, int mode, bool fell_back, bool counts, int64_t n_hot, int64_t seg_total, int64_t n_took_part, int64_t n_seg,
                int64_t N) {
        if (settled || cfg_mode != kAutoAuto || !counts) return;
        // The exact pre-filter went through, but more than half of all segments held cells it has to keep: its second scan is then
        // most of a scan, and the dense path (one scan, 16 B per sample) is faster -- measured at the reference's default geometry
        // with the noise floor 2 dB over the threshold: 213 k against 241 k MS/s ...
        bool unselective = mode == kAutoRunfilter && seg_total >= 0 && seg_total * 2 > n_took_part * n_seg;
        // ... or a pre-filter level went through with more than 1/32 of all cells on its candidate lists (possible where
        // hot_capacity was raised: signals whose side lobes fill every bin put 9 % of the cells there, and ordering lists of
        // 16 k cells per bucket took 14 - 18 ms per call where the dense path takes 1.9)
        if ((mode == kAutoRunfilter || mode == kAutoPrefilter) && n_hot * 32 > n_took_part * n_seg * N) unselective = true;
        if (unselective) {
            // The handle moves up like after an overflow (without analysing this call again: its result stands) and probes this level later.
            level = level_up(lv, mode);
            back_off();
        } else if (!fell_back && level_rank(mode) < level_rank(level)) {
            // a probe of a lower level went through: the handle moves there (and from the pre-filter level it will
            // probe the plain sparse path after the usual interval)
            level = mode;
            sticky_len = 16;
            dense_sticky = (mode == kAutoSparse) ? 0 : 16;
        }
    }
    // ... and about the next probe: the count of a call that kept one (`abs_counted`) stands until a whole batch runs dense
    // (the dense path keeps no count: what was seen is history by the time it is left; a partial dense re-run leaves it alone).
    void keep_abs_hot(bool abs_counted, uint32_t abs_hot, int mode, int n_dense_streams) {
        if (abs_counted) {
            abs_hot_seen = abs_hot;
            abs_hot_valid = true;
        } else if (mode == kAutoDense && n_dense_streams == 0) {
            abs_hot_valid = false;
        }
    }

private:
    void back_off() {
        dense_sticky = sticky_len;
        sticky_len = std::min(sticky_len * 2, 1024);
    }
};

// Chunks per "quiet level" sample of the exact pre-filter's per-bin thresholds (make_bin_thresholds): the quietest sum
// over `g` consecutive complete chunks of a workgroup's item, g the smallest power of two with g * L >= 32 segments (at
// most the item's gpw chunks) -- a small batch runs chunks of 4 segments, and the minimum over hundreds of 4-segment
// sums of exponentially distributed noise lies at a tenth of the mean, where the minimum over 32-segment sums lies at 0.55.
RT_HD int minsum_group(int L, int gpw) {
    int g = 1;
    while (g * L < 32 && g * 2 <= gpw) g *= 2;
    return g;
}

// Sampling of the absolute-threshold bits in the threshold-bit scan's items that need them only for AUTO's count (stft_scan, MODE 6
// with staged per-bin thresholds: abs_hot).  One step in P = abs_sample_period(L) builds them, P the largest power of two <= min(8, L)
// -- with chunks of 4 .. 7 segments (small batches) a fixed period of eight never sampled anything -- and a sampled cell counts P
// times.  Steps run i = 1 .. L in every chunk, so the phase must come from outside the chunk: `phase` = the item's number within
// its stream + the wave's number (uniform per wave), which turns from item to item whatever L is -- a pulse train whose period is
// a multiple of eight hops can neither hide from the count nor fill it.
RT_HD int abs_sample_period(int L) {
    int p = 1;
    while (p * 2 <= L && p < 8) p *= 2;
    return p;
}
RT_HD bool abs_sampled(int i, int phase, int period) { return ((i + phase) & (period - 1)) == 0; }

// Factor on the quiet-level estimate when its samples are longer than 32 segments (chunks of 37 .. 71 segments at nperseg >= 1024).
// The minimum over n samples of the mean of m exponentially distributed powers lies about 2 / sqrt(m) under the mean; the
// thresholds must stay under snr x the NEXT buffer's row mean, and with long samples (few of them, each close to the mean) that
// margin shrinks: 14 % at m = 128, where one bin in fifty failed the check in an experiment.  The factor puts every sample
// length on the footing of m = 32 (0.55 - 0.65 x the mean, measured safe).
RT_HD float minsum_margin(int m) {
    if (m <= 32) return 1.0f;
    return (1.0f - 2.0f / sqrtf(32.0f)) / (1.0f - 2.0f / sqrtf((float)m));
}

// times[k] of scipy: arange(N/2, B - N/2 + 1, N) / float(fs)
RT_HD double seg_time(int32_t k, int32_t nperseg, double fs) {
    return ((double)nperseg * 0.5 + (double)k * (double)nperseg) / fs;
}

// stride = max(1, int(min_d / (times[1] - times[0])))
RT_HD int32_t probe_stride(int32_t nperseg, double fs, double min_d) {
    double hop = seg_time(1, nperseg, fs) - seg_time(0, nperseg, fs);
    double q = min_d / hop;
    int32_t s = (q >= 2147483647.0) ? 2147483647 : (int32_t)q;  // int() truncates toward zero
    return s < 1 ? 1 : s;
}

// ---- Geometry of a handle (host side of rt_analyze.hip; here so that the CPU suite can test it: tests/test_host_tables.py) ----

// K: the trailing columns of the previous buffer's map a look-back can reach -- floor(max duration / hop) + 2, at most 1e6
inline int tail_cols(int nperseg, double fs, double max_d) {
    const double hop = seg_time(1, nperseg, fs) - seg_time(0, nperseg, fs);
    const double k = std::floor(max_d / hop) + 2.0;
    const int K = (int)std::min(k, 1.0e6);
    return K < 1 ? 1 : K;
}

// cells a run must have to pass the duration gate unless it runs through t = 0: (len + 1) * hop < signal_min_duration fails
// the gate (analyze.py:427-430; gate_run below), with a margin of 1e-9 for the rounding of the float64 expressions
inline long long min_run_cells(int N, double fs, double min_d) {
    const double hop = seg_time(1, N, fs) - seg_time(0, N, fs);
    const double cells = min_d * (1.0 - 1e-9) / hop;
    return (long long)std::ceil(std::min(cells, 1.0e9)) - 1;
}

inline int next_pow2(int v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

// bits of the segment index in a 32-bit cell key
inline int key_tbits(int n_seg) {
    int t = 1;
    while ((1ll << t) < (long long)n_seg) ++t;
    return t;
}

// The size edges of the sparse detection (rt_kernels.h: detect_bucket_one, detect_group, detect_runs).  They stand here, beside
// key_tbits, so that the host build (rt_hostcheck.cpp: hc_detect_order_constants) hands them to tests/detect_order_cases.py, which
// restates the choice of ordering routine from them.
constexpr int kBuckets = 16;  // candidate lists per stream: bucket = bin & 15 (a bin never spans buckets).
                              // 64 was measured: detect -6 %, but the scan +2 % (N=256) .. +8 % (N=1024)
constexpr int kSmallBucket = 1024;  // buckets up to this many cells use the small-LDS instantiation
constexpr int kQuarters = 4;        // detect_group: a wave takes a stream's buckets all together or a quarter of them
constexpr int kCandCapMax = 64;     // plateaus a bucket wave stages in LDS before it finishes them (a.cand_cap <= this); no limit per bucket
constexpr int kGroupCells = 896;    // detect_group: cells of a whole stream one wave takes
constexpr int kGroupBins = 256;     // (kSmallBucket - kGroupCells) * 8 / 4: the group's row means lie behind its cells

// Which kernel family an nperseg runs on:
//   256 r, r in {1, 2, 4, 8, 16}   the fused scans (rt_kernels.h: stft_scan<R3 = r>; 4096: rt_scan64.h), lane groups of 16 r lanes
//   16 q, q in {2, 4, 8}           the fused scans with lane groups of q lanes (stft_scan<1, .., QS = q>)
//   8192, 16 384                   one workgroup per segment (rt_scan_wg.h: stft_wg), `big` = its threads (nperseg / 32); sparse and dense path
//   every other size the reference may be given (it passes any integer on to SciPy): the other powers of two from 8 to 16 384 by a
//   general LDS transform, everything else from 8 to 8 192 by Bluestein's algorithm on it -- both on the dense path (rt_general.h)
// R3 = 1 in the last two (it sizes scratch nobody uses there).
constexpr int kGeneralMaxN = 16384;  // the general transform's longest segment: 128 KiB of LDS
struct ScanFamily {
    int R3 = 0, QS = 0, big = 0;
    bool general = false, bluestein = false;
    bool supported = false;
};
inline ScanFamily scan_family(int nperseg) {
    ScanFamily f;
    for (int r : {1, 2, 4, 8, 16})
        if (nperseg == 256 * r) f.R3 = r;
    for (int q : {2, 4, 8})
        if (nperseg == 16 * q) {
            f.R3 = 1;
            f.QS = q;
        }
    if (nperseg == 8192 || nperseg == 16384) {
        f.R3 = 1;
        f.big = nperseg / 32;  // (rt_scan_wg.h: wg_block)
    }
    f.supported = true;
    if (!f.R3) {
        const int n = nperseg;
        const bool pow2 = n > 0 && (n & (n - 1)) == 0;
        f.supported = !(n < 8 || (pow2 && n > kGeneralMaxN) || (!pow2 && n > kGeneralMaxN / 2));
        f.general = true;
        f.bluestein = !pow2;
        f.R3 = 1;
    }
    return f;
}

// Segments per chunk for a handle of `n_streams` streams whose buffers hold up to `n_seg` segments; `block` = threads of a scan
// workgroup (rt_kernels.h: scan_block(R3)), `segs_per_chunk` > 0 forces the length (rt_config.segs_per_chunk).  The chunk length
// sets the order in which a row's partial sums are added, so every part of one population must run with the same one: a laned
// handle asks with the number of streams of all lanes together and hands the answer to its lanes as a forced length.  The choice
// does depend on that number, in two places: the halving for batches too small to fill the chip (`blocks >= 2048`, and stft_wg's
// `8 * 512`), and the "at least eight rounds" cut-off of the nperseg >= 1024 search -- shards of one population that are to add
// their row sums in the same order must pass the whole population's count (or force the length), as the lanes do.
inline int choose_chunk(int nperseg, int R3, int QS, int block, double fs, double min_duration_s, int segs_per_chunk, int n_streams, int n_seg) {
    if (segs_per_chunk > 0) return segs_per_chunk;
    if (nperseg >= 8192) {
        // stft_wg: one chunk per workgroup, 512 workgroup slots on the chip (two per CU at 8192; 256 at 16 384).  A workgroup pays
        // ~2 steps on top of its L (tables, the first segment's round trip with nothing to overlap it, the row sums' stores): chunks of
        // about 40 segments where the batch fills the chip eight times over, shorter ones -- down to 8 -- for small batches; then the
        // length that leaves no short last chunk.
        int L = 40;
        while (L > 8 && (int64_t)n_streams * ((n_seg + L - 1) / L) < 8 * 512) L -= 8;
        const int chunks = std::max(1, (n_seg + L - 1) / L);
        return std::max(1, (n_seg + chunks - 1) / chunks);
    }
    const int N = QS ? 16 * QS : 256 * R3, GPW = block / (QS ? QS : 16 * R3);
    // enough workgroups to fill 256 CUs several times over, halo overhead <= 1/L
    int L = 32;
    // ... but where the run-length pre-filter is possible with chunks of 32 (minimum duration >= 64 hops) the chunks
    // stay that long for small batches too: its selectivity is p^L (a small batch is launch-bound anyway)
    // (whatever the mode: the chunk length sets the order of the row sums' partial sums, and the modes return the same bits)
    const bool keep_long = 2ll * L - 1 <= min_run_cells(N, fs, min_duration_s) && n_seg >= 2 * L;
    while (L > 4 && !keep_long) {
        const int64_t chunks = (n_seg + L - 1) / L;
        const int64_t blocks = (int64_t)n_streams * ((chunks + GPW - 1) / GPW);
        if (blocks >= 2048) break;
        L >>= 1;
    }
    if (L == 32 && R3 < 4 && n_seg > 32 && !keep_long) {
        // nperseg <= 512, a batch that fills the chip, no chunk bits to serve: a workgroup holds GPW chunks and its lane groups walk in
        // step, so a stream costs (workgroups) x L steps whatever its last workgroup holds -- 1 171 segments (the reference's default
        // geometry) are 37 chunks of 32 in three workgroups of 16, eleven lane groups idle, or 47 chunks of 25 in the same three, one
        // idle: 22 % fewer steps (551 -> 636 k MS/s).  Among the lengths 20 .. 32 the one with the fewest steps, a step of overhead per
        // workgroup, and 2 % against multiples of eight (a wave's four lane groups read four chunks L x 2 KiB apart: 32- and 64-KiB
        // strides are the slowest per step in every sweep).  (The search itself does not read the number of streams; whether it runs
        // does: only a batch that kept L = 32 through the halving above gets here.)
        // Where the chunk bits exist (config 2 / 4 geometry) the chunks stay 32 long: at config 2 a length of 25 (20 full workgroups
        // per stream instead of 15.6) makes the scan alone 1.5 - 5.5 % faster on four boxes and the uint8 path 2 %, the whole path with
        // two lanes the same, and the chunk-bit and exact pre-filter levels 2 - 7 % slower (shorter chunks are less selective, more
        // workgroups in the second scan); config 4 (2 048 segments = four full workgroups) is fastest at 32 anyway --
        // profiles/r04_q_chunk_length_sweep_nperseg256.txt.
        double best = 0.0;
        for (int cand = 20; cand <= 32; ++cand) {
            const int64_t chunks = (n_seg + cand - 1) / cand;
            const int64_t wgs = (chunks + GPW - 1) / GPW;
            const double cost = (double)wgs * (cand + 1.0) * (cand % 8 == 0 ? 1.02 : 1.0);
            if (best == 0.0 || cost < best * (1.0 - 1e-9)) {
                best = cost;
                L = cand;
            }
        }
    }
    if (L == 32 && !keep_long && R3 >= 4) {
        // nperseg >= 1024, a batch that fills the chip: the chunk length is chosen by what a workgroup costs.  All lane
        // groups of a workgroup take L steps (a last chunk that is short leaves its group idle), and a workgroup pays
        // c0 steps on top: tables into LDS, the first segment's HBM round trip with nothing to overlap it, the halo
        // step (nperseg 4096), the row-sum epilogue.  Measured (profiles/r03_a_chunk_length_sweep.txt, one lane):
        // nperseg 4096, 781 segments: L = 32 -> 71 (11 chunks, none short) takes 5.8 - 6.7 % less time at 1 024 and at
        // 4 096 streams, L = 52 (a last chunk of one segment) 1.6 % more; that fits c0 = 3.8.  nperseg 1024, 2 343 segments,
        // four chunks to a workgroup: L = 28 / 31 (84 / 76 chunks: 21 / 19 full workgroups) take 4 % less than 32 (19
        // workgroups, three chunk slots idle), 36 and 64 more: c0 = 2.  (The cost has no term for the end of the launch, so that
        // the winner does not move with the number of streams; the cut-off below does read it.)
        // nperseg 2048 (no halo step: c0 = 2.8; 512 streams x 1 000 segments): L = 72 (7 workgroups per stream) 2 % less
        // than 32, but 48 / 62 / 77 take 4 - 13 % more -- with 3 584 workgroups the launch is under five rounds of the
        // chip's 768 slots and its last round counts: the search keeps at least eight rounds.
        const double c0 = R3 >= 16 ? 3.8 : R3 >= 8 ? 2.8 : 2.0;
        const int lo = 24, hi = R3 >= 8 ? 80 : 40;
        double best = 0.0;
        for (int cand = lo; cand <= hi; ++cand) {
            const int64_t chunks = (n_seg + cand - 1) / cand;
            const int64_t wgs = (chunks + GPW - 1) / GPW;
            if ((int64_t)n_streams * wgs < 8 * 768) break;  // (nothing qualifies: L stays 32)
            const double cost = (double)wgs * (cand + c0);
            if (best == 0.0 || cost < best * (1.0 - 1e-9)) {
                best = cost;
                L = cand;
            }
        }
    }
    return L;
}

// ---- The map-free float64 path (RT_FLAG_F64_SPARSE; kernels: rt_f64_sparse.h; host side here so that the CPU suite can test it) ----
// A candidate cell's key: the bin above the segment, so that the unsigned order of the keys is the (bin, segment) order the
// detection sorts by.  20 bits of segment: a handle's max_samples / nperseg may not exceed kF64KeyMaxSeg; 12 bits of bin: nperseg
// up to 4096.
constexpr int kF64KeySegBits = 20;
constexpr int kF64KeyMaxSeg = 1 << kF64KeySegBits;
constexpr int kF64SparseMinN = 32, kF64SparseMaxN = 4096;
constexpr int kF64ScanBlock = 256;  // threads of a scan_f64 workgroup
RT_HD uint32_t f64_cell_key(int32_t fi, int32_t t) { return ((uint32_t)fi << kF64KeySegBits) | (uint32_t)t; }
RT_HD int32_t f64_key_bin(uint32_t key) { return (int32_t)(key >> kF64KeySegBits); }
RT_HD int32_t f64_key_seg(uint32_t key) { return (int32_t)(key & (uint32_t)(kF64KeyMaxSeg - 1)); }
inline bool f64_sparse_nperseg_ok(int n) { return n >= kF64SparseMinN && n <= kF64SparseMaxN && (n & (n - 1)) == 0; }
// rt_config.hot_capacity on such a handle: candidate cells per stream and call, what one workgroup sorts in LDS (12 bytes a cell:
// 8192 cells = 96 KiB).  0 = the default, 4096 (a full column of NaN cells at nperseg 2048 with its predecessor column; 48 KiB of
// LDS, so that three streams' detections share a CU); out of range: -1 (RT_E_INVALID).
constexpr int kF64HotMin = 1024, kF64HotMax = 8192, kF64HotDefault = 4096;
inline int f64_sparse_hot_capacity(int hot_capacity) {
    if (hot_capacity == 0) return kF64HotDefault;
    return (hot_capacity < kF64HotMin || hot_capacity > kF64HotMax) ? -1 : hot_capacity;
}
// Segments a scan_f64 workgroup transforms side by side: 1024 samples' worth, at most 32 (nperseg 32: 8 threads a segment)
inline int f64_sparse_group(int nperseg) { return std::max(1, std::min(32, 1024 / nperseg)); }
// Segments per chunk (L): rt_config.segs_per_chunk where set.  Else L + 1 (the chunk and its halo segment) is a whole number of
// groups -- 32 segments or eight groups, whichever is more, so the halo costs 3 % at most -- halved while the handle's largest call
// has fewer than 2048 workgroups.  L is fixed when the handle is made (from max_samples), not per call: it sets the order in which
// a row's partial sums are added.
inline int f64_sparse_chunk(int nperseg, int segs_per_chunk, int n_streams, int max_seg) {
    if (segs_per_chunk > 0) return segs_per_chunk;
    const int g = f64_sparse_group(nperseg);
    int l1 = std::max(32, 8 * g);
    while (l1 > std::max(4, g) && (int64_t)n_streams * ((max_seg + l1 - 2) / (l1 - 1)) < 2048) l1 >>= 1;
    return l1 - 1;
}
inline int f64_sparse_chunks(int n_seg, int L) { return n_seg <= 0 ? 0 : (n_seg + L - 1) / L; }
inline int f64_sparse_last_chunk(int n_seg, int L) { return n_seg <= 0 ? 0 : n_seg - (f64_sparse_chunks(n_seg, L) - 1) * L; }
// RT_FLAG_F64_RESCUE: the streams of a call whose lists overflowed are analysed again from a float64 map [slot][T][N] in a
// scratch area of kF64RescueBudget bytes -- or one stream's map where that is larger --, as many streams a round as fit.
constexpr int64_t kF64RescueBudget = 256ll << 20;
struct F64RescueRounds {
    int32_t per_round;  // streams a round takes at most (the last round: what is left)
    int32_t rounds;
};
inline F64RescueRounds f64_rescue_rounds(int n_bad, int n_seg, int nperseg, int64_t budget) {
    if (n_bad <= 0) return F64RescueRounds{0, 0};
    const int64_t one = std::max<int64_t>(8, (int64_t)n_seg * nperseg * 8);
    const int64_t fit = std::min<int64_t>(n_bad, std::max<int64_t>(1, budget / one));
    return F64RescueRounds{(int32_t)fit, (int32_t)((n_bad + fit - 1) / fit)};
}

// ---- Streams that sit out a call (rt_set_present; host side of rt_analyze.hip, here so that the CPU suite can drive it) ----
// In the reference every SDR is a SignalAnalyzer of its own: `_spectrogram_last` is the buffer ITS radio delivered before, whatever
// the other radios did meanwhile.  A handle keeps three look-back tails in rotation for all streams in lock-step (call k reads
// buffer tail_cur and writes the next one), so a stream that is absent from a call has its K columns CARRIED from the buffer the
// call reads to the one it writes (rt_present.h: carry_tails) -- after any number of absent calls the buffer the next call reads
// holds the columns of the stream's last present buffer -- and what the rotation cannot carry is kept here, per stream:
//   * the segment count of the stream's own previous buffer (`start_min`, analyze.py:383: -1 = none);
//   * its pending reset (rt_reset_stream, a changed threshold or setting): taken by its next PRESENT call;
//   * per call, in the call's slot, the snapshot every re-analysis of that call inside rt_fetch uses again (PresenceCall).
constexpr int kTailBuffers = 3;
struct PresenceCall {
    int n_present = 0;
    int tail_read = 0, tail_write = 0;  // the rotation's buffers this call reads / writes (absent streams: carried read -> write)
    std::vector<uint8_t> absent;        // [S] 1 = the stream sits this call out
    std::vector<int32_t> n_seg_last;    // [S] present: columns of its own previous buffer as this call sees it (-1: none, or its
                                        //     reset was taken); absent: what it keeps for its next present call
    std::vector<int32_t> before;        // [S] the book's count before the call      } put back when the call is rolled back
    std::vector<uint8_t> took_reset;    // [S] the call consumed the stream's reset  }
};
struct PresenceBook {
    int S = 0;
    bool active = false;               // rt_set_present has been called on the handle (it then stays on the per-stream path)
    std::vector<uint8_t> present;      // [S] the mask in force, 1 = present (sticky)
    std::vector<int32_t> n_seg_last;   // [S] columns of each stream's own latest present buffer, -1: none
    // first use: every stream inherits the handle's one count (`all` = -1: no buffer yet)
    void activate(int n_streams, int all) {
        S = n_streams;
        active = true;
        present.assign((size_t)S, (uint8_t)1);
        n_seg_last.assign((size_t)S, (int32_t)all);
    }
    // `mask` = null: every stream.  Returns whether the mask in force changed.
    bool set_mask(const uint8_t *mask) {
        bool changed = false;
        for (int s = 0; s < S; ++s) {
            const uint8_t v = (!mask || mask[s]) ? 1 : 0;
            changed = changed || v != present[(size_t)s];
            present[(size_t)s] = v;
        }
        return changed;
    }
    void forget_all() { std::fill(n_seg_last.begin(), n_seg_last.end(), (int32_t)-1); }  // rt_reset
    // A call of T segments is enqueued with the mask in force; `tail_cur` = the rotation's buffer the call before wrote.
    void begin_call(int T, int tail_cur, std::vector<uint8_t> &reset_pending, PresenceCall &c) {
        c.n_present = 0;
        c.tail_read = tail_cur;
        c.tail_write = (tail_cur + 1) % kTailBuffers;
        c.absent.assign((size_t)S, (uint8_t)0);
        c.n_seg_last.assign((size_t)S, (int32_t)-1);
        c.before = n_seg_last;
        c.took_reset.assign((size_t)S, (uint8_t)0);
        for (int s = 0; s < S; ++s) {
            const size_t i = (size_t)s;
            if (!present[i]) {
                c.absent[i] = 1;
                c.n_seg_last[i] = n_seg_last[i];  // state as if no call happened; a pending reset stays pending
                continue;
            }
            ++c.n_present;
            c.took_reset[i] = reset_pending[i];
            c.n_seg_last[i] = reset_pending[i] ? -1 : n_seg_last[i];
            reset_pending[i] = 0;
            n_seg_last[i] = T;
        }
    }
    // The newest call is undone (it failed to enqueue, or a later lane did): counts and resets as before it.
    void rollback(const PresenceCall &c, std::vector<uint8_t> &reset_pending) {
        n_seg_last = c.before;
        for (int s = 0; s < S; ++s)
            if (c.took_reset[(size_t)s]) reset_pending[(size_t)s] = 1;
    }
};

// ---- Consecutive buffers of one recording as the streams of one call (rt_set_chain; host side, driven by the CPU suite) ----
// The handle's streams are grouped into runs of `links` consecutive indices; the present streams of a run are, in index order,
// consecutive buffers of ONE analyzer of the reference.  So the buffer at stream s looks back into the nearest present stream
// before it in its run, of the SAME call (whose columns the call's own scan writes into the rotation buffer the call writes);
// a run's first present stream looks back into the run's last present stream of the latest earlier call the run took part in
// -- carried along the rotation since (PresenceBook), so it is in the buffer the call reads -- with THAT call's segment count.
// The book sits on top of a PresenceBook (the mask, the pending resets, the rotation): begin_call rewrites the n_seg_last row of
// the PresenceCall the presence book has just filled and yields each stream's source for the copy (rt_chain.h: chain_tails).
enum : int32_t { kChainNone = 0, kChainWritten = 1, kChainRead = 2 };  // ChainCall::src_buf: no copy / the buffer the call writes / reads
struct ChainCall {
    std::vector<int32_t> src_buf;   // [S] kChain*: absent streams and streams without look-back take none
    std::vector<int32_t> src_idx;   // [S] the stream whose columns are copied (-1: none)
    std::vector<int32_t> before_idx, before_T;  // [runs] the book before the call (put back when the call is rolled back)
};
struct ChainBook {
    int S = 0, links = 0;             // links >= 2: chaining is on
    std::vector<int32_t> last_idx;    // [runs] the run's last present stream of the latest call it took part in, -1: none
    std::vector<int32_t> last_T;      // [runs] ... and that call's segment count
    bool on() const { return links >= 2; }
    int runs() const { return on() ? S / links : 0; }
    void configure(int n_streams, int n_links) {
        S = n_streams;
        links = n_links >= 2 ? n_links : 0;
        last_idx.assign((size_t)runs(), (int32_t)-1);
        last_T.assign((size_t)runs(), (int32_t)-1);
    }
    void forget_all() {  // rt_reset: a cut in front of every run's first stream
        std::fill(last_idx.begin(), last_idx.end(), (int32_t)-1);
        std::fill(last_T.begin(), last_T.end(), (int32_t)-1);
    }
    // `pc`: the call's snapshot as PresenceBook::begin_call left it (absent, took_reset; n_seg_last per stream INDEX, which is
    // replaced here for the present streams by the count of the buffer each one follows, -1: none).
    void begin_call(int T, PresenceCall &pc, ChainCall &cc) {
        cc.src_buf.assign((size_t)S, (int32_t)kChainNone);
        cc.src_idx.assign((size_t)S, (int32_t)-1);
        cc.before_idx = last_idx;
        cc.before_T = last_T;
        for (int r = 0; r < runs(); ++r) {
            int pred = -1;  // the nearest present stream before s in the run, in this call
            for (int s = r * links; s < (r + 1) * links; ++s) {
                const size_t i = (size_t)s;
                if (pc.absent[i]) continue;
                if (pc.took_reset[i]) {
                    pc.n_seg_last[i] = -1;
                } else if (pred >= 0) {
                    cc.src_buf[i] = kChainWritten;
                    cc.src_idx[i] = pred;
                    pc.n_seg_last[i] = T;
                } else if (last_idx[(size_t)r] >= 0) {
                    cc.src_buf[i] = kChainRead;
                    cc.src_idx[i] = last_idx[(size_t)r];
                    pc.n_seg_last[i] = last_T[(size_t)r];
                } else {
                    pc.n_seg_last[i] = -1;
                }
                pred = s;
            }
            if (pred >= 0) {
                last_idx[(size_t)r] = pred;
                last_T[(size_t)r] = T;
            }
        }
    }
    void rollback(const ChainCall &cc) {
        last_idx = cc.before_idx;
        last_T = cc.before_T;
    }
    // the first run whose streams do not all hold the same value of `v` ([S]), or -1
    template <class V>
    int first_mixed_run(const V *v) const {
        for (int r = 0; r < runs(); ++r)
            for (int j = 1; j < links; ++j)
                if (!(v[r * links + j] == v[r * links])) return r;
        return -1;
    }
};

// Column rotation of exchange 1 in the fused scans with R3 > 1 (rt_kernels.h: "Exchange layouts"): s1(b) = (16 / R3 - 2) * b mod 16.
// The kernel rotates by it; the host folds the phase that undoes it into the pass-2 twiddles (rt_tables.h: scan_twiddles).
RT_HD int x1_rotation(int R3, int b) { return ((16 / R3 - 2) * b) & 15; }

// `not (p < thr) and not (p / avg < snr)` in float32
RT_HD bool cell_above(float p, float avg, float thr, float snr) {
    if (p < thr) return false;
    if (p / avg < snr) return false;
    return true;
}
// ... and in float64 (a float64 handle: the reference's comparisons on complex128 input)
RT_HD bool cell_above(double p, double avg, double thr, double snr) {
    if (p < thr) return false;
    if (p / avg < snr) return false;
    return true;
}

// A maximal run [b, e) of above-cells is visited by the strided probe iff it
// contains a multiple of the stride (T9).  Returns that first probe or -1.
RT_HD int32_t first_probe_in_run(int32_t b, int32_t e, int32_t stride) {
    int32_t q = (b + stride - 1) / stride;
    int64_t ti = (int64_t)q * stride;
    return ti < e ? (int32_t)ti : -1;
}

// Outcome of the downward walk (analyze.py:382-398).
struct StartWalk {
    int32_t start;   // may be negative
    bool too_long;   // ran past the readable tail: duration certainly exceeds max_d
};

// `prev(d)` returns the power of the previous buffer's column n_seg_last-d
// (d >= 1, d <= tail_cols) for the bin at hand.
template <class P, class PrevCell>
RT_HD StartWalk walk_start(const DetectParamsT<P> &p, int32_t b, int32_t ti0, typename same_t<P>::type avg, PrevCell prev) {
    StartWalk w;
    w.too_long = false;
    const int32_t start_min = (p.n_seg_last < 0) ? 0 : (1 - p.n_seg_last);
    if (ti0 <= start_min) {  // loop `while start > start_min` never runs
        w.start = ti0;
        return w;
    }
    // cells b..ti0 are above; b-1 (if >= 0) is not: the walk stops on it, or
    // earlier on start_min without testing (T11).
    int32_t s = b - 1;
    if (s < start_min) s = start_min;
    if (s >= 0 || b > 0) {
        w.start = s;
        return w;
    }
    // b == 0 and start_min < 0: continue into the previous buffer (T12)
    s = -1;
    for (;;) {
        if (s == start_min) break;  // not tested
        int32_t d = -s;
        if (d > p.tail_cols) {
            w.too_long = true;
            break;
        }
        if (!cell_above(prev(d), avg, p.thr, p.snr)) break;
        --s;
    }
    w.start = s;
    return w;
}

// start_dt / duration in float64 exactly as analyze.py:420-427
template <class P>
RT_HD double start_time(const DetectParamsT<P> &p, int32_t start) {
    return start < 0 ? -seg_time(-start, p.nperseg, p.fs) : seg_time(start, p.nperseg, p.fs);
}
template <class P>
RT_HD double run_duration(const DetectParamsT<P> &p, int32_t start, int32_t end) {
    return seg_time(end, p.nperseg, p.fs) - start_time(p, start);
}
template <class P>
RT_HD bool duration_ok(const DetectParamsT<P> &p, double dur) {
    if (dur < p.min_d) return false;
    if (dur > p.max_d) return false;
    return true;
}

// np.max / np.mean / np.std(dB(.)) over the cells of a plateau.  `cell(i)`,
// i in [0, n), yields the i-th element of `data` (analyze.py:437-440).
template <class P>
struct RunStatsT {
    P max_p, mean_p, std_db;
};
using RunStats = RunStatsT<float>;

RT_HD float db10(float v) { return 10.0f * log10f(v); }
RT_HD double db10(double v) { return 10.0 * log10(v); }

// Canonical summation order (so the wave-cooperative device code, the dense
// kernel and the host check agree bit for bit): 64 interleaved partial sums
// (cell k goes to partial k mod 64, in k order), folded by halving
// (p[l] += p[l + off], off = 32, 16, ... 1).  Sums run in float64 over the
// float32 values np.mean / np.std see; np.max propagates NaN.  The power type P is what `cell` yields (float64 maps:
// the same order, every step in float64).
constexpr int kStatLanes = 64;

template <class Cell>
RT_HD RunStatsT<typename std::decay<decltype(std::declval<Cell>()(0))>::type> run_stats(int32_t n, Cell cell) {
    using P = typename std::decay<decltype(cell(0))>::type;
    double ps[kStatLanes], pd[kStatLanes];
    P pm[kStatLanes];
    bool any_nan = false;
    for (int l = 0; l < kStatLanes; ++l) {
        ps[l] = 0.0;
        pd[l] = 0.0;
        pm[l] = -INFINITY;
    }
    for (int32_t k = 0; k < n; ++k) {
        const int l = k & (kStatLanes - 1);
        const P v = cell(k);
        ps[l] += (double)v;
        pd[l] += (double)db10(v);
        if (v != v) any_nan = true;
        if (v > pm[l]) pm[l] = v;
    }
    for (int off = kStatLanes / 2; off > 0; off >>= 1)
        for (int l = 0; l < off; ++l) {
            ps[l] += ps[l + off];
            pd[l] += pd[l + off];
            if (pm[l + off] > pm[l]) pm[l] = pm[l + off];
        }
    const double mean_db = pd[0] / (double)n;
    double pa[kStatLanes];
    for (int l = 0; l < kStatLanes; ++l) pa[l] = 0.0;
    for (int32_t k = 0; k < n; ++k) {
        const double d = (double)db10(cell(k)) - mean_db;
        pa[k & (kStatLanes - 1)] += d * d;
    }
    for (int off = kStatLanes / 2; off > 0; off >>= 1)
        for (int l = 0; l < off; ++l) pa[l] += pa[l + off];
    RunStatsT<P> r;
    r.max_p = any_nan ? (P)NAN : pm[0];
    r.mean_p = (P)(ps[0] / (double)n);
    r.std_db = (P)sqrt(pa[0] / (double)n);
    return r;
}

// datetime.timedelta(seconds=x) -> whole microseconds, CPython's algorithm:
// split off the integer seconds exactly, scale the fraction by 1e6 in double,
// split again, round the leftover half-to-even against the parity of the sum.
RT_HD int64_t timedelta_us(double seconds) {
    double ip;
    double frac = modf(seconds, &ip);
    int64_t us = (int64_t)ip * 1000000LL;
    if (frac == 0.0) return us;
    double ip2;
    double left = modf(1000000.0 * frac, &ip2);
    us += (int64_t)ip2;
    if (left != 0.0) {
        double whole = round(left);
        if (fabs(whole - left) == 0.5) {
            int odd = (int)(us & 1LL);
            whole = 2.0 * round((left + odd) * 0.5) - odd;
        }
        us += (int64_t)whole;
    }
    return us;
}

// A maximal run [b, e) of above-cells of the current buffer -> at most one
// plateau (analyze.py:401-433 in run-based form): the
// cheap decisions.  `prev(d)` reads the previous buffer's cell n_seg_last - d.
// Returns true and the first cell of `data` if the run becomes a signal.
template <class P, class Prev>
RT_HD bool gate_run(const DetectParamsT<P> &p, int32_t b, int32_t e, typename same_t<P>::type avg, Prev prev, int32_t *start_out) {
    if (e == p.n_seg) return false;  // laps into the next buffer (analyze.py:415)
    const int32_t ti0 = first_probe_in_run(b, e, p.stride);
    if (ti0 < 0) return false;       // no strided probe lands in the run (T9)
    const StartWalk sw = walk_start(p, b, ti0, avg, prev);
    if (sw.too_long) return false;
    if (!duration_ok(p, run_duration(p, sw.start, e))) return false;
    *start_out = sw.start;
    return true;
}

// Cell `t` of a plateau's `data` (analyze.py:437-440) for bin `fi`: segment t >= 0 of the buffer's map `map` ([T][F], this
// stream's), t < 0 counted back from the end of the previous buffer (analyze.py:438: `_spectrogram_last[fi][start:]`), of which
// `prev` holds the last `prev_cols` columns ([prev_cols][F], this stream's: a whole previous map, or the look-back tail).  The
// one indexing rule of the dense detectors' statistics, the record-cells gather (rt_cells.h) and the host check.
template <class P>
RT_HD P record_cell(const P *map, const P *prev, int32_t prev_cols, int32_t F, int32_t fi, int32_t t) {
    return t < 0 ? prev[((int64_t)prev_cols + t) * F + fi] : map[(int64_t)t * F + fi];
}

// gate + statistics for one run, sequentially (host check; the kernels gate
// per thread and compute the statistics wave-cooperatively in the same order)
template <class P, class Cur, class Prev, class Emit>
RT_HD void finish_run(const DetectParamsT<P> &p, int32_t b, int32_t e, typename same_t<P>::type avg, Cur cur, Prev prev, Emit emit) {
    int32_t start;
    if (!gate_run(p, b, e, avg, prev, &start)) return;
    auto cell = [&](int32_t k) -> P {
        const int32_t t = start + k;
        return t < 0 ? prev(-t) : cur(t);
    };
    emit(start, e, run_stats(e - start, cell));
}

// Sequential scan of one bin's row of a dense spectrogram (analyze.py:357-450):
// calls on_run(b, e, avg) for every maximal run of above-cells.  Returns false
// when no cell reaches the absolute threshold (the row mean is then unused).
// `row_sum` < 0 means "not known": the row is summed here.  `sum_out` (or null): that sum, whatever the row holds
// (RT_FLAG_ROW_MEANS: the float64 handle keeps every row's mean).
// np.mean(row) (analyze.py:375) from the row's float64 sum: float32 rows as float32 (the sum rounded once), float64 rows in float64
RT_HD float row_mean_of(double sum, int32_t T, float) { return (float)sum / (float)T; }
RT_HD double row_mean_of(double sum, int32_t T, double) { return sum / (double)T; }

template <class P, class Cur, class OnRun>
RT_HD bool scan_dense_row(const DetectParamsT<P> &p, Cur cur, double row_sum, P *avg_out, OnRun on_run, double *sum_out = nullptr) {
    const int32_t T = p.n_seg;
    double sum = 0.0;
    bool any = false;
    for (int32_t t = 0; t < T; ++t) {
        const P v = cur(t);
        sum += (double)v;
        any |= !(v < p.thr);
    }
    if (sum_out) *sum_out = row_sum >= 0.0 ? row_sum : sum;
    if (!any) return false;
    if (row_sum >= 0.0) sum = row_sum;
    const P avg = row_mean_of(sum, T, P());  // np.mean(row) (analyze.py:375)
    *avg_out = avg;
    int32_t b = -1;
    for (int32_t t = 0; t <= T; ++t) {
        const bool ab = (t < T) && cell_above(cur(t), avg, p.thr, p.snr);
        if (ab) {
            if (b < 0) b = t;
            continue;
        }
        if (b < 0) continue;
        const int32_t rb = b;
        b = -1;
        on_run(rb, t, avg);
    }
    return true;
}

// is_shadow_of (analyze.py:300-311) on microsecond offsets from ts_start.
template <class P>
RT_HD bool shadowed_by(int64_t ts_i, int64_t dur_i, P max_i, int64_t ts_j, int64_t dur_j, P max_j) {
    if (ts_i > ts_j + dur_j) return false;
    if (ts_i + dur_i < ts_j) return false;
    return max_j > max_i;
}

// Position of record i in (fi, start) order and its shadow verdict against
// the unfiltered list (analyze.py:325).  max is compared as the reference's
// float32 dBW figure (analyze.py:442) -- float64 records (P = double) as the float64 one.
template <class Rec, class P>
RT_HD void rank_and_shadow(int32_t i, int32_t n, const Rec *rec, const long long *ts_us, const long long *dur_us,
                           P cal_db, int32_t *rank_out, int32_t *shadow_out) {
    const int32_t fi = rec[i].fi, st = rec[i].start;
    const P mx_i = db10(rec[i].max_p) - cal_db;
    int32_t rank = 0, shadow = 0;
    for (int32_t j = 0; j < n; ++j) {
        if (rec[j].fi < fi || (rec[j].fi == fi && rec[j].start < st)) ++rank;
        const P mx_j = db10(rec[j].max_p) - cal_db;
        if (shadowed_by(ts_us[i], dur_us[i], mx_i, ts_us[j], dur_us[j], mx_j)) shadow = 1;
    }
    *rank_out = rank;
    *shadow_out = shadow;
}

// ---- records from a float64 cell list (RT_FLAG_F64_SPARSE: detect_sparse_f64 in rt_f64_sparse.h, hc_extract_sparse_f64) ----
// A stream's list holds every cell at or above the absolute threshold (NaN included) and every cell whose successor in time is
// one (the scan's emission rule), so a cell that is missing is below the threshold.  Sorted by key (f64_cell_key), the cells
// [start, end) of a plateau that lie in this buffer are neighbours in the list: the run's cells are above, the one before it
// has a hot successor.
// Entry j of the sorted list (keys(j), vals(j); n entries): does a maximal run of above-cells begin on it?  Then [*b, *e).
template <class Keys, class Vals>
RT_HD bool sparse_run_at(const DetectParamsT<double> &p, Keys keys, Vals vals, int32_t n, int32_t j, double avg, int32_t *b, int32_t *e) {
    const uint32_t key = keys(j);
    const int32_t t = f64_key_seg(key);
    if (!cell_above(vals(j), avg, p.thr, p.snr)) return false;
    if (t > 0 && j > 0 && keys(j - 1) == key - 1u && cell_above(vals(j - 1), avg, p.thr, p.snr)) return false;  // inside a run
    int32_t jj = j, tt = t;
    while (jj + 1 < n && tt + 1 < p.n_seg && keys(jj + 1) == keys(jj) + 1u && cell_above(vals(jj + 1), avg, p.thr, p.snr)) {
        ++jj;
        ++tt;
    }
    *b = t;
    *e = tt + 1;
    return true;
}

// ---- exact run-length pre-filter: the planner's arithmetic (rt_kernels.h: plan_runs; host copy in rt_hostcheck.cpp) ----
// One 64-bit word = 64 independent cells (the threshold bits of four lanes' sixteen bins each); the planner walks a word column
// upwards in time with two bit-sliced counters of K planes, r = the cells a plateau needs:
//     SAT[u] = the threshold run ending at row u has r cells or more     (sticky while the run lasts)
//     FAR[u] = no SAT row among the last r rows
// step(h) takes row u's word and returns C[u - r + 1] = ~FAR[u]: "row u - r + 1 lies in a threshold run of >= r cells".
// K planes hold counts up to 2^K - 1 >= r - 1; a count that wraps while its flag is already set changes nothing.
constexpr int kPlanRowsPerWave = 16384;  // rows of one wave at most (its byte flags in LDS)
constexpr int kPlanMaxRun = 65536;       // r at most (16 counter planes)
template <int K>
struct RunPlanner {
    unsigned long long c1[K], c2[K], inv[K], sat, far;
    RT_HD void init(int r) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            c1[k] = 0ull;
            c2[k] = 0ull;
            inv[k] = (((unsigned)(r - 1) >> k) & 1u) ? 0ull : ~0ull;  // (plane ^ inv[k]) is all ones where the plane agrees with bit k of r - 1
        }
        sat = 0ull;
        far = ~0ull;
    }
    RT_HD unsigned long long step(unsigned long long hh) {
        unsigned long long eq = ~0ull;
#pragma unroll
        for (int k = 0; k < K; ++k) eq &= c1[k] ^ inv[k];
        sat = hh & (sat | eq);  // run[u - 1] reached r - 1 at some point and the bit stayed set
        unsigned long long carry = ~0ull;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const unsigned long long t = c1[k] ^ carry;
            carry &= c1[k];
            c1[k] = t & hh;  // (a clear bit ends the run)
        }
        eq = ~0ull;
#pragma unroll
        for (int k = 0; k < K; ++k) eq &= c2[k] ^ inv[k];
        far = ~sat & (far | eq);
        carry = ~0ull;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const unsigned long long t = c2[k] ^ carry;
            carry &= c2[k];
            c2[k] = t & ~sat;
        }
        return ~far;
    }
};
// Rows per planning tile for a call of n_seg segments: tiles a few halos long (a tile reads 2 r - 1 rows beside its own),
// a whole number of waves' worth of them per stream (a wave holds 64 / w tiles side by side), a wave's rows within its flags.
RT_HD int plan_tile_rows(int n_seg, int lg, int r) {
    const int tpw = 64 / (lg / 4);
    const int target = (4 * r > 64) ? 4 * r : 64;
    int waves = n_seg / (tpw * target);
    if (waves < 1) waves = 1;
    const int waves_min = (n_seg + kPlanRowsPerWave - 1) / kPlanRowsPerWave;
    if (waves < waves_min) waves = waves_min;
    const int tiles = waves * tpw;
    int rows = (n_seg + tiles - 1) / tiles;
    return rows < 1 ? 1 : rows;
}
// One word column of one tile (rows a .. a + B - 1 of a buffer of n_seg rows): `row(u)` yields row u's word for 0 <= u < n_seg,
// `emit(t, need)` receives need[t] = C[t] | C[t + 1] (the cell before a run: `data` starts on it) for the tile's rows inside
// the buffer.  Rows before the buffer count as set (a run through t = 0 may continue a plateau of the previous buffer: any
// length keeps it), rows past it as clear.  The kernel runs the same steps, eight rows per batch with the loads ahead.
template <int K, class Row, class Emit>
RT_HD void plan_tile_column(int a, int B, int n_seg, int r, Row row, Emit emit) {
    RunPlanner<K> pl;
    pl.init(r);
    unsigned long long c_prev = 0ull;
    const int t_end = (a + B < n_seg) ? a + B : n_seg;
    for (int u = a - r + 1; u <= a + B + r - 1; ++u) {
        const unsigned long long hh = (u < 0) ? ~0ull : (u < n_seg) ? row(u) : 0ull;
        const unsigned long long c_now = pl.step(hh);
        const int t = u - r;
        if (t >= a && t < t_end) emit(t, c_prev | ((t + 1 < n_seg) ? c_now : 0ull));
        c_prev = c_now;
    }
}

}  // namespace rt
#endif
