// rt_record_stft_book.h -- host side of rt_fetch_record_stft (include/rt_analyze.h): the work list record_stft (rt_record_stft.h)
// runs from, and the one factor it multiplies by.  Host-only (no HIP): rt_analyze.hip calls it inside the entry, rt_hostcheck.cpp
// exports it to the CPU suite (hc_stft_*), tests/c/stft_work.cpp runs it under the sanitizers.
//
// A delivered call's snippets lie in its slot's pool in record order, whole segments only (rt_record_iq_book.h: iq_build_descs), so
// delivered segment g of the call -- counted over all records -- starts at sample g * N of the pool.  The kernel therefore needs no
// entry per segment: the records' first segments as a prefix [n + 1] (the IQ entry's offsets divided by N) and each record's bin
// are the whole list, and a wave finds its record by binary search over the prefix.
#ifndef RT_RECORD_STFT_BOOK_H
#define RT_RECORD_STFT_BOOK_H

#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

namespace rt {

struct StftWork {
    std::vector<int64_t> seg_first;  // [n + 1] delivered segments in front of each record; seg_first[n]: all of them
    std::vector<int32_t> fi;         // [n] each record's bin, fftfreq order
};

// `offsets` [n + 1]: IqSlot::offsets (samples); `fi` [n]: the records' bins.  Returns the call's delivered segments, or -1 where the
// lists are not what iq_build_descs writes (an offset that is no multiple of N or runs backwards, a bin outside 0 .. N - 1): the
// kernel indexes its twiddle table with fi and the pool with the prefix, so nothing is launched from such a list.
inline int64_t stft_build_work(const int64_t *offsets, const int32_t *fi, size_t n, int N, StftWork *w) {
    if (N < 1 || !offsets || offsets[0] != 0 || (n && !fi)) return -1;
    if (w) {
        w->seg_first.assign(n + 1, 0);
        w->fi.assign(n, 0);
    }
    for (size_t i = 0; i < n; ++i) {
        if (offsets[i + 1] < offsets[i] || offsets[i + 1] % N != 0 || fi[i] < 0 || fi[i] >= N) return -1;
        if (w) {
            w->seg_first[i + 1] = offsets[i + 1] / N;
            w->fi[i] = fi[i];
        }
    }
    return offsets[n] / N;
}

// the record whose segments hold delivered segment g (0 <= g < seg_first[n]): the last one that starts at or before it -- records
// without a segment are stepped over.  The kernel's search, word for word.
inline int stft_record_of(const int64_t *seg_first, int n, int64_t g) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (seg_first[mid] <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// ---- rt_fetch_record_stft_hop: frames every h = N / k samples (record_stft_hop, rt_record_stft_hop.h) ----
// A record's delivered segments fall into two PARTS that lie one behind the other in the pool: the Lp segments below 0 (the
// predecessor buffer's) and the Lc from 0 on (the call's own).  A part of L >= 1 segments has (L - 1) k + 1 frames, frame j the N
// samples from sample j h of the part; a part without a segment has none, and no frame straddles the two parts -- the predecessor's
// ragged remainder lies between them.  The list is per record again; a lane group finds its record by binary search over the frame
// prefix and its part by one comparison.
struct StftHopWork {
    int N = 0, k = 0;
    std::vector<int64_t> frame_first;  // [n + 1] frames in front of each record; frame_first[n]: all of them
    std::vector<int64_t> pool_seg;     // [n] the pool segment of each record's first delivered segment
    std::vector<int32_t> lp;           // [n] segments of the predecessor part: clamp(-first_seg, 0, L)
    std::vector<int32_t> fi;           // [n] each record's bin, fftfreq order
};

constexpr int kStftHopMaxDiv = 16;

inline bool stft_hop_div_ok(int N, int k) { return N >= 1 && k >= 1 && k <= kStftHopMaxDiv && N % k == 0; }
inline int64_t stft_hop_part_frames(int64_t L, int k) { return L > 0 ? (L - 1) * k + 1 : 0; }

// `offsets`, `fi` as stft_build_work takes them, `first_seg` [n]: IqSlot::first_seg.  Returns the call's frames, or -1 where the
// lists are not what iq_build_descs writes or k is no divisor of N in 1 .. 16: nothing is launched from such a list.
inline int64_t stft_hop_build_work(const int64_t *offsets, const int32_t *first_seg, const int32_t *fi, size_t n, int N, int k, StftHopWork *w) {
    if (!stft_hop_div_ok(N, k) || (n && !first_seg)) return -1;
    if (stft_build_work(offsets, fi, n, N, nullptr) < 0) return -1;
    if (w) {
        w->N = N;
        w->k = k;
        w->frame_first.assign(n + 1, 0);
        w->pool_seg.assign(n, 0);
        w->lp.assign(n, 0);
        w->fi.assign(n, 0);
    }
    int64_t frames = 0;
    for (size_t i = 0; i < n; ++i) {
        const int64_t L = (offsets[i + 1] - offsets[i]) / N;
        const int64_t Lp = std::min<int64_t>(std::max<int64_t>(-(int64_t)first_seg[i], 0), L);
        if (L > INT32_MAX) return -1;
        frames += stft_hop_part_frames(Lp, k) + stft_hop_part_frames(L - Lp, k);
        if (w) {
            w->frame_first[i + 1] = frames;
            w->pool_seg[i] = offsets[i] / N;
            w->lp[i] = (int32_t)Lp;
            w->fi[i] = fi[i];
        }
    }
    return frames;
}

struct StftHopFrame {
    int record;      // the record frame g belongs to
    int part;        // 0: the predecessor part, 1: the record's own
    int64_t sample;  // the frame's first sample in the pool
};

// frame g (0 <= g < frame_first[n]) -> its record (the last one that starts at or before it), its part and where its N samples
// start.  The kernel's search, word for word.
inline StftHopFrame stft_hop_frame_at(const int64_t *frame_first, const int64_t *pool_seg, const int32_t *lp, int n, int N, int k, int64_t g) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (frame_first[mid] <= g) lo = mid; else hi = mid - 1;
    }
    const int64_t j = g - frame_first[lo], h = N / k;
    const int64_t Lp = lp[lo], Fp = Lp > 0 ? (Lp - 1) * k + 1 : 0;
    if (j < Fp) return StftHopFrame{lo, 0, pool_seg[lo] * N + j * h};
    return StftHopFrame{lo, 1, (pool_seg[lo] + Lp) * N + (j - Fp) * h};
}
inline StftHopFrame stft_hop_frame_at(const StftHopWork &w, int64_t g) {
    return stft_hop_frame_at(w.frame_first.data(), w.pool_seg.data(), w.lp.data(), (int)w.lp.size(), w.N, w.k, g);
}

// ---- rt_fetch_record_band: the bins beside each record's bin (record_band, rt_record_band.h) ----
// The frames and the work list are the hop entry's (StftHopWork, stft_hop_frame_at): nothing per record is added.  A frame has
// B = 2 w + 1 columns, column j the bin (fi + j - w) mod N in fftfreq order -- the band is circular.
constexpr int kStftBandMaxHalf = 8;

inline bool stft_band_ok(int N, int k, int w) { return stft_hop_div_ok(N, k) && w >= 0 && w <= kStftBandMaxHalf && 2 * w + 1 <= N; }
inline int stft_band_columns(int w) { return 2 * w + 1; }
// column j (0 <= j < 2 w + 1) of a record at bin fi (0 <= fi < N) -> its bin in 0 .. N - 1
inline int stft_band_bin(int fi, int j, int w, int N) {
    int b = fi + (j - w);  // (|j - w| <= 8 < N: one correction either way)
    if (b < 0) b += N;
    if (b >= N) b -= N;
    return b;
}
// complex values of the pool for `frames` frames: frames * (2 w + 1), or -1 where that (or its bytes at 16 a value) leaves int64
inline int64_t stft_band_elems(int64_t frames, int w) {
    if (frames < 0 || w < 0 || w > kStftBandMaxHalf) return -1;
    const int64_t B = 2 * (int64_t)w + 1;
    if (frames > (INT64_MAX / 16) / B) return -1;
    return frames * B;
}

// ---- rt_fetch_record_estimates: one row per record from the frames (record_estimates, rt_record_estimates.h) ----
// The frames are the hop entry's, so the prefix and lp are StftHopWork's.  On top of them a record has, per part, the frames that
// lie wholly INSIDE its own cells -- start * N <= position and position + N <= end * N.  A part's positions rise by h, so its
// inside frames are one run [lo, hi) of the record's frame indices (part 0: 0 .. Fp, part 1: Fp .. F), an empty run being lo == hi;
// `base` is the position of each part's first frame (first_seg * N, max(first_seg, 0) * N) and `fmod` the turn-back index fi mod k.
struct EstimatesWork {
    int N = 0, k = 0;
    std::vector<int64_t> frame_first;  // [n + 1] StftHopWork::frame_first
    std::vector<int32_t> lp;           // [n] StftHopWork::lp
    std::vector<int32_t> range;        // [n][4] lo0, hi0, lo1, hi1: frame indices inside the record
    std::vector<int64_t> base;         // [n][2] position of frame 0 of part 0 and of part 1, relative to sample 0 of the call's buffer
    std::vector<int32_t> fmod;         // [n] fi mod k
};

// The run [lo, hi) of j in 0 .. F with start * N <= (seg0 * N + j h) and (seg0 * N + j h) + N <= end * N, h = N / k: positions are
// whole hops, so the bounds are (start - seg0) k and (end - 1 - seg0) k + 1, clamped.
inline void estimates_inside(int64_t seg0, int64_t F, int64_t start, int64_t end, int k, int64_t *lo, int64_t *hi) {
    *lo = std::min(std::max((start - seg0) * k, (int64_t)0), F);
    *hi = std::min(std::max((end - 1 - seg0) * k + 1, (int64_t)0), F);
    if (*hi < *lo) *hi = *lo;
}

// `offsets`, `first_seg`, `fi` as stft_hop_build_work takes them; `start`, `end` [n]: the records' cells.  Returns the call's
// frames, or -1 for what stft_hop_build_work refuses, for start > end, for a record of more than INT32_MAX frames and for a run
// that leaves its part: nothing is launched from such a list.
inline int64_t estimates_build_work(const int64_t *offsets, const int32_t *first_seg, const int32_t *fi, const int32_t *start, const int32_t *end,
                                    size_t n, int N, int k, EstimatesWork *w) {
    StftHopWork hop;
    const int64_t frames = stft_hop_build_work(offsets, first_seg, fi, n, N, k, &hop);
    if (frames < 0 || (n && (!start || !end))) return -1;
    if (w) {
        w->N = N;
        w->k = k;
        w->frame_first = hop.frame_first;
        w->lp = hop.lp;
        w->range.assign(4 * n, 0);
        w->base.assign(2 * n, 0);
        w->fmod.assign(n, 0);
    }
    for (size_t i = 0; i < n; ++i) {
        if (start[i] > end[i]) return -1;
        const int64_t F = hop.frame_first[i + 1] - hop.frame_first[i], Fp = stft_hop_part_frames(hop.lp[i], k);
        if (F > INT32_MAX) return -1;
        const int64_t seg0[2] = {(int64_t)first_seg[i], std::max<int64_t>(first_seg[i], 0)};
        int64_t lo[2], hi[2];
        estimates_inside(seg0[0], Fp, start[i], end[i], k, &lo[0], &hi[0]);
        estimates_inside(seg0[1], F - Fp, start[i], end[i], k, &lo[1], &hi[1]);
        lo[1] += Fp;
        hi[1] += Fp;
        if (lo[0] < 0 || hi[0] > Fp || lo[1] < Fp || hi[1] > F || lo[0] > hi[0] || lo[1] > hi[1]) return -1;
        if (w) {
            for (int p = 0; p < 2; ++p) {
                w->range[4 * i + 2 * p] = (int32_t)lo[p];
                w->range[4 * i + 2 * p + 1] = (int32_t)hi[p];
                w->base[2 * i + p] = seg0[p] * N;
            }
            w->fmod[i] = fi[i] % k;
        }
    }
    return frames;
}

// the turn-back table: (cos, sin) of 2 pi m / k for m = 0 .. k - 1; R is multiplied by cos - i sin.  The angle is formed as
// NumPy forms -2j * pi * m / k, so the factors are record_fine's (cos is even, sin odd in every libm).
inline void estimates_turn_table(int k, double *cs /* [2 k] */) {
    for (int m = 0; m < k; ++m) {
        const double x = 2.0 * 3.141592653589793 * (double)m / (double)k;
        cs[2 * m] = std::cos(x);
        cs[2 * m + 1] = std::sin(x);
    }
}

// ---- rt_fetch_record_spectrum: one row per record from the band's frames (record_spectrum, rt_record_spectrum.h) ----
// The frames are the band entry's and the inside runs the estimates entry's: the plan is EstimatesWork (estimates_build_work) and
// the argument rule stft_band_ok.  What an entry says where its rule refuses, before anything is launched or copied; empty where
// it accepts: the hop and estimates entries of (k, N), the band and spectrum entries of (k, w, N).
inline std::string stft_hop_rule(int N, int k) {
    return "hop_div k = " + std::to_string(k) + " must be 1 ... " + std::to_string(kStftHopMaxDiv) + " and divide nperseg N = " + std::to_string(N);
}
inline std::string stft_hop_refusal(int N, int k) { return stft_hop_div_ok(N, k) ? std::string() : stft_hop_rule(N, k); }
inline std::string spectrum_refusal(int N, int k, int w) {
    if (stft_band_ok(N, k, w)) return std::string();
    return stft_hop_rule(N, k) + ", half_width w = " + std::to_string(w) + " must be 0 ... " + std::to_string(kStftBandMaxHalf) + " with 2 w + 1 <= N";
}
// bytes of a slot's row pool for n records: the 48-byte rows, then the means and the peaks, [n][2 w + 1] float64 each
inline size_t spectrum_pool_bytes(size_t n, int w) { return n * (48 + 2 * sizeof(double) * (size_t)stft_band_columns(w)); }

// sqrt(scale), the factor between the windowed transform and a value: evaluated in float64, and on a float32 handle rounded once
inline float stft_root_f32(float scale) { return (float)std::sqrt((double)scale); }
inline double stft_root_f64(double scale) { return std::sqrt(scale); }

}  // namespace rt
#endif
