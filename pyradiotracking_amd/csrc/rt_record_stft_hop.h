// rt_record_stft_hop.h -- device side of rt_fetch_record_stft_hop (include/rt_analyze.h): record_stft_hop<P, FMT, G>, the complex
// STFT value of the record's bin for FRAMES every h = nperseg / k samples of a record's delivered parts.  A frame is a segment that
// starts elsewhere: its value is record_stft's (rt_record_stft.h) on the frame's N samples, with the window, the mean about the
// frame's first sample and the phase reference exp(-2 pi i fi n / N) all counted from the frame's start.  The work list is the
// host's (rt_record_stft_book.h: StftHopWork): the frame prefix, each record's first pool segment, the length of its predecessor
// part and its bin.
//
// A frame is taken by a GROUP of G lanes, G = 64 or -- where the frame has at most 32, 16 or 8 pieces of 16 bytes -- 32, 16 or 8;
// the 64 / G groups of a wave take consecutive frames, four waves a workgroup.  Lane l of the group owns the pieces l, l + G, ...
// counted from the frame's first byte and walks them as stft_segment does: the mean about the pivot, four fmas a sample against the
// table twiddle, then a butterfly inside the group (xor G / 2 ... 1).  With G = 64 that is stft_segment operation for operation.
// With G < 64 every lane holds at most one piece, the same one lane l of a whole wave would hold, and the lanes a whole wave would
// leave without a piece are simply not there: they would have added +0 in the butterfly's first steps, and v + (+0) is v for every
// v an accumulator can hold (it starts at +0 and cannot become -0: a sum that cancels exactly rounds to +0).  So a frame that is a
// delivered segment has the bytes record_stft gives it, whatever G (tests/test_record_stft_hop_contract.py restates both orders).
//
// The unit the pieces are loaded in (16, 8, 4 or 2 bytes) is one for the whole launch: the widest that divides the pool's address,
// a hop's bytes and a frame's bytes, hence every frame's first byte and length -- the groups of a wave never diverge on it.
// Consecutive frames overlap by (k - 1) / k and sit on consecutive groups and waves, so all but the first read of a line comes from
// L1 / L2; the samples are not staged in LDS.
#ifndef RT_RECORD_STFT_HOP_H
#define RT_RECORD_STFT_HOP_H

#include "rt_record_stft.h"

namespace rt {

template <class P>
struct StftHopArgs {
    const char *pool;            // the slot's snippets: delivered segment s at sample s * nperseg
    const int64_t *frame_first;  // [n_records + 1]
    const int64_t *pool_seg;     // [n_records]
    const int32_t *lp;           // [n_records]
    const int32_t *fi;           // [n_records], each in 0 .. nperseg - 1
    int32_t n_records;
    int32_t nperseg;
    int32_t hop_div;             // k: a divisor of nperseg in 1 .. 16
    int64_t n_frames;            // frame_first[n_records]
    int64_t pool_samples;        // samples the pool holds of this call: no frame may end behind them
    const P *window;             // [nperseg] the handle's window as the caller gave it
    const typename stft_types<P>::C *tw;  // [nperseg] W_N^j (rt_tables.h: record_stft_twiddles)
    P root;                      // sqrt(scale)
    typename stft_types<P>::C *values;    // [n_frames]
};

// the group's sum in a fixed order: the last log2(G) steps of stft_wave_sum; every lane of the group returns the same bits
template <int G, class C>
__device__ __forceinline__ C stft_group_sum(C v) {
#pragma unroll
    for (int m = G / 2; m >= 1; m >>= 1) {
        v.x += __shfl_xor(v.x, m, 64);
        v.y += __shfl_xor(v.y, m, 64);
    }
    return v;
}

// One frame by one group of G lanes; `lane`: the lane's number inside its group; W: the launch's load unit.  stft_segment
// (rt_record_stft.h) with G lanes for its 64; a group of fewer than 64 lanes holds one piece a lane and makes one round.
template <class P, int FMT, class W, int G>
__device__ __forceinline__ void stft_frame(const StftHopArgs<P> &a, const char *seg, int fi, int64_t g, int lane) {
    using C = typename stft_types<P>::C;
    using R = typename stft_raw<P, FMT>::type;
    constexpr int SPP = 16 / (int)sizeof(R);  // samples of a piece
    constexpr int LPP = 16 / (int)sizeof(W);  // loads of a piece
    constexpr int SPL = SPP / LPP;            // samples of a load
    constexpr int HOLD = G == 64 ? kStftHold : 1;
    static_assert(SPL >= 1, "a load holds whole samples");
    union Piece {
        W w[LPP];
        R r[SPP];
    };
    const int N = a.nperseg;
    const int n_pieces = (N + SPP - 1) / SPP;
    const int round = G * HOLD;
    Piece raw[HOLD];
    const auto load_round = [&](int base) {
#pragma unroll
        for (int j = 0; j < HOLD; ++j) {
            const int p = base + j * G + lane;
            const W *const src = reinterpret_cast<const W *>(seg + (int64_t)p * 16);
#pragma unroll
            for (int k = 0; k < LPP; ++k)
                if (p < n_pieces && p * SPP + k * SPL < N) raw[j].w[k] = src[k];  // (whole loads: SPL divides N)
        }
    };
    // 1. the mean about the frame's first sample
    const C x0 = stft_convert<P, FMT>(*reinterpret_cast<const R *>(seg));
    C sum{(P)0, (P)0};
    for (int base = 0; base < n_pieces; base += round) {
        load_round(base);
#pragma unroll
        for (int j = 0; j < HOLD; ++j) {
            const int n0 = (base + j * G + lane) * SPP;
#pragma unroll
            for (int e = 0; e < SPP; ++e)
                if (n0 + e < N) {
                    const C x = stft_convert<P, FMT>(raw[j].r[e]);
                    sum.x += x.x - x0.x;
                    sum.y += x.y - x0.y;
                }
        }
    }
    sum = stft_group_sum<G>(sum);
    const C mean{x0.x + sum.x / (P)N, x0.y + sum.y / (P)N};
    // 2. the windowed, detrended samples against W_N^(fi n), n from the frame's start
    const bool held = n_pieces <= round;  // the one round of pass 1 is still in `raw`
    const int step = (int)(((int64_t)fi * (G * SPP)) % N);
    int k_piece = (int)(((int64_t)fi * ((int64_t)lane * SPP)) % N);  // (fi n) mod N at the first sample of the lane's next piece
    C acc{(P)0, (P)0};
    for (int base = 0; base < n_pieces; base += round) {
        if (!held) load_round(base);
#pragma unroll
        for (int j = 0; j < HOLD; ++j) {
            const int n0 = (base + j * G + lane) * SPP;
            int k = k_piece;
#pragma unroll
            for (int e = 0; e < SPP; ++e) {
                if (n0 + e < N) {
                    const C x = stft_convert<P, FMT>(raw[j].r[e]);
                    const P w = a.window[n0 + e];
                    const C v{w * (x.x - mean.x), w * (x.y - mean.y)};
                    const C t = a.tw[k];
                    acc.x = stft_fma(v.x, t.x, acc.x);
                    acc.x = stft_fma(-v.y, t.y, acc.x);
                    acc.y = stft_fma(v.x, t.y, acc.y);
                    acc.y = stft_fma(v.y, t.x, acc.y);
                }
                k += fi;
                if (k >= N) k -= N;
            }
            k_piece += step;
            if (k_piece >= N) k_piece -= N;
        }
    }
    acc = stft_group_sum<G>(acc);
    if (lane == 0) a.values[g] = C{a.root * acc.x, a.root * acc.y};
}

// the lane group a frame of `nperseg` samples of `bytes_per_sample` takes: the smallest of 8, 16, 32 that holds its pieces, else 64
inline int stft_hop_group(int nperseg, int bytes_per_sample) {
#ifdef RT_STFT_HOP_FORCE_G64  // (tests/perf/bench_record_stft_hop.py builds this variant for its A/B; the product never defines it)
    return 64;
#endif
    const int64_t pieces = ((int64_t)nperseg * bytes_per_sample + 15) / 16;
    return pieces <= 8 ? 8 : pieces <= 16 ? 16 : pieces <= 32 ? 32 : 64;
}

template <class P, int FMT, int G>
__global__ __launch_bounds__(kStftBlock) void record_stft_hop(StftHopArgs<P> a) {
    using R = typename stft_raw<P, FMT>::type;
    constexpr int GPW = 64 / G;  // groups (frames) of a wave
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int in_wave = (int)(threadIdx.x & 63u);
    const int lane = in_wave & (G - 1);
    const int64_t g = ((int64_t)blockIdx.x * kStftWaves + wave) * GPW + in_wave / G;
    if (g >= a.n_frames) return;  // (whole groups leave: the butterflies stay inside a group)
    // the last record that starts at or before this frame, its part and the frame's first sample
    // (rt_record_stft_book.h: stft_hop_frame_at)
    int lo = 0, hi = a.n_records - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.frame_first[mid] <= g) lo = mid; else hi = mid - 1;
    }
    const int N = a.nperseg, k = a.hop_div;
    const int64_t j = g - a.frame_first[lo], h = N / k;
    const int64_t Lp = a.lp[lo], Fp = Lp > 0 ? (Lp - 1) * k + 1 : 0;
    const int64_t sample = j < Fp ? a.pool_seg[lo] * N + j * h : (a.pool_seg[lo] + Lp) * N + (j - Fp) * h;
    const int fi = a.fi[lo];
    if (fi < 0 || fi >= N || sample < 0 || sample + N > a.pool_samples) return;
    const char *const seg = a.pool + sample * (int64_t)sizeof(R);
    // one load unit for the launch: it divides the pool's address, a hop and a frame, so every frame's first byte and length
    const uintptr_t al = reinterpret_cast<uintptr_t>(a.pool) | (uintptr_t)(h * (int64_t)sizeof(R)) | (uintptr_t)((int64_t)N * (int64_t)sizeof(R));
    if ((al & 15u) == 0) {
        stft_frame<P, FMT, stft_u4, G>(a, seg, fi, g, lane);
    } else if constexpr (sizeof(R) <= 8) {
        if ((al & 7u) == 0) {
            stft_frame<P, FMT, stft_u2, G>(a, seg, fi, g, lane);
        } else if constexpr (sizeof(R) <= 4) {
            if ((al & 3u) == 0) {
                stft_frame<P, FMT, uint32_t, G>(a, seg, fi, g, lane);
            } else if constexpr (sizeof(R) <= 2) {
                stft_frame<P, FMT, uint16_t, G>(a, seg, fi, g, lane);
            }
        }
    }
}

}  // namespace rt
#endif
