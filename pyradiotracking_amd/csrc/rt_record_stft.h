// rt_record_stft.h -- device side of rt_fetch_record_stft (include/rt_analyze.h): record_stft<P, FMT>, one complex STFT value per
// delivered segment of a call's records, read from the slot's snippet pool (rt_record_iq.h filled it).  The work list is the
// host's (rt_record_stft_book.h): the records' first segments as a prefix and their bins.
//
//   value = sqrt(scale) * sum_n w[n] (x[n] - mean(x)) W_N^(fi n)          x: the segment's N samples, converted as the scans do
//
// One wave per segment, four waves a workgroup.  The segment is cut into PIECES of 16 bytes (2 complex64 samples, 4 int16 pairs,
// 8 uint8 / int8 pairs, 1 complex128); lane l owns the pieces l, l + 64, l + 128, ... and walks them in that order, the samples of
// a piece in theirs.  Which lane adds which sample when is fixed by that alone, so a value depends on the snippet and the bin and on
// nothing else -- not on where in the pool the snippet lies, which only decides how a piece is LOADED: in one 16-byte load where the
// segment's first byte and its length are multiples of 16, else in the widest of 8, 4 or 2 bytes that divides both (uint8 at
// nperseg 300: 600-byte segments, 8-byte loads and a last piece of 8 bytes).
//   1. the mean, about a pivot: x0 = the segment's first sample, mean = x0 + sum(x[n] - x0) / N.  A segment of one finite value
//      has every difference 0, mean = x0 and x - mean = 0 exactly, whatever N and however many bits the value has; the sum no
//      longer carries the offset, so its round-off scales with the spread of the samples, not with a DC level.
//   2. acc += (w[n] (x[n] - mean)) W_N^(fi n) by four fmas, the twiddle from the N-entry table at (fi n) mod N -- the index moves
//      by fi from sample to sample and by (64 * samples-per-piece * fi) mod N from piece to piece, reduced by one conditional
//      subtraction each: two integer divisions a wave, none in the loop, and no sincos.
//   Both sums: per lane in walk order, then a butterfly over the wave (xor 32, 16, ... 1; every lane ends with the same bits).  No
//   atomics: the same call gives the same bytes.  A segment of up to kStftHold pieces a lane (4 KiB) stays in registers between
//   the passes; a longer one is read again (from L2: a wave's segment is at most 256 KiB, and it read it a moment ago).
#ifndef RT_RECORD_STFT_H
#define RT_RECORD_STFT_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_kernels.h"

namespace rt {

constexpr int kStftBlock = 256;  // four waves, a segment each
constexpr int kStftWaves = kStftBlock / 64;
constexpr int kStftHold = 4;     // pieces of a lane in flight: all loads of a round before the first use
typedef uint32_t stft_u4 __attribute__((ext_vector_type(4)));  // the load units of 16 and 8 bytes
typedef uint32_t stft_u2 __attribute__((ext_vector_type(2)));

template <class P> struct stft_types { using C = cf; };
template <> struct stft_types<double> { using C = cd; };
// the raw sample of a format: the scans' own types; complex128 on a float64 handle
template <class P, int FMT> struct stft_raw { using type = typename raw_of<FMT>::type; };
template <> struct stft_raw<double, kFmtC64> { using type = cd; };

// a raw sample in the handle's precision: float32 as the scan kernels convert (rt_kernels.h: to_cf, uint8 by their one fma),
// float64 as rt_f64.h: load_f64 does (a division and a subtraction for uint8; the integer formats are exact either way)
template <class P, int FMT, class R>
__device__ __forceinline__ typename stft_types<P>::C stft_convert(R r) {
    if constexpr (sizeof(P) == 4) {
        return to_cf(r);
    } else if constexpr (FMT == kFmtU8) {
        return cd{(double)(r.iq & 0xFFu) / 127.5 - 1.0, (double)(r.iq >> 8) / 127.5 - 1.0};
    } else if constexpr (FMT == kFmtI16) {
        return cd{(double)(int16_t)(r.iq & 0xFFFFu) * (1.0 / 32768.0), (double)((int32_t)r.iq >> 16) * (1.0 / 32768.0)};
    } else if constexpr (FMT == kFmtI8) {
        return cd{(double)(int8_t)(r.iq & 0xFFu) * (1.0 / 128.0), (double)((int16_t)r.iq >> 8) * (1.0 / 128.0)};
    } else {
        return r;
    }
}

__device__ __forceinline__ float stft_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double stft_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }

// the wave's sum in a fixed order; every lane returns the same bits (a + b == b + a)
template <class C>
__device__ __forceinline__ C stft_wave_sum(C v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        v.x += __shfl_xor(v.x, m, 64);
        v.y += __shfl_xor(v.y, m, 64);
    }
    return v;
}

template <class P>
struct StftArgs {
    const char *pool;          // the slot's snippets: delivered segment g at sample g * nperseg
    const int64_t *seg_first;  // [n_records + 1]
    const int32_t *fi;         // [n_records], each in 0 .. nperseg - 1
    int32_t n_records;
    int32_t nperseg;
    int64_t n_segs;            // seg_first[n_records]
    const P *window;           // [nperseg] the handle's window as the caller gave it
    const typename stft_types<P>::C *tw;  // [nperseg] W_N^j (rt_tables.h: record_stft_twiddles)
    P root;                    // sqrt(scale)
    typename stft_types<P>::C *values;    // [n_segs]
};

// One segment by one wave; W: the unit its pieces are loaded in (wave-uniform: it divides the segment's address and length).
template <class P, int FMT, class W>
__device__ __forceinline__ void stft_segment(const StftArgs<P> &a, const char *seg, int fi, int64_t g, int lane) {
    using C = typename stft_types<P>::C;
    using R = typename stft_raw<P, FMT>::type;
    constexpr int SPP = 16 / (int)sizeof(R);  // samples of a piece
    constexpr int LPP = 16 / (int)sizeof(W);  // loads of a piece
    constexpr int SPL = SPP / LPP;            // samples of a load
    static_assert(SPL >= 1, "a load holds whole samples");
    union Piece {
        W w[LPP];
        R r[SPP];
    };
    const int N = a.nperseg;
    const int n_pieces = (N + SPP - 1) / SPP;
    const int round = 64 * kStftHold;
    Piece raw[kStftHold];
    const auto load_round = [&](int base) {
#pragma unroll
        for (int j = 0; j < kStftHold; ++j) {
            const int p = base + j * 64 + lane;
            const W *const src = reinterpret_cast<const W *>(seg + (int64_t)p * 16);
#pragma unroll
            for (int k = 0; k < LPP; ++k)
                if (p < n_pieces && p * SPP + k * SPL < N) raw[j].w[k] = src[k];  // (whole loads: SPL divides N)
        }
    };
    // 1. the mean about the segment's first sample
    const C x0 = stft_convert<P, FMT>(*reinterpret_cast<const R *>(seg));
    C sum{(P)0, (P)0};
    for (int base = 0; base < n_pieces; base += round) {
        load_round(base);
#pragma unroll
        for (int j = 0; j < kStftHold; ++j) {
            const int n0 = (base + j * 64 + lane) * SPP;
#pragma unroll
            for (int e = 0; e < SPP; ++e)
                if (n0 + e < N) {
                    const C x = stft_convert<P, FMT>(raw[j].r[e]);
                    sum.x += x.x - x0.x;
                    sum.y += x.y - x0.y;
                }
        }
    }
    sum = stft_wave_sum(sum);
    const C mean{x0.x + sum.x / (P)N, x0.y + sum.y / (P)N};
    // 2. the windowed, detrended samples against W_N^(fi n)
    const bool held = n_pieces <= round;  // the one round of pass 1 is still in `raw`
    const int step = (int)(((int64_t)fi * (64 * SPP)) % N);
    int k_piece = (int)(((int64_t)fi * ((int64_t)lane * SPP)) % N);  // (fi n) mod N at the first sample of the lane's next piece
    C acc{(P)0, (P)0};
    for (int base = 0; base < n_pieces; base += round) {
        if (!held) load_round(base);
#pragma unroll
        for (int j = 0; j < kStftHold; ++j) {
            const int n0 = (base + j * 64 + lane) * SPP;
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
    acc = stft_wave_sum(acc);
    if (lane == 0) a.values[g] = C{a.root * acc.x, a.root * acc.y};
}

template <class P, int FMT>
__global__ __launch_bounds__(kStftBlock) void record_stft(StftArgs<P> a) {
    using R = typename stft_raw<P, FMT>::type;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = (int)(threadIdx.x & 63u);
    const int64_t g = (int64_t)blockIdx.x * kStftWaves + wave;
    if (g >= a.n_segs) return;
    // the last record that starts at or before this segment (rt_record_stft_book.h: stft_record_of)
    int lo = 0, hi = a.n_records - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.seg_first[mid] <= g) lo = mid; else hi = mid - 1;
    }
    const int fi = a.fi[lo];
    if (fi < 0 || fi >= a.nperseg) return;
    const int64_t seg_bytes = (int64_t)a.nperseg * (int64_t)sizeof(R);
    const char *const seg = a.pool + g * seg_bytes;
    const uintptr_t al = reinterpret_cast<uintptr_t>(seg) | (uintptr_t)seg_bytes;
    if ((al & 15u) == 0) {
        stft_segment<P, FMT, stft_u4>(a, seg, fi, g, lane);
    } else if constexpr (sizeof(R) <= 8) {
        if ((al & 7u) == 0) {
            stft_segment<P, FMT, stft_u2>(a, seg, fi, g, lane);
        } else if constexpr (sizeof(R) <= 4) {
            if ((al & 3u) == 0) {
                stft_segment<P, FMT, uint32_t>(a, seg, fi, g, lane);
            } else if constexpr (sizeof(R) <= 2) {
                stft_segment<P, FMT, uint16_t>(a, seg, fi, g, lane);
            }
        }
    }
}

}  // namespace rt
#endif
