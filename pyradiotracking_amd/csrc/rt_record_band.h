// rt_record_band.h -- device side of rt_fetch_record_band (include/rt_analyze.h): record_band<P, FMT, G, HW>, for every frame of
// rt_fetch_record_stft_hop the complex STFT values of the B = 2 w + 1 bins (fi - w ... fi + w) mod N around the record's bin.  The
// frames, the work list and the search are that entry's (rt_record_stft_hop.h, rt_record_stft_book.h: StftHopWork); so is the
// lane-group form: G = 8 / 16 / 32 / 64 lanes by the frame's 16-byte pieces, consecutive frames on consecutive groups, four waves
// a workgroup, one load unit for the launch.
//
// A frame's samples are loaded once and its mean is taken once (pass 1, stft_frame's).  Pass 2 forms w[n] (x[n] - mean) once a
// sample and adds it into one accumulator per column against that column's own table twiddle: per column the four fmas, their
// order and the group butterfly are stft_frame's at that bin, so a column's value depends on the frame's samples and its bin alone
// -- column w is the hop entry's bytes, and a record d bins away has this column's bytes in its own centre column.  (Rotating the
// centre bin's products by W^(d n) would be cheaper and round differently: it is not done.)
//
// The columns are a template bound: HW = 0, 2 or 8 is the smallest that holds the call's w, the accumulators and twiddle indices
// are arrays of 2 HW + 1 with every index a constant after unrolling (registers, no scratch), and the columns beyond w of such an
// instantiation are computed and not stored.  A column's twiddle index steps by its bin modulo N; the indices of neighbouring
// columns differ by n mod N, so only the first column's start takes a division.  The twiddles are read from the N-entry table in
// global memory (EXPERIMENTS.md section 4.8: the LDS copy, -DRT_BAND_LDS_TABLE).  After the butterfly every lane of the group
// holds all sums; lane 0 stores the frame's B values in one run, float32 values two to a 16-byte store where the run's address
// allows.
#ifndef RT_RECORD_BAND_H
#define RT_RECORD_BAND_H

#include "rt_record_stft_hop.h"

namespace rt {

template <class P>
struct StftBandArgs {
    StftHopArgs<P> hop;   // the hop entry's arguments; hop.values: [n_frames][2 w + 1]
    int32_t half_width;   // w: 0 .. 8, 2 w + 1 <= nperseg
};

// the template bound an instantiation is compiled for: the smallest of 0, 2, 8 that holds w
inline int stft_band_bound(int w) { return w <= 0 ? 0 : w <= 2 ? 2 : 8; }
// dynamic LDS of a launch: none -- but for the A/B variant that keeps the twiddle table there
inline size_t stft_band_lds_bytes(int nperseg, size_t value_bytes) {
#ifdef RT_BAND_LDS_TABLE
    return (size_t)nperseg * value_bytes;
#else
    (void)nperseg;
    (void)value_bytes;
    return 0;
#endif
}

template <class P, int FMT, class W, int G, int HW>
__device__ __forceinline__ void band_frame(const StftBandArgs<P> &b, const typename stft_types<P>::C *tw, const char *seg, int fi, int64_t g, int lane) {
    using C = typename stft_types<P>::C;
    using R = typename stft_raw<P, FMT>::type;
    constexpr int SPP = 16 / (int)sizeof(R);  // samples of a piece
    constexpr int LPP = 16 / (int)sizeof(W);  // loads of a piece
    constexpr int SPL = SPP / LPP;            // samples of a load
    constexpr int HOLD = G == 64 ? kStftHold : 1;
    constexpr int BT = 2 * HW + 1;            // columns this instantiation carries
    static_assert(SPL >= 1, "a load holds whole samples");
    union Piece {
        W w[LPP];
        R r[SPP];
    };
    const StftHopArgs<P> &a = b.hop;
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
    // 1. the mean about the frame's first sample (stft_frame's pass 1)
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
    // 2. the windowed, detrended samples against W_N^(bin n) for every column's bin, n from the frame's start
    const bool held = n_pieces <= round;  // the one round of pass 1 is still in `raw`
    int bin[BT], k_piece[BT], step[BT];
    C acc[BT];
    {
        const int first = ((fi - HW) % N + N) % N;               // column 0's bin
        const int m_lane = (int)(((int64_t)lane * SPP) % N);     // n mod N at the lane's first piece, and over a round of pieces
        const int m_step = (int)((int64_t)(G * SPP) % N);
        bin[0] = first;
        k_piece[0] = (int)(((int64_t)first * ((int64_t)lane * SPP)) % N);
        step[0] = (int)(((int64_t)first * (G * SPP)) % N);
#pragma unroll
        for (int c = 1; c < BT; ++c) {  // ((bin + 1) n) mod N = ((bin n) mod N + n mod N) mod N
            bin[c] = bin[c - 1] + 1 == N ? 0 : bin[c - 1] + 1;
            k_piece[c] = bin[c] == 0 ? 0 : k_piece[c - 1] + m_lane;
            if (k_piece[c] >= N) k_piece[c] -= N;
            step[c] = bin[c] == 0 ? 0 : step[c - 1] + m_step;
            if (step[c] >= N) step[c] -= N;
        }
#pragma unroll
        for (int c = 0; c < BT; ++c) acc[c] = C{(P)0, (P)0};
    }
    for (int base = 0; base < n_pieces; base += round) {
        if (!held) load_round(base);
#pragma unroll
        for (int j = 0; j < HOLD; ++j) {
            const int n0 = (base + j * G + lane) * SPP;
            int k[BT];
#pragma unroll
            for (int c = 0; c < BT; ++c) k[c] = k_piece[c];
#pragma unroll
            for (int e = 0; e < SPP; ++e) {
                if (n0 + e < N) {
                    const C x = stft_convert<P, FMT>(raw[j].r[e]);
                    const P w = a.window[n0 + e];
                    const C v{w * (x.x - mean.x), w * (x.y - mean.y)};
#pragma unroll
                    for (int c = 0; c < BT; ++c) {
                        const C t = tw[k[c]];
                        acc[c].x = stft_fma(v.x, t.x, acc[c].x);
                        acc[c].x = stft_fma(-v.y, t.y, acc[c].x);
                        acc[c].y = stft_fma(v.x, t.y, acc[c].y);
                        acc[c].y = stft_fma(v.y, t.x, acc[c].y);
                    }
                }
#pragma unroll
                for (int c = 0; c < BT; ++c) {
                    k[c] += bin[c];
                    if (k[c] >= N) k[c] -= N;
                }
            }
#pragma unroll
            for (int c = 0; c < BT; ++c) {
                k_piece[c] += step[c];
                if (k_piece[c] >= N) k_piece[c] -= N;
            }
        }
    }
#pragma unroll
    for (int c = 0; c < BT; ++c) acc[c] = stft_group_sum<G>(acc[c]);
    if (lane != 0) return;
    // the frame's run of B = 2 w + 1 values: column c of this instantiation is column c - (HW - w) of the output
    const int skip = HW - b.half_width, B = 2 * b.half_width + 1;
    C *const out = a.values + g * (int64_t)B;
    if constexpr (sizeof(P) == 4) {
        typedef float band_f4 __attribute__((ext_vector_type(4)));
        const int odd = (int)((g * (int64_t)B) & 1);  // the run starts on the upper half of a 16-byte unit
#pragma unroll
        for (int c = 0; c < BT; ++c) {
            const int o = c - skip;
            if (o < 0 || o >= B) continue;
            const C v{a.root * acc[c].x, a.root * acc[c].y};
            if (((o + odd) & 1) != 0) {
                if (o == 0) out[o] = v;  // (otherwise stored with its left neighbour)
            } else if (c + 1 < BT && o + 1 < B) {
                const band_f4 two = {v.x, v.y, a.root * acc[c + 1 < BT ? c + 1 : c].x, a.root * acc[c + 1 < BT ? c + 1 : c].y};
                *reinterpret_cast<band_f4 *>(out + o) = two;
            } else {
                out[o] = v;
            }
        }
    } else {
#pragma unroll
        for (int c = 0; c < BT; ++c) {
            const int o = c - skip;
            if (o >= 0 && o < B) out[o] = C{a.root * acc[c].x, a.root * acc[c].y};
        }
    }
}

template <class P, int FMT, int G, int HW>
__global__ __launch_bounds__(kStftBlock) void record_band(StftBandArgs<P> b) {
    using R = typename stft_raw<P, FMT>::type;
    const StftHopArgs<P> &a = b.hop;
    constexpr int GPW = 64 / G;  // groups (frames) of a wave
#ifdef RT_BAND_LDS_TABLE  // (tests/perf/bench_record_band.py builds this variant for its A/B; the product never defines it)
    // the table copied to LDS by every workgroup, before any group leaves: nperseg * sizeof(C) bytes of dynamic LDS, which the
    // launch asks for -- a table that does not fit fails the launch, the variant is for sizes that do
    extern __shared__ char band_lds[];
    typename stft_types<P>::C *const tw = reinterpret_cast<typename stft_types<P>::C *>(band_lds);
    for (int i = (int)threadIdx.x; i < a.nperseg; i += kStftBlock) tw[i] = a.tw[i];
    __syncthreads();
#else
    const typename stft_types<P>::C *const tw = a.tw;
#endif
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int in_wave = (int)(threadIdx.x & 63u);
    const int lane = in_wave & (G - 1);
    const int64_t g = ((int64_t)blockIdx.x * kStftWaves + wave) * GPW + in_wave / G;
    if (g >= a.n_frames) return;  // (whole groups leave: the butterflies stay inside a group)
    if (b.half_width < 0 || b.half_width > HW || 2 * b.half_width + 1 > a.nperseg) return;
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
        band_frame<P, FMT, stft_u4, G, HW>(b, tw, seg, fi, g, lane);
    } else if constexpr (sizeof(R) <= 8) {
        if ((al & 7u) == 0) {
            band_frame<P, FMT, stft_u2, G, HW>(b, tw, seg, fi, g, lane);
        } else if constexpr (sizeof(R) <= 4) {
            if ((al & 3u) == 0) {
                band_frame<P, FMT, uint32_t, G, HW>(b, tw, seg, fi, g, lane);
            } else if constexpr (sizeof(R) <= 2) {
                band_frame<P, FMT, uint16_t, G, HW>(b, tw, seg, fi, g, lane);
            }
        }
    }
}

}  // namespace rt
#endif
