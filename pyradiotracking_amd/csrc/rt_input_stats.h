// rt_input_stats.h -- rt_set_input_stats / rt_fetch_input_stats (include/rt_analyze.h, which must be included first): one
// rt_input_stats row per stream from the RAW input of a call -- level, DC, clipping, non-finite components -- computed once, when
// the call is enqueued, by a streaming kernel family of its own.  No kernel of the analysis is touched.
//   input_stats<FMT>      grid (stream, chunk), one workgroup of kInputStatsBlock threads per kInputStatsChunk samples of a
//                         present stream; writes one InputStatsPart row per (stream, chunk).  No atomics.
//   input_stats_fold<A>   one thread per stream: adds the stream's rows in chunk order, converts once and writes the
//                         rt_input_stats row into the call slot's pinned host memory (zeros for an absent stream).
// The per-component rule -- raw value, rail, non-finite, what is added -- is stats_component below, host and device.  The integer
// formats accumulate exactly (every order gives the same integers), so their 16-byte pieces take a packed form of the same rule
// (stats_word8: four bytes per dot product; stats_word16), which the CPU suite holds to stats_component on every byte value.
// The float formats add in float64 in an order that is a function of the sample index alone:
//   piece p = (sample index within the chunk) / (samples per 16 bytes) belongs to thread p % kInputStatsBlock; a thread takes its
//   pieces in ascending order, a piece's components in memory order; the threads of a wave are folded by the xor butterfly
//   1, 2, 4 ... 32 (stats_butterfly), the waves in wave order, the chunks in chunk order.
// Only the WIDTH of a load depends on the row's alignment (a complex64 row that is only 8-byte aligned loads a piece as two
// halves).  input_stats_host runs all of this on the host, thread for thread: rt_hostcheck.cpp (hc_input_stats) and
// tests/c/input_stats_work.cpp.
#ifndef RT_INPUT_STATS_H
#define RT_INPUT_STATS_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "rt_core.h"

namespace rt {

constexpr int kInputStatsChunk = 16384;  // samples of one (stream, chunk) workgroup -- part of the float formats' summation order
constexpr int kInputStatsBlock = 256;    // its threads
constexpr int kInputStatsWave = 64;
constexpr int kInputStatsInFlight = 4;   // 16-byte loads of a thread in flight before the first is consumed
// the kernels' formats: kFmtC64 / kFmtU8 / kFmtI16 / kFmtI8 as the library numbers them, and complex128 (a float64 handle's kFmtC64)
constexpr int kStatsC64 = 0, kStatsU8 = 1, kStatsI16 = 2, kStatsI8 = 3, kStatsC128 = 4;

RT_HD constexpr int stats_sample_bytes(int fmt) { return fmt == kStatsC128 ? 16 : fmt == kStatsC64 ? 8 : fmt == kStatsI16 ? 4 : 2; }
RT_HD constexpr bool stats_is_float(int fmt) { return fmt == kStatsC64 || fmt == kStatsC128; }
RT_HD constexpr int32_t stats_unit(int fmt) { return fmt == kStatsU8 ? 255 : fmt == kStatsI8 ? 128 : fmt == kStatsI16 ? 32768 : 1; }
RT_HD constexpr int32_t stats_public_format(int fmt) { return fmt == kStatsC128 ? kStatsC64 : fmt; }

// One (stream, chunk) row, and a thread's registers: A = int64_t (integer formats) or double (float formats).
// Width (part of the contract): a chunk of int16 rails adds kInputStatsChunk * 2^31 = 2^45 to sum_sq; a buffer of n < 2^32 such
// samples stays below 2^63.
template <class A>
struct InputStatsPart {
    int64_t n_rail, n_nonfinite;
    A sum_i, sum_q, sum_sq, peak;
};
static_assert(sizeof(InputStatsPart<int64_t>) == 48 && sizeof(InputStatsPart<double>) == 48, "one row layout for both");

template <class A>
RT_HD void stats_clear(InputStatsPart<A> &a) {
    a.n_rail = a.n_nonfinite = 0;
    a.sum_i = a.sum_q = a.sum_sq = a.peak = (A)0;
}

// ---- the per-component rule ----
// Integer formats: `v` is the component as stored (uint8: the byte b; int8 / int16: the integer); comp 0 = I, 1 = Q.
template <int FMT>
RT_HD void stats_component(InputStatsPart<int64_t> &a, int32_t v, int comp) {
    static_assert(FMT == kStatsU8 || FMT == kStatsI8 || FMT == kStatsI16, "integer formats");
    const int32_t raw = FMT == kStatsU8 ? 2 * v - 255 : v;  // (2 b - 255) / 255 == b / 127.5 - 1
    const bool rail = FMT == kStatsU8 ? (v == 0 || v == 255) : FMT == kStatsI8 ? (v == -128 || v == 127) : (v == -32768 || v == 32767);
    a.n_rail += rail ? 1 : 0;
    if (comp == 0) a.sum_i += raw; else a.sum_q += raw;
    a.sum_sq += (int64_t)raw * raw;
    const int64_t mag = raw < 0 ? -(int64_t)raw : (int64_t)raw;
    a.peak = mag > a.peak ? mag : a.peak;
}
// Float formats: `c` is the component (a float widened exactly).  A NaN or an infinity is counted and takes part in nothing else.
// One select, no branch (a wave's lanes stay together): +0.0 stands in for it, and adding +0.0 changes no bit of a sum that began
// as +0.0 -- such a sum is never -0.0, the one value x + 0.0 would alter.
RT_HD void stats_component(InputStatsPart<double> &a, double c, int comp) {
    const bool finite = fabs(c) <= 1.7976931348623157e308;
    const double v = finite ? c : 0.0, mag = fabs(v);
    a.n_nonfinite += finite ? 0 : 1;
    a.n_rail += mag >= 1.0 ? 1 : 0;
    if (comp == 0) a.sum_i += v; else a.sum_q += v;
    a.sum_sq += v * v;
    a.peak = fmax(a.peak, mag);
}

// ---- the packed form of the integer rule ----
// Dot products over the four bytes of a word; the device forms are single instructions.
RT_HD uint32_t stats_udot4(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_udot4(a, b, c, false);
#else
    for (int i = 0; i < 4; ++i) c += ((a >> (8 * i)) & 255u) * ((b >> (8 * i)) & 255u);
    return c;
#endif
}
RT_HD int32_t stats_sdot4(uint32_t a, uint32_t b, int32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_sdot4((int)a, (int)b, c, false);
#else
    for (int i = 0; i < 4; ++i) c += (int32_t)(int8_t)(a >> (8 * i)) * (int32_t)(int8_t)(b >> (8 * i));
    return c;
#endif
}
// the larger of each 16-bit half
RT_HD uint32_t stats_pkmax16(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef unsigned short us2 __attribute__((ext_vector_type(2)));
    const us2 r = __builtin_elementwise_max(__builtin_bit_cast(us2, a), __builtin_bit_cast(us2, b));
    return __builtin_bit_cast(uint32_t, r);
#else
    const uint32_t lo = (a & 0xffffu) > (b & 0xffffu) ? (a & 0xffffu) : (b & 0xffffu), hi = (a >> 16) > (b >> 16) ? (a >> 16) : (b >> 16);
    return lo | (hi << 16);
#endif
}
RT_HD int stats_popc(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __popc(x);
#else
    return __builtin_popcount(x);
#endif
}
// the bytes of x that are neither 0 nor 255: add 1 to every byte without a carry between bytes, drop bit 0, count what is left
RT_HD int stats_not_rail4(uint32_t x) {
    const uint32_t y = ((x & 0x7f7f7f7fu) + 0x01010101u) ^ (x & 0x80808080u);
    const uint32_t z = y & 0xfefefefeu;
    return stats_popc((((z & 0x7f7f7f7fu) + 0x7f7f7f7fu) | z) & 0x80808080u);
}
// a byte's larger distance from the middle, per byte.  uint8: max(b, 255 - b), in 128 ... 255 (|2 b - 255| = 2 m - 255); int8: |i|,
// in 0 ... 128
template <int FMT>
RT_HD uint32_t stats_fold4(uint32_t x) {
    if (FMT == kStatsU8) {
        const uint32_t s = (~x >> 7) & 0x01010101u;  // bytes below 128
        return x ^ ((s << 8) - s);
    }
    const uint32_t s = (x >> 7) & 0x01010101u;  // negative bytes: ~i + 1, and ~i <= 127 leaves no carry
    return (x ^ ((s << 8) - s)) + s;
}

// What a thread keeps over the 16-byte pieces of a chunk of 8-bit samples.  Width: a thread takes at most
// kInputStatsChunk * 2 / 16 / kInputStatsBlock = 8 pieces = 32 words, each adding at most 4 * 255^2 to sq: < 2^24.
struct StatsWords8 {
    uint32_t si = 0, sq_ = 0, sqq = 0;  // sums over the I bytes, the Q bytes, the squares (int8: as int32)
    uint32_t not_rail = 0, pk = 0, words = 0;
};
static_assert((int64_t)kInputStatsChunk * 2 / 4 / kInputStatsBlock * 4 * 255 * 255 < (1ll << 31), "a thread's 32-bit sums hold a chunk of rails");

template <int FMT>
RT_HD void stats_word8(StatsWords8 &w, uint32_t x) {
    static_assert(FMT == kStatsU8 || FMT == kStatsI8, "8-bit formats");
    if (FMT == kStatsU8) {
        w.si = stats_udot4(x, 0x00010001u, w.si);
        w.sq_ = stats_udot4(x, 0x01000100u, w.sq_);
        w.sqq = stats_udot4(x, x, w.sqq);
        w.not_rail += (uint32_t)stats_not_rail4(x);
    } else {
        w.si = (uint32_t)stats_sdot4(x, 0x00010001u, (int32_t)w.si);
        w.sq_ = (uint32_t)stats_sdot4(x, 0x01000100u, (int32_t)w.sq_);
        w.sqq = (uint32_t)stats_sdot4(x, x, (int32_t)w.sqq);
        w.not_rail += (uint32_t)stats_not_rail4(x ^ 0x80808080u);  // -128 -> 0, 127 -> 255
    }
    const uint32_t m = stats_fold4<FMT>(x);
    w.pk = stats_pkmax16(stats_pkmax16(w.pk, m & 0x00ff00ffu), (m >> 8) & 0x00ff00ffu);
    w.words += 1;
}
// ... into the thread's row, as stats_component would have left it
template <int FMT>
RT_HD void stats_words8_close(InputStatsPart<int64_t> &a, const StatsWords8 &w) {
    if (w.words == 0) return;
    const int64_t n = (int64_t)w.words * 2;  // I bytes, and Q bytes
    const uint32_t m = (w.pk & 0xffffu) > (w.pk >> 16) ? (w.pk & 0xffffu) : (w.pk >> 16);
    int64_t peak;
    if (FMT == kStatsU8) {
        const int64_t bi = w.si, bq = w.sq_, b2 = w.sqq;  // sums of b and b^2; raw = 2 b - 255
        a.sum_i += 2 * bi - 255 * n;
        a.sum_q += 2 * bq - 255 * n;
        a.sum_sq += 4 * b2 - 4 * 255 * (bi + bq) + 255ll * 255 * 2 * n;
        peak = 2 * (int64_t)m - 255;
    } else {
        a.sum_i += (int32_t)w.si;
        a.sum_q += (int32_t)w.sq_;
        a.sum_sq += (int32_t)w.sqq;
        peak = m;
    }
    a.n_rail += 2 * n - w.not_rail;
    a.peak = peak > a.peak ? peak : a.peak;
}
// one int16 sample (I in the low half) -- plain arithmetic: I^2 + Q^2 reaches 2^31 and goes straight into 64 bits
RT_HD void stats_word16(InputStatsPart<int64_t> &a, uint32_t x) {
    stats_component<kStatsI16>(a, (int32_t)(int16_t)(x & 0xffffu), 0);
    stats_component<kStatsI16>(a, (int32_t)(int16_t)(x >> 16), 1);
}

// `n` whole samples at `p` (sample-aligned), through the rule
template <int FMT>
RT_HD void stats_samples_int(InputStatsPart<int64_t> &a, const char *p, int64_t n) {
    for (int64_t j = 0; j < n; ++j) {
        if (FMT == kStatsI16) {
            uint32_t x;
            memcpy(&x, p + 4 * j, 4);
            stats_word16(a, x);
        } else {
            const uint8_t i = (uint8_t)p[2 * j], q = (uint8_t)p[2 * j + 1];
            stats_component<FMT>(a, FMT == kStatsU8 ? (int32_t)i : (int32_t)(int8_t)i, 0);
            stats_component<FMT>(a, FMT == kStatsU8 ? (int32_t)q : (int32_t)(int8_t)q, 1);
        }
    }
}
// one aligned 16-byte piece of an integer format
template <int FMT>
RT_HD void stats_piece_int(InputStatsPart<int64_t> &a, StatsWords8 &w, const uint32_t x[4]) {
    for (int k = 0; k < 4; ++k) {
        if constexpr (FMT == kStatsI16) stats_word16(a, x[k]);
        else stats_word8<FMT>(w, x[k]);
    }
}

template <class A>
RT_HD void stats_add(InputStatsPart<A> &a, const InputStatsPart<A> &b) {
    a.n_rail += b.n_rail;
    a.n_nonfinite += b.n_nonfinite;
    a.sum_i += b.sum_i;
    a.sum_q += b.sum_q;
    a.sum_sq += b.sum_sq;
    a.peak = b.peak > a.peak ? b.peak : a.peak;
}

// The bytes [head, head + 16 * pieces) of a chunk of an integer row are its aligned 16-byte pieces; `head` and `tail` bytes (whole
// samples, < 16 each) lie in front and behind.  `begin` is the chunk's first byte, `bytes` its length.
struct StatsSplit {
    int64_t head, pieces, tail;
};
RT_HD StatsSplit stats_split(uintptr_t begin, int64_t bytes) {
    StatsSplit s;
    s.head = (int64_t)((16u - (begin & 15u)) & 15u);
    if (s.head > bytes) s.head = bytes;
    s.pieces = (bytes - s.head) / 16;
    s.tail = bytes - s.head - 16 * s.pieces;
    return s;
}

// the row rt_fetch_input_stats delivers, from a stream's folded parts
template <class A>
RT_HD void stats_row(rt_input_stats &r, const InputStatsPart<A> &t, int64_t n_samples, int fmt) {
    r.n_samples = n_samples;
    r.n_rail = t.n_rail;
    r.n_nonfinite = t.n_nonfinite;
    r.sum_i = (double)t.sum_i;
    r.sum_q = (double)t.sum_q;
    r.sum_sq = (double)t.sum_sq;
    r.peak = (double)t.peak;
    r.format = stats_public_format(fmt);
    r.unit = stats_unit(fmt);
}

// the xor butterfly over a wave's 64 rows, as the kernel's cross-lane steps run it: every lane ends with the same row
template <class A>
inline void stats_butterfly(InputStatsPart<A> *lane) {
    InputStatsPart<A> next[kInputStatsWave];
    for (int off = 1; off < kInputStatsWave; off <<= 1) {
        for (int l = 0; l < kInputStatsWave; ++l) {
            next[l] = lane[l];
            stats_add(next[l], lane[l ^ off]);
        }
        for (int l = 0; l < kInputStatsWave; ++l) lane[l] = next[l];
    }
}

// ---- the whole computation on the host, thread for thread (one stream) ----
template <int FMT>
inline void input_stats_chunk_host(const char *row, int64_t first, int64_t count, InputStatsPart<double> *out) {
    static_assert(stats_is_float(FMT), "float formats");
    constexpr int per = 16 / stats_sample_bytes(FMT);  // samples of a piece
    InputStatsPart<double> th[kInputStatsBlock];
    for (auto &t : th) stats_clear(t);
    for (int64_t j = 0; j < count; ++j) {
        InputStatsPart<double> &t = th[(j / per) % kInputStatsBlock];
        if (FMT == kStatsC64) {
            float c[2];
            memcpy(c, row + (first + j) * 8, 8);
            stats_component(t, (double)c[0], 0);
            stats_component(t, (double)c[1], 1);
        } else {
            double c[2];
            memcpy(c, row + (first + j) * 16, 16);
            stats_component(t, c[0], 0);
            stats_component(t, c[1], 1);
        }
    }
    stats_clear(*out);
    for (int w = 0; w < kInputStatsBlock / kInputStatsWave; ++w) {
        stats_butterfly(th + w * kInputStatsWave);
        stats_add(*out, th[w * kInputStatsWave]);
    }
}
template <int FMT>
inline void input_stats_chunk_host(const char *row, int64_t first, int64_t count, InputStatsPart<int64_t> *out) {
    static_assert(!stats_is_float(FMT), "integer formats");
    constexpr int bps = stats_sample_bytes(FMT);
    const char *const p = row + first * bps;
    const StatsSplit sp = stats_split(reinterpret_cast<uintptr_t>(p), count * bps);
    stats_clear(*out);
    stats_samples_int<FMT>(*out, p, sp.head / bps);
    StatsWords8 th[kInputStatsBlock];
    for (int64_t i = 0; i < sp.pieces; ++i) {
        uint32_t x[4];
        memcpy(x, p + sp.head + 16 * i, 16);
        stats_piece_int<FMT>(*out, th[i % kInputStatsBlock], x);
    }
    if constexpr (FMT != kStatsI16)
        for (const StatsWords8 &w : th) stats_words8_close<FMT>(*out, w);
    stats_samples_int<FMT>(*out, p + sp.head + 16 * sp.pieces, sp.tail / bps);
}
template <int FMT, class A>
inline void input_stats_host_fmt(const void *row, int64_t n, rt_input_stats *out) {
    InputStatsPart<A> total, part;
    stats_clear(total);
    for (int64_t first = 0; first < n; first += kInputStatsChunk) {
        input_stats_chunk_host<FMT>(static_cast<const char *>(row), first, n - first < kInputStatsChunk ? n - first : (int64_t)kInputStatsChunk, &part);
        stats_add(total, part);
    }
    stats_row(*out, total, n, FMT);
}
// fmt: kStats*; `row`: n samples, sample-aligned.  false: no such format
inline bool input_stats_host(int fmt, const void *row, int64_t n, rt_input_stats *out) {
    switch (fmt) {
    case kStatsC64: input_stats_host_fmt<kStatsC64, double>(row, n, out); return true;
    case kStatsU8: input_stats_host_fmt<kStatsU8, int64_t>(row, n, out); return true;
    case kStatsI16: input_stats_host_fmt<kStatsI16, int64_t>(row, n, out); return true;
    case kStatsI8: input_stats_host_fmt<kStatsI8, int64_t>(row, n, out); return true;
    case kStatsC128: input_stats_host_fmt<kStatsC128, double>(row, n, out); return true;
    }
    return false;
}

#if defined(__HIP__)
// ---- the kernels ----
struct InputStatsArgs {
    const char *iq;          // the call's IQ
    int64_t stream_stride;   // samples
    int64_t n_samples;       // per stream: all of them, the remainder past the last whole segment included
    int32_t n_streams;
    int32_t n_chunks;        // ceil(n_samples / kInputStatsChunk)
    const int32_t *absent;   // [S] non-zero: the stream sits the call out (null: none does)
    void *parts;             // [S][n_chunks] InputStatsPart
    rt_input_stats *rows;    // [S], pinned host memory
};

template <class A>
__device__ __forceinline__ A stats_xor(A v, int off) {
    return __shfl_xor(v, off, kInputStatsWave);
}
template <class A>
__device__ __forceinline__ void stats_wave_fold(InputStatsPart<A> &a) {
#pragma unroll
    for (int off = 1; off < kInputStatsWave; off <<= 1) {
        InputStatsPart<A> b;
        b.n_rail = stats_xor(a.n_rail, off);
        b.n_nonfinite = stats_xor(a.n_nonfinite, off);
        b.sum_i = stats_xor(a.sum_i, off);
        b.sum_q = stats_xor(a.sum_q, off);
        b.sum_sq = stats_xor(a.sum_sq, off);
        b.peak = stats_xor(a.peak, off);
        stats_add(a, b);
    }
}
// the workgroup's row: waves through LDS, added in wave order by thread 0
template <class A>
__device__ __forceinline__ void stats_block_store(InputStatsPart<A> a, InputStatsPart<A> *out) {
    constexpr int kWaves = kInputStatsBlock / kInputStatsWave;
    __shared__ InputStatsPart<A> lds[kWaves];
    stats_wave_fold(a);
    if ((threadIdx.x & (kInputStatsWave - 1)) == 0) lds[threadIdx.x / kInputStatsWave] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        InputStatsPart<A> t;
        stats_clear(t);
        for (int w = 0; w < kWaves; ++w) stats_add(t, lds[w]);
        *out = t;
    }
}

// One 16-byte piece of a float row -> its components, widened.  WIDE: the piece is 16-byte aligned (always, for complex128); else
// a complex64 piece is loaded as its two samples.
template <int FMT, bool WIDE>
__device__ __forceinline__ void stats_load_piece(const char *q, double c[4]) {
    if constexpr (FMT == kStatsC128) {
        const double2 v = *reinterpret_cast<const double2 *>(q);
        c[0] = v.x, c[1] = v.y;
    } else if constexpr (WIDE) {
        const float4 v = *reinterpret_cast<const float4 *>(q);
        c[0] = (double)v.x, c[1] = (double)v.y, c[2] = (double)v.z, c[3] = (double)v.w;
    } else {
        const float2 lo = *reinterpret_cast<const float2 *>(q), hi = *reinterpret_cast<const float2 *>(q + 8);
        c[0] = (double)lo.x, c[1] = (double)lo.y, c[2] = (double)hi.x, c[3] = (double)hi.y;
    }
}
// A thread's pieces of a chunk of a float row, in ascending order: tid, tid + kInputStatsBlock, ...
template <int FMT, bool WIDE>
__device__ __forceinline__ void stats_float_pieces(InputStatsPart<double> &acc, const char *p, int64_t count, int tid) {
    constexpr int per = 16 / stats_sample_bytes(FMT);  // samples of a piece: 2 (complex64), 1 (complex128)
    constexpr int comps = 2 * per;
    const int n_full = (int)(count / per);  // whole pieces; a complex64 chunk of an odd length ends in half a piece
    int base = tid;
    for (; base + (kInputStatsInFlight - 1) * kInputStatsBlock < n_full; base += kInputStatsBlock * kInputStatsInFlight) {
        double c[kInputStatsInFlight][4];
#pragma unroll
        for (int j = 0; j < kInputStatsInFlight; ++j) stats_load_piece<FMT, WIDE>(p + (int64_t)(base + j * kInputStatsBlock) * 16, c[j]);
#pragma unroll
        for (int j = 0; j < kInputStatsInFlight; ++j) {
#pragma unroll
            for (int k = 0; k < comps; ++k) stats_component(acc, c[j][k], k & 1);
        }
    }
    for (; base < n_full; base += kInputStatsBlock) {
        double c[4];
        stats_load_piece<FMT, WIDE>(p + (int64_t)base * 16, c);
#pragma unroll
        for (int k = 0; k < comps; ++k) stats_component(acc, c[k], k & 1);
    }
    if (FMT == kStatsC64 && (count & 1) && base == n_full) {  // (the half piece is its thread's last)
        const float2 v = *reinterpret_cast<const float2 *>(p + (int64_t)n_full * 16);
        stats_component(acc, (double)v.x, 0);
        stats_component(acc, (double)v.y, 1);
    }
}

template <int FMT>
__global__ __launch_bounds__(kInputStatsBlock) void input_stats(InputStatsArgs a) {
    using A = typename std::conditional<stats_is_float(FMT), double, int64_t>::type;
    constexpr int bps = stats_sample_bytes(FMT);
    const int s = (int)(blockIdx.x / (unsigned)a.n_chunks), chunk = (int)(blockIdx.x % (unsigned)a.n_chunks);  // grid: n_streams * n_chunks
    if (s >= a.n_streams) return;
    if (a.absent && a.absent[s]) return;
    const int64_t first = (int64_t)chunk * kInputStatsChunk;
    const int64_t count = a.n_samples - first < kInputStatsChunk ? a.n_samples - first : (int64_t)kInputStatsChunk;  // >= 1
    const char *const p = a.iq + ((int64_t)s * a.stream_stride + first) * bps;
    const int tid = (int)threadIdx.x;
    InputStatsPart<A> acc;
    stats_clear(acc);
    if constexpr (stats_is_float(FMT)) {
        // (the chunk's first byte: every piece of it is aligned alike)
        if ((reinterpret_cast<uintptr_t>(p) & 15u) == 0) stats_float_pieces<FMT, true>(acc, p, count, tid);
        else stats_float_pieces<FMT, false>(acc, p, count, tid);
    } else {
        const StatsSplit sp = stats_split(reinterpret_cast<uintptr_t>(p), count * bps);
        const int n_head = (int)(sp.head / bps), n_tail = (int)(sp.tail / bps), n_pieces = (int)sp.pieces;
        if (tid < n_head) stats_samples_int<FMT>(acc, p + (int64_t)tid * bps, 1);
        const char *const body = p + sp.head;
        StatsWords8 w;
        for (int base = tid; base < n_pieces; base += kInputStatsBlock * kInputStatsInFlight) {
            uint4 v[kInputStatsInFlight];
#pragma unroll
            for (int j = 0; j < kInputStatsInFlight; ++j) {
                const int piece = base + j * kInputStatsBlock;
                if (piece < n_pieces) v[j] = *reinterpret_cast<const uint4 *>(body + (int64_t)piece * 16);
            }
#pragma unroll
            for (int j = 0; j < kInputStatsInFlight; ++j) {
                if (base + j * kInputStatsBlock >= n_pieces) continue;
                const uint32_t x[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
                stats_piece_int<FMT>(acc, w, x);
            }
        }
        if constexpr (FMT != kStatsI16) stats_words8_close<FMT>(acc, w);
        // (the tail's samples go to the block's last threads: the head's and the tail's loads do not wait for each other)
        if (tid >= kInputStatsBlock - n_tail) stats_samples_int<FMT>(acc, body + 16 * sp.pieces + (int64_t)(tid - (kInputStatsBlock - n_tail)) * bps, 1);
    }
    stats_block_store(acc, static_cast<InputStatsPart<A> *>(a.parts) + (int64_t)s * a.n_chunks + chunk);
}

template <class A>
__global__ __launch_bounds__(kInputStatsBlock) void input_stats_fold(InputStatsArgs a, int fmt) {
    const int s = (int)(blockIdx.x * kInputStatsBlock + threadIdx.x);
    if (s >= a.n_streams) return;
    InputStatsPart<A> t;
    stats_clear(t);
    const bool absent = a.absent && a.absent[s];
    if (!absent) {
        const InputStatsPart<A> *const parts = static_cast<const InputStatsPart<A> *>(a.parts) + (int64_t)s * a.n_chunks;
        for (int c = 0; c < a.n_chunks; ++c) stats_add(t, parts[c]);
    }
    rt_input_stats r;
    stats_row(r, t, absent ? 0 : a.n_samples, fmt);
    a.rows[s] = r;
}
#endif  // __HIP__

}  // namespace rt
#endif
