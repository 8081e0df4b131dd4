// rt_record_iq.h -- device side of rt_set_record_iq / rt_fetch_record_iq (include/rt_analyze.h): the two streaming kernels that
// move raw sample bytes.  What they copy is decided on the host (rt_record_iq_book.h: IqTailBook, iq_build_descs).
//   iq_tails           at enqueue, on the scan's stream, in front of the scan: the last min(T, K + m) whole segments of every
//                      present stream's row -> that stream's tail row, as the bytes the caller passed.
//   record_iq_gather   inside rt_fetch, once the call's record list stands: a variable-length segmented copy from the call's IQ
//                      rows and the tail rows into the slot's byte pool, one descriptor per contiguous piece.
// Both copy in tiles of kIqTileBytes, one workgroup per tile, so that one long record next to thousands of short ones does not
// serialise (tile -> descriptor by binary search over the tile prefix).  A tile whose source, destination and length are multiples
// of 16 bytes moves as 16-byte pieces, four loads of a thread in flight before its first store; any other tile (a uint8 / int8 row
// need only be 2-byte aligned, and the stride is free) moves in the widest unit of 8, 4 or 2 bytes that divides all three.
// Plain loads and stores: the tails are read once, a call later, and the pool is read by a copy to the host -- a pure copy gains
// nothing from the non-temporal forms (as rt_chain.h: chain_tails).
#ifndef RT_RECORD_IQ_H
#define RT_RECORD_IQ_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_record_iq_book.h"

namespace rt {

constexpr int kIqBlock = 256;
constexpr int kIqVecs = 4;  // units of a thread in flight: all loads before the first store
static_assert((int64_t)kIqBlock * kIqVecs * 16 == kIqTileBytes, "one pass of 16-byte pieces covers a tile");

template <class U>
__device__ __forceinline__ void iq_copy_units(const char *__restrict__ src, char *__restrict__ dst, int64_t bytes) {
    const U *const s = reinterpret_cast<const U *>(src);
    U *const d = reinterpret_cast<U *>(dst);
    const int64_t n = bytes / (int64_t)sizeof(U);
    for (int64_t base = threadIdx.x; base < n; base += (int64_t)kIqBlock * kIqVecs) {
        U r[kIqVecs];
#pragma unroll
        for (int j = 0; j < kIqVecs; ++j) {
            const int64_t i = base + (int64_t)j * kIqBlock;
            if (i < n) r[j] = s[i];
        }
#pragma unroll
        for (int j = 0; j < kIqVecs; ++j) {
            const int64_t i = base + (int64_t)j * kIqBlock;
            if (i < n) d[i] = r[j];
        }
    }
}

// `bytes` (even, <= kIqTileBytes) from src to dst by the whole workgroup; both at least 2-byte aligned
__device__ __forceinline__ void iq_copy_tile(const char *src, char *dst, int64_t bytes) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst) | (uintptr_t)bytes;
    if ((a & 15u) == 0)
        iq_copy_units<uint4>(src, dst, bytes);
    else if ((a & 7u) == 0)
        iq_copy_units<uint2>(src, dst, bytes);
    else if ((a & 3u) == 0)
        iq_copy_units<uint32_t>(src, dst, bytes);
    else
        iq_copy_units<uint16_t>(src, dst, bytes);
}

struct IqTailsArgs {
    const char *iq;            // the call's IQ
    int64_t stream_stride;     // samples
    int32_t bps;               // bytes per sample
    int32_t n_streams;
    int64_t src_sample;        // (T - D) * N: the first sample kept
    int64_t bytes;             // D * N * bps: bytes kept per stream
    int32_t tiles_per_stream;  // ceil(bytes / kIqTileBytes)
    const int32_t *write_buf;  // [S] the row each stream writes, -1: none
    char *tails;               // [kIqRows][S][row_bytes]
    int64_t row_bytes;
};

__global__ __launch_bounds__(kIqBlock) void iq_tails(IqTailsArgs a) {
    const int s = (int)(blockIdx.x / (unsigned)a.tiles_per_stream);
    if (s >= a.n_streams) return;
    const int32_t buf = a.write_buf[s];
    if (buf < 0 || buf >= kIqRows) return;
    const int64_t off = (int64_t)(blockIdx.x % (unsigned)a.tiles_per_stream) * kIqTileBytes;
    if (off >= a.bytes) return;
    const int64_t n = a.bytes - off < kIqTileBytes ? a.bytes - off : kIqTileBytes;
    const char *const src = a.iq + ((int64_t)s * a.stream_stride + a.src_sample) * a.bps + off;
    char *const dst = a.tails + ((int64_t)buf * a.n_streams + s) * a.row_bytes + off;
    iq_copy_tile(src, dst, n);
}

struct IqGatherArgs {
    const IqDesc *descs;
    const int64_t *tile_first;  // [n_descs + 1]
    int32_t n_descs;
    int32_t bps;
    int32_t n_streams;
    const char *iq;  // the call's IQ
    int64_t stream_stride;
    const char *tails;
    int64_t row_bytes;
    char *pool;
};

__global__ __launch_bounds__(kIqBlock) void record_iq_gather(IqGatherArgs a) {
    const int64_t tile = (int64_t)blockIdx.x;
    if (tile >= a.tile_first[a.n_descs]) return;
    // the last descriptor whose first tile is not behind this one (descriptors hold at least one tile each)
    int lo = 0, hi = a.n_descs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.tile_first[mid] <= tile) lo = mid; else hi = mid - 1;
    }
    const IqDesc d = a.descs[lo];
    const int64_t total = d.len * a.bps;
    const int64_t off = (tile - a.tile_first[lo]) * kIqTileBytes;
    if (off >= total || d.row < 0 || d.row >= a.n_streams) return;
    const int64_t n = total - off < kIqTileBytes ? total - off : kIqTileBytes;
    const char *src;
    if (d.kind == kIqFromTail) {
        if (d.buf < 0 || d.buf >= kIqRows) return;
        src = a.tails + ((int64_t)d.buf * a.n_streams + d.row) * a.row_bytes + d.src_sample * a.bps;
    } else {
        src = a.iq + ((int64_t)d.row * a.stream_stride + d.src_sample) * a.bps;
    }
    iq_copy_tile(src + off, a.pool + d.dst_sample * a.bps + off, n);
}

}  // namespace rt
#endif
