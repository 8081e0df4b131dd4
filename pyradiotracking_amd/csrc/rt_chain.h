// rt_chain.h -- device side of rt_set_chain (include/rt_analyze.h): the look-back columns of a chained call.
// The streams of a chained handle are consecutive buffers of a recording (rt_core.h: ChainBook), so the detection of stream s
// looks back into ANOTHER stream's K columns: the ones this call's scan has just written for s's predecessor, or -- a run's first
// present stream -- the ones the rotation carries for the run's last stream of an earlier call.  The detection kernels take their
// look-back through one pointer and index it by their own stream (DetectArgs::prev), so the columns are copied, per call, into a
// buffer of the call's slot laid out as the rotation's buffers are ([S][K][N]); the detection reads that buffer as `prev`.
// Behind every scan of the call on the scan's stream, in front of every detection of it.
#ifndef RT_CHAIN_H
#define RT_CHAIN_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_core.h"

namespace rt {

constexpr int kChainBlock = 256;
constexpr int kChainVecs = 2;  // 16-byte pieces a thread copies: both loads in flight before the first store
// elements of P a workgroup copies (8 KiB: six workgroups per stream at 48 columns of 256 float bins, so a few dozen streams fill the chip)
template <class P>
constexpr int64_t chain_per_block() { return (int64_t)kChainBlock * kChainVecs * (16 / (int)sizeof(P)); }
template <class P>
inline int chain_blocks(int64_t per_stream) { return (int)((per_stream + chain_per_block<P>() - 1) / chain_per_block<P>()); }

template <class P>
struct alignas(16) ChainVec {
    P v[16 / sizeof(P)];
};

// dst[s] = (src_buf[s] == kChainWritten ? written : read)[src_idx[s]], [K][N] = `per_stream` elements each, for every stream s
// with src_buf[s] != kChainNone.  A wave copies whole 128-byte lines (64 lanes x 16 bytes, consecutive) while per_stream is a
// multiple of 16 bytes -- every buffer is a hipMalloc of its own, so each stream's block is then 16-byte aligned --, else element
// by element.  Plain loads and stores: the copy is read by the detection launched next, which finds it in the L2 it was stored
// through; a non-temporal store keeps the line there as well and a non-temporal load only passes L1, so neither hint buys anything.
template <class P>
__global__ __launch_bounds__(kChainBlock) void chain_tails(const int32_t *__restrict__ src_buf, const int32_t *__restrict__ src_idx, int n_streams,
                                                           int blocks_per_stream, const P *__restrict__ written, const P *__restrict__ read,
                                                           P *__restrict__ dst, int64_t per_stream) {
    const int s = (int)blockIdx.x / blocks_per_stream;
    if (s >= n_streams) return;
    const int32_t which = src_buf[s];
    if (which == kChainNone) return;
    const int32_t from = src_idx[s];
    if (from < 0 || from >= n_streams) return;
    const P *const src = (which == kChainWritten ? written : read) + (int64_t)from * per_stream;
    P *const out = dst + (int64_t)s * per_stream;
    const int64_t e0 = (int64_t)((int)blockIdx.x % blocks_per_stream) * chain_per_block<P>();
    constexpr int kPer = 16 / (int)sizeof(P);
    if (per_stream % kPer == 0) {
        const int64_t n_vec = per_stream / kPer;
        const int64_t v0 = e0 / kPer + threadIdx.x;
        const ChainVec<P> *const sv = reinterpret_cast<const ChainVec<P> *>(src);
        ChainVec<P> *const dv = reinterpret_cast<ChainVec<P> *>(out);
        ChainVec<P> r[kChainVecs];
#pragma unroll
        for (int j = 0; j < kChainVecs; ++j) {
            const int64_t i = v0 + (int64_t)j * kChainBlock;
            if (i < n_vec) r[j] = sv[i];
        }
#pragma unroll
        for (int j = 0; j < kChainVecs; ++j) {
            const int64_t i = v0 + (int64_t)j * kChainBlock;
            if (i < n_vec) dv[i] = r[j];
        }
    } else {
        for (int64_t i = e0 + threadIdx.x; i < e0 + chain_per_block<P>() && i < per_stream; i += kChainBlock) out[i] = src[i];
    }
}

}  // namespace rt
#endif
