// rt_present.h -- device side of rt_set_present (include/rt_analyze.h): what a stream that sits out a call needs done for it.
// The scans and the detection leave such a stream alone (their launches run over lists of the present streams -- rt_kernels.h: StftParams::stream_list --; DetectArgs::absent);
// the bookkeeping is host code (rt_core.h: PresenceBook).  What is left is the rotation of the look-back tails: call k reads
// buffer (k - 1) % 3 and writes k % 3 for ALL streams, so the K columns of a stream the scan does not write are carried over.
#ifndef RT_PRESENT_H
#define RT_PRESENT_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rt {

constexpr int kCarryBlock = 256;
constexpr int kCarryPerThread = 4;  // elements a thread copies

// blocks per absent stream for `per_stream` = K * N elements (>= 1: K >= 1 and N >= 8 on every handle; enqueue_carry launches nothing otherwise)
inline int carry_blocks(int64_t per_stream) { return (int)((per_stream + kCarryBlock * kCarryPerThread - 1) / (kCarryBlock * kCarryPerThread)); }

// dst[s] = src[s] ([K][N] each) for the `n_list` streams of `list`.  On the call's scan stream, where the scan's own tail stores
// are: behind everything that still reads `dst` (the call three back), ahead of everything that reads it next.
template <class P>
__global__ __launch_bounds__(kCarryBlock) void carry_tails(const int32_t *list, int n_list, int blocks_per_stream, const P *src, P *dst, int64_t per_stream) {
    const int pos = (int)blockIdx.x / blocks_per_stream;
    if (pos >= n_list) return;
    const int64_t base = (int64_t)list[pos] * per_stream;
    const int64_t i0 = (int64_t)((int)blockIdx.x % blocks_per_stream) * (kCarryBlock * kCarryPerThread) + threadIdx.x;
#pragma unroll
    for (int j = 0; j < kCarryPerThread; ++j) {
        const int64_t i = i0 + (int64_t)j * kCarryBlock;
        if (i < per_stream) dst[base + i] = src[base + i];
    }
}

}  // namespace rt
#endif
