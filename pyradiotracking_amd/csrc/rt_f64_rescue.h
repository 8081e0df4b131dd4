// rt_f64_rescue.h -- RT_FLAG_F64_RESCUE (include/rt_analyze.h): the streams of a map-free float64 call whose
// candidate lists overflowed, analysed again on their own inside rt_fetch_f64.  Three kernels for a LIST of streams:
//   scan_map_f64         scan_f64's transform (rt_f64_sparse.h) for the listed streams, grid n_list x n_chunks: every power of the
//                        chunk goes to the rescue map [slot][T][N], the chunk's row sums to the rescue partials
//                        [slot][n_chunks][N].  No emission, no halo segment, no tail (the call's scan has written it).  The
//                        arithmetic and its order are scan_f64's, so a cell and a partial have the bits that kernel computed; the
//                        body is restated, not shared, so that scan_f64's machine code stays what it was.
//   detect_list_f64      one thread per (listed stream, bin): the partials folded in chunk order (the row sum detect_sparse_f64
//                        formed, hence the same row mean), rt::scan_dense_row with that sum, rt::gate_run with the slot's tail as
//                        `prev`; candidates into the stream's raw area, counted in raw_count[s].
//   stats_list_f64       one workgroup per listed stream: run_stats_wave_f64 over the map cells and the tail, wave by wave.
// finalize_sparse_f64 then ranks and packs the whole call again (the other streams' raw records are still in place).
#ifndef RT_F64_RESCUE_H
#define RT_F64_RESCUE_H

#include "rt_f64_sparse.h"

namespace rt {

struct F64MapScanParams {
    const void *iq;          // [S][stream_stride] complex128, or an integer wire format
    int64_t stream_stride;   // samples
    int32_t n_seg, nperseg;
    int32_t group;           // G (f64_sparse_group)
    int32_t chunk;           // L: the handle's segments per chunk
    int32_t n_chunks;        // chunks of this call
    int32_t n_list;          // streams of this round
    const int32_t *list;     // [n_list] their stream indices
    double scale;
    const double *window;    // [N]
    const cd *tw;            // [N / 2]
    double *map;             // [n_list][T][N]
    double *partial;         // [n_list][n_chunks][N]
};

// NB, LDS: as scan_f64.
template <int FMT, int NB>
__global__ __launch_bounds__(kF64ScanBlock) void scan_map_f64(const F64MapScanParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char f64m_smem[];
    __shared__ double red[2 * (kF64ScanBlock / 64)];
    const int N = p.nperseg, G = p.group, T = p.n_seg, L = p.chunk;
    const int tid = threadIdx.x, lane = tid & 63;
    const int slot = blockIdx.x / p.n_chunks, c = blockIdx.x % p.n_chunks;
    if (slot >= p.n_list) return;
    const int s = p.list[slot];
    cd *const x = reinterpret_cast<cd *>(f64m_smem);                   // [G][N]
    double *const pw = reinterpret_cast<double *>(f64m_smem);          // [G][N] the row sums' fold (aliases x)
    double *const win = reinterpret_cast<double *>(x + (size_t)G * N);  // [N]
    cd *const tw = reinterpret_cast<cd *>(win + N);                    // [N / 2]
    const int TPS = kF64ScanBlock / G;  // threads per segment
    const int q = tid / TPS, lt = tid % TPS;
    const int half = N >> 1, quarter = N >> 2;
    cd *const xs = x + (size_t)q * N;
    for (int n = tid; n < N; n += kF64ScanBlock) win[n] = p.window[n];
    for (int n = tid; n < half; n += kF64ScanBlock) tw[n] = p.tw[n];
    const int c0 = c * L;
    const int cend = c0 + L < T ? c0 + L : T;  // the chunk's segments: [c0, cend)
    int place[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) place[i] = f64_dif_place(lt + i * TPS, N);
    double sum[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) sum[i] = 0.0;
    double *const map = p.map + (int64_t)slot * T * N;
    __syncthreads();

    for (int g = c0; g < cend; g += G) {
        const int seg = g + q;
        const bool live = seg < cend;
        cd v[NB];
        double sx = 0.0, sy = 0.0;
        const int64_t first = (int64_t)s * p.stream_stride + (int64_t)seg * N;
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            v[j] = live ? load_f64<FMT>(p.iq, first + lt + j * TPS) : cd{0.0, 0.0};
            sx += v[j].x;
            sy += v[j].y;
        }
        // the segment's sum: scan_f64's order
        for (int off = (TPS < 64 ? TPS : 64) >> 1; off > 0; off >>= 1) {
            sx += __shfl_xor(sx, off);
            sy += __shfl_xor(sy, off);
        }
        if (TPS > 64) {
            if (lane == 0) {
                red[2 * (tid >> 6)] = sx;
                red[2 * (tid >> 6) + 1] = sy;
            }
            __syncthreads();
            sx = 0.0;
            sy = 0.0;
            const int w0 = q * (TPS >> 6);
            for (int w = 0; w < (TPS >> 6); ++w) {
                sx += red[2 * (w0 + w)];
                sy += red[2 * (w0 + w) + 1];
            }
        }
        const double mx = sx / (double)N, my = sy / (double)N;
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const double w = win[lt + j * TPS];
            v[j] = cd{(v[j].x - mx) * w, (v[j].y - my) * w};
        }
        // pass 1 on the registers
#pragma unroll
        for (int u = 0; u < NB / 4; ++u) {
            const int k = lt + u * TPS;
            cd &a0 = v[u], &a1 = v[u + NB / 4], &a2 = v[u + 2 * (NB / 4)], &a3 = v[u + 3 * (NB / 4)];
            f64_dft4(a0, a1, a2, a3);
            xs[k] = a0;
            xs[k + quarter] = dmul(a1, f64_tw(tw, k, half));
            xs[k + 2 * quarter] = dmul(a2, f64_tw(tw, 2 * k, half));
            xs[k + 3 * quarter] = dmul(a3, f64_tw(tw, 3 * k, half));
        }
        __syncthreads();
        // the other passes in place
        int n = quarter;
        for (; n >= 4; n >>= 2) {
            const int m = n >> 2, step = N / n;
#pragma unroll
            for (int u = 0; u < NB / 4; ++u) {
                const int b = lt + u * TPS;
                const int k = b & (m - 1);
                const int i0 = (b / m) * n + k;
                cd a0 = xs[i0], a1 = xs[i0 + m], a2 = xs[i0 + 2 * m], a3 = xs[i0 + 3 * m];
                f64_dft4(a0, a1, a2, a3);
                xs[i0] = a0;
                xs[i0 + m] = dmul(a1, f64_tw(tw, k * step, half));
                xs[i0 + 2 * m] = dmul(a2, f64_tw(tw, 2 * k * step, half));
                xs[i0 + 3 * m] = dmul(a3, f64_tw(tw, 3 * k * step, half));
            }
            __syncthreads();
        }
        if (n == 2) {
#pragma unroll
            for (int u = 0; u < NB / 2; ++u) {
                const int i0 = 2 * (lt + u * TPS);
                const cd a0 = xs[i0], a1 = xs[i0 + 1];
                xs[i0] = dadd(a0, a1);
                xs[i0 + 1] = dsub(a0, a1);
            }
            __syncthreads();
        }
        // the powers: row sums, and the segment's map row (a thread's bins lt + i TPS: for each i the segment's threads write
        // TPS neighbouring doubles)
        double *const dst = live ? map + (int64_t)seg * N : nullptr;
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const cd z = xs[place[i]];
            const double re2 = z.x * z.x, im2 = z.y * z.y;
            const double pwr = (re2 + im2) * p.scale;
            if (live) {
                sum[i] += pwr;
                dst[lt + i * TPS] = pwr;
            }
        }
        __syncthreads();  // (the next group's pass 1 writes over the transform)
    }
    // the chunk's row sums: the G segment columns of a bin in order, as scan_f64 folds them
#pragma unroll
    for (int i = 0; i < NB; ++i) pw[(size_t)q * N + lt + i * TPS] = sum[i];
    __syncthreads();
    double *const pdst = p.partial + ((int64_t)slot * p.n_chunks + c) * N;
    for (int k = tid; k < N; k += kF64ScanBlock) {
        double acc = 0.0;
        for (int r = 0; r < G; ++r) acc += pw[(size_t)r * N + k];
        pdst[k] = acc;
    }
}

// ---- detection of the listed streams from the rescue map ----
struct F64ListArgs {
    F64DetectArgs a;         // thresholds, the tail as `prev`, the raw area (a.spec: the rescue map [n_list][T][F])
    const int32_t *list;     // [n_list]
    int32_t n_list;
    const double *partial;   // [n_list][n_chunks][F]
    int32_t n_chunks;
};

__global__ __launch_bounds__(256) void detect_list_f64(const F64ListArgs la) {
    const F64DetectArgs &a = la.a;
    const int F = a.n_bins;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)la.n_list * F) return;
    const int slot = (int)(i / F), fi = (int)(i % F);
    const int s = la.list[slot];
    const DetectParams64 dp = f64_stream_params(a, s);
    // the row sum: the chunks' partials in chunk order, as detect_sparse_f64 folds them
    const double *src = la.partial + (int64_t)slot * la.n_chunks * F + fi;
    double rsum = 0.0;
    for (int c = 0; c < la.n_chunks; ++c) rsum += src[(int64_t)c * F];
    const double *row = a.spec + (int64_t)slot * dp.n_seg * F + fi;
    const F64Prev prev{a.prev ? a.prev + ((int64_t)s * a.prev_cols + a.prev_cols) * F + fi : nullptr, F};
    auto cur = [&](int t) -> double { return row[(int64_t)t * F]; };
    double avg = 0.0;
    auto on_run = [&](int b, int e, double av) {
        int start;
        if (!gate_run(dp, b, e, av, prev, &start)) return;
        const int k = atomicAdd(&a.raw_count[s], 1);
        if (k >= a.rec_cap) return;  // (counted: the fetch grows the capacity and analyses the call again)
        rt_record_f64 r{};
        r.stream = s;
        r.fi = fi;
        r.start = start;
        r.end = e;
        r.row_mean = av;
        a.raw[(int64_t)s * a.rec_cap + k] = r;
    };
    scan_dense_row(dp, cur, rsum, &avg, on_run);
}

__global__ __launch_bounds__(256) void stats_list_f64(const F64ListArgs la) {
    const F64DetectArgs &a = la.a;
    const int slot = blockIdx.x, tid = threadIdx.x;
    const int s = la.list[slot];
    const int F = a.n_bins;
    const int wanted = a.raw_count[s];
    const int n = wanted < a.rec_cap ? wanted : a.rec_cap;
    rt_record_f64 *raw = a.raw + (int64_t)s * a.rec_cap;
    const double *sp = a.spec + (int64_t)slot * a.dp.n_seg * F;
    for (int c = tid >> 6; c < n; c += 4) {
        rt_record_f64 &r = raw[c];
        const int start = r.start;
        const double *row = sp + r.fi;
        const F64Prev prev{a.prev ? a.prev + ((int64_t)s * a.prev_cols + a.prev_cols) * F + r.fi : nullptr, F};
        auto cell = [&](int k) -> double {
            const int t = start + k;
            return t < 0 ? prev(-t) : row[(int64_t)t * F];
        };
        const RunStatsT<double> st = run_stats_wave_f64(r.end - start, cell);
        if ((tid & 63) == 0) {
            r.max_p = st.max_p;
            r.mean_p = st.mean_p;
            r.std_db = st.std_db;
        }
    }
}

}  // namespace rt
#endif
