// rt_f64_sparse.h -- the map-free path of a float64 handle (RT_FLAG_F64_SPARSE, include/rt_analyze.h).  Two kernels
// and the shared record packing per call, no [S][T][N] map:
//   scan_f64           a workgroup walks a chunk of L consecutive segments of one stream, G segments side by side (G * nperseg =
//                      1024 samples up to nperseg 1024, one segment beyond): float64 segment mean subtracted, float64 window,
//                      radix-4 transform (first pass on the loaded registers, the others in place in LDS, one barrier a pass; a
//                      last radix-2 pass where log2 nperseg is odd), (re^2 + im^2) * scale.  A thread owns the same bins in every
//                      segment: its row sums stay in registers and go to the per-chunk partials [S][chunks][N]; cells of the last
//                      K segments go to the look-back tail as in stft_f64; a cell is emitted to its stream's list iff it or its
//                      successor in time is not below the stream's absolute threshold (a halo segment, transformed but neither
//                      summed nor emitted, gives the last segment of a chunk its successor).
//   detect_sparse_f64  one workgroup per stream: the partials folded in chunk order (the row sums, every row's mean), the list
//                      sorted by (bin, segment) in LDS, runs through rt::sparse_run_at and rt::gate_run, statistics by
//                      run_stats_wave_f64 on the sorted cells and the tail;
//   finalize_sparse_f64  rank, shadow verdict and packing as in finalize_f64 (rt_f64.h).
// Traffic per sample: 16 B complex128 read (2 or 4 B for the integer formats); 8 B / L for the partials; the tail and the
// candidate cells beside it.
#ifndef RT_F64_SPARSE_H
#define RT_F64_SPARSE_H

#include "rt_f64.h"

namespace rt {

struct F64ScanParams {
    const void *iq;          // [S][stream_stride] complex128, or an integer wire format
    int64_t stream_stride;   // samples
    int32_t n_streams, n_seg, nperseg;
    int32_t group;           // G: segments a workgroup transforms side by side (f64_sparse_group)
    int32_t chunk;           // L: segments per chunk
    int32_t n_chunks;        // chunks of this call: f64_sparse_chunks(n_seg, L)
    int32_t chunk_cap;       // chunks per stream the partials have room for
    int32_t tail_cols;       // K
    int32_t hot_cap;         // cells per stream the lists have room for
    double scale;            // 1/(fs*sum(w*w)) in float64
    double thr;              // the absolute threshold, or per stream:
    const double *thr_s;     // [S], or null
    const double *window;    // [N]
    const cd *tw;            // [N / 2] W_N^j (rt_tables.h: transform_twiddles in long double)
    double *tail;            // [S][K][N]
    const int32_t *absent;   // [S] non-zero: the stream sits this call out; or null
    double *partial;         // [S][chunk_cap][N] row sums per chunk
    uint32_t *keys;          // [S][hot_cap] f64_cell_key of the stream's candidate cells, in no particular order
    double *vals;            // [S][hot_cap] their powers
    int32_t *count;          // [S] cells each stream emitted (counted past hot_cap, never written past it)
};

// W_N^j for 0 <= j < N from the half table (W_N^(j + N/2) = -W_N^j, exactly)
__device__ __forceinline__ cd f64_tw(const cd *tw, int j, int half) {
    if (j < half) return tw[j];
    const cd w = tw[j - half];
    return cd{-w.x, -w.y};
}

// forward 4-point transform of a[0..3] in place
__device__ __forceinline__ void f64_dft4(cd &a0, cd &a1, cd &a2, cd &a3) {
    const cd s02 = dadd(a0, a2), d02 = dsub(a0, a2), s13 = dadd(a1, a3), d13 = dsub(a1, a3);
    const cd md{d13.y, -d13.x};  // -i (a1 - a3)
    a0 = dadd(s02, s13);
    a1 = dadd(d02, md);
    a2 = dsub(s02, s13);
    a3 = dsub(d02, md);
}

// Where bin k of a length-N transform lies after the in-place decimation-in-frequency passes (radix 4, a last radix 2 where
// log2 N is odd): a pass of radix r on blocks of n leaves the bins = q (mod r) of each block in its q-th part of n / r.
__device__ __forceinline__ int f64_dif_place(int k, int N) {
    int p = 0, rem = N;
    while (rem >= 4) {
        rem >>= 2;
        p += (k & 3) * rem;
        k >>= 2;
    }
    if (rem == 2) p += k & 1;
    return p;
}

// NB = bins (and samples) a thread holds per segment: nperseg * G / 256 = 4 up to nperseg 1024, 8 at 2048, 16 at 4096.
// Dynamic LDS: G * N complex doubles (the transform; afterwards the powers' exchange and the row sums' fold), N doubles of
// window, N / 2 complex doubles of twiddles = 16 N (G + 1) bytes.
template <int FMT, int NB>
__global__ __launch_bounds__(kF64ScanBlock) void scan_f64(const F64ScanParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char f64s_smem[];
    __shared__ double red[2 * (kF64ScanBlock / 64)];
    const int N = p.nperseg, G = p.group, T = p.n_seg, L = p.chunk;
    const int tid = threadIdx.x, lane = tid & 63;
    const int s = blockIdx.x / p.n_chunks, c = blockIdx.x % p.n_chunks;
    if (s >= p.n_streams) return;
    if (p.absent && p.absent[s] != 0) return;  // (workgroup-uniform, ahead of the first barrier)
    cd *const x = reinterpret_cast<cd *>(f64s_smem);                   // [G][N]
    double *const pw = reinterpret_cast<double *>(f64s_smem);          // [G + 1][N] powers, after a group's transform (aliases x)
    double *const win = reinterpret_cast<double *>(x + (size_t)G * N);  // [N]
    cd *const tw = reinterpret_cast<cd *>(win + N);                    // [N / 2]
    const int TPS = kF64ScanBlock / G;  // threads per segment
    const int q = tid / TPS, lt = tid % TPS;
    const int half = N >> 1, quarter = N >> 2;
    cd *const xs = x + (size_t)q * N;
    for (int n = tid; n < N; n += kF64ScanBlock) win[n] = p.window[n];
    for (int n = tid; n < half; n += kF64ScanBlock) tw[n] = p.tw[n];
    const double thr = p.thr_s ? p.thr_s[s] : p.thr;
    const int c0 = c * L;
    const int cend = c0 + L < T ? c0 + L : T;         // the chunk's own segments: [c0, cend)
    const int hend = cend + 1 < T ? cend + 1 : T;     // ... and its halo segment, where the buffer has one
    int place[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) place[i] = f64_dif_place(lt + i * TPS, N);
    double sum[NB], before[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        sum[i] = 0.0;
        before[i] = 0.0;
    }
    uint32_t *const keys = p.keys + (int64_t)s * p.hot_cap;
    double *const vals = p.vals + (int64_t)s * p.hot_cap;
    __syncthreads();

    for (int g = c0; g < cend + 1; g += G) {
        const int seg = g + q;
        const bool live = seg < hend;
        // samples n = lt + j TPS into registers, their float64 sums
        cd v[NB];
        double sx = 0.0, sy = 0.0;
        const int64_t first = (int64_t)s * p.stream_stride + (int64_t)seg * N;
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            v[j] = live ? load_f64<FMT>(p.iq, first + lt + j * TPS) : cd{0.0, 0.0};
            sx += v[j].x;
            sy += v[j].y;
        }
        // the segment's sum: a butterfly over the lanes of the segment (every lane the same bits: x + y = y + x), then its waves
        // in order
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
        const double mx = sx / (double)N, my = sy / (double)N;  // np.mean (detrend='constant')
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const double w = win[lt + j * TPS];
            v[j] = cd{(v[j].x - mx) * w, (v[j].y - my) * w};
        }
        // pass 1 on the registers: butterfly u holds the samples k + m N / 4, k = lt + u TPS
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
        // the other passes in place: blocks of n, butterflies over n / 4
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
        // conj(X) X = re^2 + im^2, then * scale (_spectral_py.py:2126-2128); sums and tail for the chunk's own segments
        double pwr[NB];
        const bool own = seg < cend;
        const int col = seg - (T - p.tail_cols);
        double *const tdst = (own && col >= 0) ? p.tail + ((int64_t)s * p.tail_cols + col) * N : nullptr;
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const cd z = xs[place[i]];
            const double re2 = z.x * z.x, im2 = z.y * z.y;
            pwr[i] = (re2 + im2) * p.scale;
            if (own) sum[i] += pwr[i];
            if (tdst) tdst[lt + i * TPS] = pwr[i];
        }
        __syncthreads();
        // the powers side by side: row r + 1 = segment g + r, row 0 = the group before's last segment
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            pw[(size_t)(q + 1) * N + lt + i * TPS] = pwr[i];
            if (q == G - 1) pw[lt + i * TPS] = before[i];
        }
        __syncthreads();
        // cell (bin, seg - 1), whose successor this thread holds: emitted iff one of the two is not below the threshold
        const int t = seg - 1;
        const bool mine = t >= c0 && t < cend;
        const bool has_next = seg < T;
        double cell[NB];
        unsigned emit = 0u;
        int ne = 0;
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            cell[i] = pw[(size_t)q * N + lt + i * TPS];
            const bool hot = mine && (!(cell[i] < thr) || (has_next && !(pwr[i] < thr)));
            if (hot) {
                emit |= 1u << i;
                ++ne;
            }
            before[i] = pwr[i];
        }
        // one returned atomic per wave and group: the wave's cells behind each other in the stream's list
        int incl = ne;
        for (int off = 1; off < 64; off <<= 1) {
            const int up = __shfl_up(incl, off);
            if (lane >= off) incl += up;
        }
        const int total = __shfl(incl, 63);
        if (total > 0) {
            int base = 0;
            if (lane == 0) base = atomicAdd(&p.count[s], total);
            base = __shfl(base, 0);
            int at = base + incl - ne;
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                if (emit & (1u << i)) {
                    if (at < p.hot_cap) {
                        keys[at] = f64_cell_key(lt + i * TPS, t);
                        vals[at] = cell[i];
                    }
                    ++at;
                }
            }
        }
        __syncthreads();  // (the next group's pass 1 writes over the powers)
    }
    // the chunk's row sums: the G segment columns of a bin in order
#pragma unroll
    for (int i = 0; i < NB; ++i) pw[(size_t)q * N + lt + i * TPS] = sum[i];
    __syncthreads();
    double *const dst = p.partial + ((int64_t)s * p.chunk_cap + c) * N;
    for (int k = tid; k < N; k += kF64ScanBlock) {
        double acc = 0.0;
        for (int r = 0; r < G; ++r) acc += pw[(size_t)r * N + k];
        dst[k] = acc;
    }
}

// ---- detection from the lists ----
struct F64SparseArgs {
    F64DetectArgs a;         // thresholds, the tail as `prev`, the raw area and the outputs (a.spec is not used)
    const double *partial;   // [S][chunk_cap][N]
    int32_t n_chunks, chunk_cap;
    double *row_sums;        // [S][N] scratch: the folded sums
    const uint32_t *keys;    // [S][hot_cap]
    const double *vals;
    const int32_t *count;    // [S]
    int32_t hot_cap;
    int32_t sort_cap;        // next power of two >= hot_cap: the LDS arrays' length
    int32_t *hot_out;        // [S] pinned: the cells each stream emitted (> hot_cap: the call has no result)
};

// Dynamic LDS: sort_cap keys (uint32) and sort_cap powers (double).
template <bool ROW_MEANS>
__global__ __launch_bounds__(256) void detect_sparse_f64(const F64SparseArgs sa) {
    extern __shared__ __attribute__((aligned(16))) unsigned char f64d_smem[];
    __shared__ int sh_rec;
    const F64DetectArgs &a = sa.a;
    const int s = blockIdx.x, tid = threadIdx.x;
    const int F = a.n_bins;
    if (a.absent && a.absent[s] != 0) {  // the stream sat this call out: no records, NaN row means
        if constexpr (ROW_MEANS)
            for (int k = tid; k < F; k += 256) a.row_means[(int64_t)s * F + k] = NAN;
        if (tid == 0) sa.hot_out[s] = 0;
        return;
    }
    const DetectParams64 dp = f64_stream_params(a, s);
    // the row sums: the chunks' partials in chunk order
    double *const rs = sa.row_sums + (int64_t)s * F;
    for (int k = tid; k < F; k += 256) {
        const double *src = sa.partial + (int64_t)s * sa.chunk_cap * F + k;
        double acc = 0.0;
        for (int c = 0; c < sa.n_chunks; ++c) acc += src[(int64_t)c * F];
        rs[k] = acc;
        if constexpr (ROW_MEANS) a.row_means[(int64_t)s * F + k] = row_mean_of(acc, dp.n_seg, double());
    }
    const int n = sa.count[s];
    if (tid == 0) {
        sa.hot_out[s] = n;
        sh_rec = 0;
    }
    if (n == 0 || n > sa.hot_cap) return;  // (more than the list holds: rt_fetch_f64 reports RT_E_HOT_OVERFLOW)
    double *const sval = reinterpret_cast<double *>(f64d_smem);            // [sort_cap]
    uint32_t *const skey = reinterpret_cast<uint32_t *>(sval + sa.sort_cap);  // [sort_cap]
    int M = 1;
    while (M < n) M <<= 1;  // (the lengths at their edges, up to hot_cap and one past it: tests/detect_order_cases.py)
    for (int j = tid; j < M; j += 256) {
        skey[j] = j < n ? sa.keys[(int64_t)s * sa.hot_cap + j] : 0xFFFFFFFFu;
        sval[j] = j < n ? sa.vals[(int64_t)s * sa.hot_cap + j] : 0.0;
    }
    __threadfence_block();
    __syncthreads();
    // bitonic sort by key (the keys of a list are distinct: a cell has one owner)
    for (int kk = 2; kk <= M; kk <<= 1)
        for (int jj = kk >> 1; jj > 0; jj >>= 1) {
            for (int i = tid; i < M; i += 256) {
                const int l = i ^ jj;
                if (l > i) {
                    const uint32_t ka = skey[i], kb = skey[l];
                    const bool up = (i & kk) == 0;
                    if ((ka > kb) == up) {
                        skey[i] = kb;
                        skey[l] = ka;
                        const double va = sval[i];
                        sval[i] = sval[l];
                        sval[l] = va;
                    }
                }
            }
            __syncthreads();
        }
    // runs: the entry a run begins on gates it
    auto keys = [&](int j) -> uint32_t { return skey[j]; };
    auto vals = [&](int j) -> double { return sval[j]; };
    rt_record_f64 *raw = a.raw + (int64_t)s * a.rec_cap;
    for (int j = tid; j < n; j += 256) {
        const int fi = f64_key_bin(skey[j]);
        const double avg = row_mean_of(rs[fi], dp.n_seg, double());
        int b, e, start;
        if (!sparse_run_at(dp, keys, vals, n, j, avg, &b, &e)) continue;
        const F64Prev prev{a.prev ? a.prev + ((int64_t)s * a.prev_cols + a.prev_cols) * F + fi : nullptr, F};
        if (!gate_run(dp, b, e, avg, prev, &start)) continue;
        const int k = atomicAdd(&sh_rec, 1);
        if (k >= a.rec_cap) continue;  // (counted: the fetch grows the capacity and analyses the call again)
        rt_record_f64 r{};
        r.stream = s;
        r.fi = fi;
        r.start = start;
        r.end = e;
        r.row_mean = avg;
        r.reserved = j - b;  // the list entry of the bin's segment 0, were it there (finalize_sparse_f64 clears the field)
        raw[k] = r;
    }
    __threadfence_block();
    __syncthreads();
    const int wanted = sh_rec;
    if (tid == 0) a.raw_count[s] = wanted;
    const int nrec = wanted < a.rec_cap ? wanted : a.rec_cap;
    for (int c = tid >> 6; c < nrec; c += 4) {
        rt_record_f64 &r = raw[c];
        const int start = r.start, at0 = r.reserved;
        const F64Prev prev{a.prev ? a.prev + ((int64_t)s * a.prev_cols + a.prev_cols) * F + r.fi : nullptr, F};
        auto cell = [&](int k) -> double {
            const int t = start + k;
            return t < 0 ? prev(-t) : sval[at0 + t];
        };
        const RunStatsT<double> st = run_stats_wave_f64(r.end - start, cell);
        if ((tid & 63) == 0) {
            r.max_p = st.max_p;
            r.mean_p = st.mean_p;
            r.std_db = st.std_db;
        }
    }
}

// finalize_f64 (rt_f64.h) without its statistics pass: detect_sparse_f64 has written them.  The steps are restated here, not shared:
// with either a statistics functor or a common ranking function, finalize_f64 compiled to other machine code than before (two
// instructions changed places), and the dense handle's kernels stay as they are.
__global__ __launch_bounds__(256) void finalize_sparse_f64(const F64DetectArgs a) {
    __shared__ int sh_off;
    __shared__ int sh_part[256];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int wanted = a.raw_count[s];
    const int n = wanted < a.rec_cap ? wanted : a.rec_cap;
    // this stream's place in `out`, as in finalize_f64: the records of the streams before it
    int part = 0;
    for (int j = tid; j < s; j += 256) {
        const int c = a.raw_count[j];
        part += c < a.rec_cap ? c : a.rec_cap;
    }
    sh_part[tid] = part;
    __syncthreads();
    if (tid == 0) {
        int off = 0;
        for (int j = 0; j < 256; ++j) off += sh_part[j];
        sh_off = off;
        a.out_off[s] = off;
        a.out_count[s] = wanted;
        if (s == a.n_streams - 1) a.out_off[a.n_streams] = off + n;
    }
    __syncthreads();
    if (n == 0) return;
    const DetectParams64 dp = f64_stream_params(a, s);
    const rt_record_f64 *raw = a.raw + (int64_t)s * a.rec_cap;
    const int off = sh_off;
    for (int i = tid; i < n; i += 256) {
        rt_record_f64 mine = raw[i];
        const long long ts_i = timedelta_us(start_time(dp, mine.start));
        const long long dur_i = timedelta_us(run_duration(dp, mine.start, mine.end));
        const double mx_i = db10(mine.max_p) - dp.cal_db;
        int rank = 0, shadow = 0;
        for (int j = 0; j < n; ++j) {
            const rt_record_f64 &rj = raw[j];
            if (rj.fi < mine.fi || (rj.fi == mine.fi && rj.start < mine.start)) ++rank;
            const long long ts_j = timedelta_us(start_time(dp, rj.start));
            const long long dur_j = timedelta_us(run_duration(dp, rj.start, rj.end));
            if (shadowed_by(ts_i, dur_i, mx_i, ts_j, dur_j, db10(rj.max_p) - dp.cal_db)) shadow = 1;
        }
        mine.shadowed = shadow;
        mine.reserved = 0;
        a.out[off + rank] = mine;
    }
}

// The list and raw counters back to zero for the slot's next call (behind finalize_sparse_f64)
__global__ __launch_bounds__(256) void clear_counts_sparse_f64(int32_t *raw_count, int32_t *cell_count, int n_streams) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n_streams) {
        raw_count[i] = 0;
        cell_count[i] = 0;
    }
}

}  // namespace rt
#endif
