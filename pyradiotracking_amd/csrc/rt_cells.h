// rt_cells.h -- RT_FLAG_RECORD_CELLS: the spectrogram cells behind every record of a call (the reference's `data`,
// analyze.py:437-440), gathered behind the call's detection into a per-slot device pool for rt_fetch_record_cells[_f64]
// (include/rt_analyze.h).  Three small launches per analysis, only on a handle created with the flag:
//   cells_stream_totals  a workgroup per stream: its final records from the pinned host pool into device memory (the stream's
//                        raw-record area, free by then) in whole words, and the cells they hold (sum of end - start)
//   cells_stream_bases   one workgroup: exclusive prefix over the streams -> each stream's first cell in the pool, the call's
//                        total to pinned host memory (the fetch grows the pool from it and analyses the call again)
//   cells_gather         a workgroup per stream, a wave per record: the cells themselves, from where the detection read them --
//                        the dense map (detect_dense, the partial dense re-run's streams, the float64 map), or the stream's
//                        candidate lists (sparse levels), and the look-back tail for segments of the previous buffer.
// The cells lie in delivery order -- streams ascending, a stream's records in (fi, start) order -- so the host derives the
// offsets from the records it delivered.  Nothing here touches a detect or scan kernel: the gather reads the FINAL records.
#ifndef RT_CELLS_H
#define RT_CELLS_H

namespace rt {

template <class P, class Rec>
struct CellsArgs {
    const Rec *records;          // the call's final records (float32: the slot's pinned pool; float64: its packed output)
    const int32_t *rec_off;      // [S] each stream's first record there (float64: [S + 1], packed)
    const int32_t *rec_cnt;      // [S] its records, or null: rec_off[s + 1] - rec_off[s]
    Rec *stage;                  // [S][rec_cap] device copy of each stream's final records (the slot's raw-record area: its unordered
    int32_t rec_cap;             //     lists are spent once finalize_records / detect_dense / finalize_f64 has published them)
    int32_t n_streams, n_bins, n_seg;
    const P *spec;               // dense map [.][T][F] (indexed by stream, or by the position in stream_list), or null: the candidate lists
    const int32_t *stream_list;  // null, or the n_list streams `spec` holds (partial dense re-run); every other stream: its lists
    int32_t n_list;
    const P *prev;               // [S][prev_cols][F] the look-back tail the call read
    int32_t prev_cols;
    const uint2 *hot;            // [S][kBuckets][hot_cap] candidate cells (key = bin << tbits | t, power bits) ...
    const uint32_t *hot_count;   // [S][kBuckets] ... and how many: the copy taken in front of finalize_records, which zeroes the counters
    int32_t hot_cap, tbits;
    long long *stream_cells;     // [S] cells of each stream's records
    long long *stream_base;      // [S] its first cell in `cells`
    P *cells;                    // the slot's pool
    long long cell_cap;          // cells it holds
    unsigned long long *info;    // pinned host: [0] cells the call wants, [1] non-zero: a record's cells were not all on its list
};

// (in front of finalize_records on a handle with the flag: the per-bucket counters it is about to put back to zero)
__global__ __launch_bounds__(256) void cells_keep_counts(const uint32_t *src, uint32_t *dst, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

template <class P, class Rec>
__device__ __forceinline__ int cells_records_of(const CellsArgs<P, Rec> &a, int s, int *off) {
    *off = a.rec_off[s];
    return a.rec_cnt ? a.rec_cnt[s] : a.rec_off[s + 1] - a.rec_off[s];
}

// The records live in pinned host memory, where the detection publishes them: read there field by field they cost a round
// trip over the host link per access (5.9 % of config 5's share).  Here they cross it once, in consecutive 8-byte words.
template <class P, class Rec>
__global__ __launch_bounds__(256) void cells_stream_totals(const CellsArgs<P, Rec> a) {
    static_assert(sizeof(Rec) % 8 == 0, "records are copied in 8-byte words");
    __shared__ long long part[4];
    const int s = blockIdx.x, tid = threadIdx.x;
    int off;
    const int n = cells_records_of(a, s, &off);
    Rec *mine = a.stage + (int64_t)s * a.rec_cap;
    {
        const unsigned long long *src = reinterpret_cast<const unsigned long long *>(a.records + (int64_t)off);
        unsigned long long *dst = reinterpret_cast<unsigned long long *>(mine);
        const int words = n * (int)(sizeof(Rec) / 8);
        for (int w = tid; w < words; w += 256) dst[w] = src[w];
    }
    __threadfence_block();
    __syncthreads();
    long long sum = 0;
    for (int i = tid; i < n; i += 256) sum += (long long)(mine[i].end - mine[i].start);
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if ((tid & 63) == 0) part[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) a.stream_cells[s] = part[0] + part[1] + part[2] + part[3];
}

constexpr int kCellsScanBlock = 1024;
__global__ __launch_bounds__(kCellsScanBlock) void cells_stream_bases(const long long *stream_cells, long long *stream_base, int n_streams,
                                                                      unsigned long long *info) {
    __shared__ long long sh[kCellsScanBlock];
    const int tid = threadIdx.x;
    const int per = (n_streams + kCellsScanBlock - 1) / kCellsScanBlock;
    const int s0 = tid * per < n_streams ? tid * per : n_streams;
    const int s1 = s0 + per < n_streams ? s0 + per : n_streams;
    long long sum = 0;
    for (int s = s0; s < s1; ++s) sum += stream_cells[s];
    sh[tid] = sum;
    __syncthreads();
    for (int o = 1; o < kCellsScanBlock; o <<= 1) {
        const long long v = tid >= o ? sh[tid - o] : 0;
        __syncthreads();
        sh[tid] += v;
        __syncthreads();
    }
    long long base = sh[tid] - sum;
    for (int s = s0; s < s1; ++s) {
        stream_base[s] = base;
        base += stream_cells[s];
    }
    if (tid == kCellsScanBlock - 1) {
        info[0] = (unsigned long long)sh[tid];
        info[1] = 0ull;
    }
}

template <class P, class Rec>
__global__ __launch_bounds__(256) void cells_gather(const CellsArgs<P, Rec> a) {
    __shared__ int t_fi[256], t_start[256], t_len[256], sc[256];
    __shared__ long long t_off[256];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int F = a.n_bins;
    int off;
    const int n = cells_records_of(a, s, &off);
    if (n == 0) return;
    const Rec *recs = a.stage + (int64_t)s * a.rec_cap;
    // the stream's rows of a dense map, or (pos < 0) its candidate lists
    int pos = -1;
    if (a.spec) {
        if (a.stream_list) {
            for (int j = 0; j < a.n_list; ++j)
                if (a.stream_list[j] == s) pos = j;
        } else {
            pos = s;
        }
    }
    const P *map = pos >= 0 ? a.spec + (int64_t)pos * a.n_seg * F : nullptr;
    const P *prev = a.prev + (int64_t)s * a.prev_cols * F;
    long long carry = a.stream_base[s];
    for (int i0 = 0; i0 < n; i0 += 256) {
        // this tile's records and their places: an exclusive prefix over their lengths behind the tiles before
        const int i = i0 + tid;
        int len = 0;
        if (i < n) {
            const Rec &r = recs[i];
            t_fi[tid] = r.fi;
            t_start[tid] = r.start;
            len = r.end - r.start;
        }
        t_len[tid] = len;
        sc[tid] = len;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {
            const int v = tid >= o ? sc[tid - o] : 0;
            __syncthreads();
            sc[tid] += v;
            __syncthreads();
        }
        t_off[tid] = carry + (long long)(sc[tid] - len);
        carry += (long long)sc[255];
        __syncthreads();
        const int nt = n - i0 < 256 ? n - i0 : 256;
        for (int c = wave; c < nt; c += 4) {  // a wave per record
            const int fi = t_fi[c], start = t_start[c], ln = t_len[c];
            const long long o = t_off[c];
            if (o + ln > a.cell_cap) continue;  // (the pool is too small: info[0] tells the fetch, which grows it and analyses the call again)
            P *dst = a.cells + o;
            if (map) {
                for (int k = lane; k < ln; k += 64) dst[k] = record_cell(map, prev, a.prev_cols, F, fi, start + k);
                continue;
            }
            if constexpr (sizeof(P) == sizeof(float)) {
                // segments of the previous buffer from the look-back tail, the others from the bin's candidate list: the scan emits a
                // cell iff it reaches the absolute threshold or directly precedes one that does, and every cell of `data` is one
                // or the other.  The list is unordered: the wave strides over it, a lane that meets one of the record's cells stores it.
                const int neg = start < 0 ? (-start < ln ? -start : ln) : 0;
                for (int k = lane; k < neg; k += 64) dst[k] = record_cell(map, prev, a.prev_cols, F, fi, start + k);
                const int b = fi & (kBuckets - 1);
                uint32_t cnt = a.hot_count[s * kBuckets + b];
                if (cnt > (uint32_t)a.hot_cap) cnt = (uint32_t)a.hot_cap;
                const uint2 *lst = a.hot + ((int64_t)s * kBuckets + b) * a.hot_cap;
                const uint32_t tmask = (1u << a.tbits) - 1u;
                const int t0 = start + neg, end = start + ln;
                int found = 0;
                for (uint32_t j0 = 0; j0 < cnt; j0 += 64) {
                    const uint32_t j = j0 + (uint32_t)lane;
                    bool hit = false;
                    if (j < cnt) {
                        const uint2 e = lst[j];
                        const int t = (int)(e.x & tmask);
                        hit = (int)(e.x >> a.tbits) == fi && t >= t0 && t < end;
                        if (hit) dst[t - start] = __uint_as_float(e.y);
                    }
                    found += __builtin_popcountll(__builtin_amdgcn_ballot_w64(hit));
                }
                if (found != end - t0 && lane == 0) a.info[1] = 1ull;  // (cannot happen while the emission rule holds: no garbage is delivered)
            }
        }
        __syncthreads();
    }
}

}  // namespace rt
#endif
