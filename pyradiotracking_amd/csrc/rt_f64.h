// rt_f64.h -- the float64 analysis path of a handle made by rt_create_f64 (include/rt_analyze.h): the reference's arithmetic on
// the complex128 buffers pyrtlsdr delivers (SciPy keeps the input dtype; thresholds and statistics are Python floats).
// Dense path only, three kernels per call:
//   stft_f64       x -> float64 segment mean subtracted -> float64 window -> FFT in double (radix-2 in LDS; other sizes by
//                  Bluestein's algorithm on it) -> (re^2 + im^2) * scale  (scipy _spectral_py.py:2185-2202, 2126-2128),
//                  written as the float64 map [S][T][N] plus the look-back tail [S][K][N];
//   detect_f64     one thread per (stream, bin) row: the row's float64 sum and mean, then its runs of above-cells gated by the
//                  rt_core.h predicates instantiated on double (rt::scan_dense_row, gate_run); candidates into the stream's
//                  unordered raw area;
//   finalize_f64   one workgroup per stream: plateau statistics wave by wave (rt::run_stats' order), (fi, start) rank and shadow
//                  verdict (rt::rank_and_shadow in float64), the stream's records packed behind those of the streams before it.
// Traffic per sample (dense call, no records): 16 B complex128 read + 8 B map write + 8 B map read by the row scan (+ 8 B more for
// rows that hold a cell at or above the absolute threshold: their second pass).
#ifndef RT_F64_H
#define RT_F64_H

#include "rt_kernels.h"

namespace rt {

// (struct cd, two doubles: rt_core.h)
__device__ __forceinline__ cd dadd(cd a, cd b) { return cd{a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ cd dsub(cd a, cd b) { return cd{a.x - b.x, a.y - b.y}; }
__device__ __forceinline__ cd dmul(cd a, cd b) { return cd{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }

constexpr int kF64Block = 256;
constexpr int kF64MaxM = 8192;  // LDS transform length at most: 8192 complex doubles = 128 KiB of the CU's 160 KiB
constexpr int kF64MaxN = 4096;  // every nperseg up to here (Bluestein: M >= 2 N - 1), beyond it the powers of two up to kF64MaxM

struct F64StftParams {
    const void *iq;          // [S][stream_stride] complex128, or interleaved uint8 I/Q
    int64_t stream_stride;   // samples
    int32_t n_streams, n_seg, nperseg;
    int32_t m, log2m;        // LDS transform length (nperseg, or Bluestein's M) and its log2
    int32_t segs_per_block;  // SPB segments per workgroup (M * SPB <= 1024 where M < 1024)
    int32_t tail_cols;       // K
    double scale;            // 1/(fs*sum(w*w)) in float64
    const double *window;    // [N] float64 window (powers of two)
    const cd *cwin;          // [N] window * exp(-i pi n^2 / N) (Bluestein)
    const cd *bfilt;         // [M] FFT_M of the chirp filter / M, bit-reversed order (Bluestein)
    const cd *tw;            // [M / 2] W_M^j  (these three: rt_tables.h, bluestein_tables / transform_twiddles in long double)
    double *spec;            // [S][T][N]
    double *tail;            // [S][K][N], or null
    const int32_t *absent;   // [S] non-zero: the stream sits this call out (rt_set_present) -- its workgroups end at once; or null
};

// One segment's sample n in float64: complex128 as it is; a wire-format byte pair as pyrtlsdr converts it (packed_bytes_to_iq:
// `iq /= 127.5; iq -= 1 + 1j` -- a division by (127.5 + 0j) is the real division, then the subtraction; no fma, -ffp-contract=off)
// An int16 pair is component / 32768: the conversion and the multiplication by 2^-15 are exact.  An int8 pair is component / 128, as exact.
template <int FMT>
__device__ __forceinline__ cd load_f64(const void *base, int64_t i) {
    if constexpr (FMT == kFmtU8) {
        const uint16_t b = reinterpret_cast<const uint16_t *>(base)[i];  // low byte I, high byte Q
        return cd{(double)(b & 0xFFu) / 127.5 - 1.0, (double)(b >> 8) / 127.5 - 1.0};
    } else if constexpr (FMT == kFmtI16) {
        const uint32_t b = reinterpret_cast<const uint32_t *>(base)[i];  // low half I, high half Q
        return cd{(double)(int16_t)(b & 0xFFFFu) * (1.0 / 32768.0), (double)((int32_t)b >> 16) * (1.0 / 32768.0)};
    } else if constexpr (FMT == kFmtI8) {
        const uint16_t b = reinterpret_cast<const uint16_t *>(base)[i];  // low byte I, high byte Q
        return cd{(double)(int8_t)(b & 0xFFu) * (1.0 / 128.0), (double)((int16_t)b >> 8) * (1.0 / 128.0)};
    } else {
        const double2 v = reinterpret_cast<const double2 *>(base)[i];
        return cd{v.x, v.y};
    }
}

// Radix-2 stages on the M complex doubles at xs (in LDS), one stage per barrier; `lt` of TPS threads of this segment work.
// DIT: input at bit-reversed places, natural order out.  DIF: natural order in, bit-reversed out (twiddles behind the differences).
__device__ __forceinline__ void f64_fft_dit(cd *xs, int M, int LOG, const cd *tw, int lt, int TPS) {
    for (int st = 0; st < LOG; ++st) {
        const int h = 1 << st;
        const int step = M >> (st + 1);  // W_(2 h)^k = W_M^(k M / (2 h))
        for (int b = lt; b < M / 2; b += TPS) {
            const int k = b & (h - 1);
            const int i0 = ((b >> st) << (st + 1)) | k;
            const cd u = xs[i0], v = dmul(xs[i0 + h], tw[k * step]);
            xs[i0] = dadd(u, v);
            xs[i0 + h] = dsub(u, v);
        }
        __syncthreads();
    }
}
__device__ __forceinline__ void f64_fft_dif(cd *xs, int M, int LOG, const cd *tw, int lt, int TPS) {
    for (int st = LOG - 1; st >= 0; --st) {
        const int h = 1 << st;
        const int step = M >> (st + 1);
        for (int b = lt; b < M / 2; b += TPS) {
            const int k = b & (h - 1);
            const int i0 = ((b >> st) << (st + 1)) | k;
            const cd u = xs[i0], v = xs[i0 + h];
            xs[i0] = dadd(u, v);
            xs[i0 + h] = dmul(dsub(u, v), tw[k * step]);
        }
        __syncthreads();
    }
}

// SPB segments per workgroup of kF64Block threads (TPS = kF64Block / SPB threads each); M * SPB complex doubles of dynamic LDS.
// BLU = false: nperseg = M is a power of two.  BLU = true: Bluestein -- A = DIF_M((x - mean) * cwin, zero-padded) (bit-reversed),
// conj(A * bfilt) in place, DIT_M of that = FFT(conj(C)), whose first N values have the spectrum's magnitudes (rt_general.h).
template <int FMT, bool BLU>
__global__ __launch_bounds__(kF64Block) void stft_f64(const F64StftParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char f64_smem[];
    cd *const x = reinterpret_cast<cd *>(f64_smem);  // [SPB][M]
    __shared__ double red[2 * kF64Block];
    const int N = p.nperseg, M = p.m, LOG = p.log2m, SPB = p.segs_per_block, T = p.n_seg;
    const int tid = threadIdx.x;
    const int blocks_per_stream = (T + SPB - 1) / SPB;
    const int s = blockIdx.x / blocks_per_stream;
    const int seg0 = (blockIdx.x % blocks_per_stream) * SPB;
    if (s >= p.n_streams) return;
    if (p.absent && p.absent[s] != 0) return;  // (workgroup-uniform, ahead of the first barrier)
    const int TPS = kF64Block / SPB;
    const int q = tid / TPS, lt = tid % TPS;
    cd *const xs = x + (int64_t)q * M;
    const int seg = seg0 + q;
    const bool live = seg < T;
    const int64_t first = (int64_t)s * p.stream_stride + (int64_t)seg * N;

    // samples -> LDS (bit-reversed places for the DIT transform, natural ones for Bluestein's DIF), their float64 sums
    double sx = 0.0, sy = 0.0;
    if (live) {
        for (int n = lt; n < N; n += TPS) {
            const cd v = load_f64<FMT>(p.iq, first + n);
            sx += v.x;
            sy += v.y;
            xs[BLU ? n : (int)(__brev((unsigned)n) >> (32 - LOG))] = v;
        }
    }
    red[2 * tid] = sx;
    red[2 * tid + 1] = sy;
    __syncthreads();
    double tx = 0.0, ty = 0.0;  // the segment's sum: its TPS partial sums in a fixed order
    for (int j = 0; j < TPS; ++j) {
        tx += red[2 * (q * TPS + j)];
        ty += red[2 * (q * TPS + j) + 1];
    }
    const double mx = tx / (double)N, my = ty / (double)N;  // np.mean (detrend='constant', scipy _signaltools.py:3926)
    if (live) {
        if constexpr (BLU) {
            for (int n = lt; n < M; n += TPS)
                xs[n] = n < N ? dmul(cd{xs[n].x - mx, xs[n].y - my}, p.cwin[n]) : cd{0.0, 0.0};
        } else {
            for (int n = lt; n < N; n += TPS) {
                const int at = (int)(__brev((unsigned)n) >> (32 - LOG));
                const double w = p.window[n];  // (float64 window times complex128: (w + 0i)(a + bi) = w a + i w b exactly)
                xs[at] = cd{(xs[at].x - mx) * w, (xs[at].y - my) * w};
            }
        }
    }
    __syncthreads();
    if constexpr (BLU) {
        f64_fft_dif(xs, M, LOG, p.tw, lt, TPS);
        if (live)
            for (int j = lt; j < M; j += TPS) {
                const cd c = dmul(xs[j], p.bfilt[j]);
                xs[j] = cd{c.x, -c.y};
            }
        __syncthreads();
    }
    f64_fft_dit(xs, M, LOG, p.tw, lt, TPS);
    // conj(X) X = re^2 + im^2 (the imaginary part cancels exactly), then * scale (_spectral_py.py:2126-2128)
    if (live) {
        double *dst = p.spec + ((int64_t)s * T + seg) * N;
        const int col = seg - (T - p.tail_cols);
        double *tdst = (p.tail && col >= 0) ? p.tail + ((int64_t)s * p.tail_cols + col) * N : nullptr;
        for (int k = lt; k < N; k += TPS) {
            const cd v = xs[k];
            const double re2 = v.x * v.x, im2 = v.y * v.y;
            const double pw = (re2 + im2) * p.scale;
            dst[k] = pw;
            if (tdst) tdst[k] = pw;
        }
    }
}

// ---- detection ----
struct F64DetectArgs {
    DetectParams64 dp;          // n_seg_last / thresholds per stream from the arrays below
    const double *spec;         // [S][T][F]
    const double *prev;         // [S][prev_cols][F]: the previous buffer's last prev_cols columns (look-back), or null
    int32_t prev_cols;
    int32_t n_streams, n_bins;  // S, F
    const int32_t *no_last;     // [S] non-zero: the stream has no previous buffer in this call, or null
    const double *thr_s;        // [S] per-stream thresholds, or null
    const double *cal_s;        // [S] per-stream calibrations, or null
    const StreamSettings64 *set_s;  // [S] per-stream snr_threshold, duration gates and probe stride (rt_set_stream_settings_f64), or null
    rt_record_f64 *raw;         // [S][rec_cap] unordered candidates
    int32_t *raw_count;         // [S] candidates each stream found (may exceed rec_cap: the fetch then grows it); zeroed by finalize_f64
    int32_t rec_cap;
    rt_record_f64 *out;         // the call's records, ordered by (stream, fi, start): stream s from out_off[s]
    int32_t *out_off;           // [S + 1] each stream's first record in `out`, and the total
    int32_t *out_count;         // [S] records each stream wanted (copied to the host behind the call)
    double *row_means;          // RT_FLAG_ROW_MEANS: [S][F] every row's mean (the call slot's device buffer), written by detect_f64<true> only
    // a handle whose streams may sit out a call (rt_set_present; null on every other handle)
    const int32_t *absent;        // [S] non-zero: the stream is absent from this call -- no records, NaN row means
    const int32_t *n_seg_last_s;  // [S] columns of each stream's OWN previous buffer (-1: none -- takes no_last's place)
    int32_t tail_k;               // ... and K, the columns the look-back tail holds
};

__device__ __forceinline__ DetectParams64 f64_stream_params(const F64DetectArgs &a, int s) {
    DetectParams64 dp = a.dp;
    if (a.no_last && a.no_last[s]) {
        dp.n_seg_last = -1;
        dp.tail_cols = 0;
    }
    if (a.n_seg_last_s) {
        const int32_t n = a.n_seg_last_s[s];
        dp.n_seg_last = n;
        dp.tail_cols = n < 0 ? 0 : (n < a.tail_k ? n : a.tail_k);
    }
    if (a.thr_s) dp.thr = a.thr_s[s];
    if (a.cal_s) dp.cal_db = a.cal_s[s];
    if (a.set_s) apply_stream_settings(dp, a.set_s[s]);
    return dp;
}

struct F64Prev {
    const double *base;  // the stream's look-back at its bin, one past its last column
    int stride;
    __device__ double operator()(int d) const { return base[-(int64_t)d * stride]; }
};

// One thread per (stream, bin): rt::scan_dense_row on float64 cells (neighbouring threads read neighbouring bins: whole lines),
// each run through rt::gate_run; a plateau goes to the stream's raw area with its start, end and the row mean.
// ROW_MEANS (RT_FLAG_ROW_MEANS): every row's mean -- from the sum scan_dense_row forms anyway -- to a.row_means as well.
template <bool ROW_MEANS>
__global__ __launch_bounds__(256) void detect_f64(const F64DetectArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)a.n_streams * a.n_bins) return;
    const int s = (int)(i / a.n_bins), fi = (int)(i % a.n_bins);
    const int F = a.n_bins;
    if (a.absent && a.absent[s] != 0) {  // the stream sat this call out: no row (its raw counter stays zero), NaN as at T == 0
        if constexpr (ROW_MEANS) a.row_means[i] = NAN;
        return;
    }
    const DetectParams64 dp = f64_stream_params(a, s);
    const double *row = a.spec + (int64_t)s * dp.n_seg * F + fi;
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
    if constexpr (ROW_MEANS) {
        double sum = 0.0;
        scan_dense_row(dp, cur, -1.0, &avg, on_run, &sum);
        a.row_means[i] = row_mean_of(sum, dp.n_seg, double());  // (the record's row_mean: the same expression on the same sum)
    } else {
        scan_dense_row(dp, cur, -1.0, &avg, on_run);
    }
}

// np.max / np.mean / np.std(dB(.)) of one plateau by one wave: rt::run_stats' 64 interleaved partials and halving fold, in float64
template <class Cell>
__device__ __forceinline__ RunStatsT<double> run_stats_wave_f64(int n, Cell cell) {
    const int lane = threadIdx.x & 63;
    double ps = 0.0, pd = 0.0, pm = -INFINITY;
    int any_nan = 0;
    for (int k = lane; k < n; k += 64) {
        const double v = cell(k);
        ps += v;
        pd += db10(v);
        if (v != v) any_nan = 1;
        if (v > pm) pm = v;
    }
    const auto add64 = [](double x, double y) { return x + y; };
    ps = butterfly_all(ps, add64);
    pd = butterfly_all(pd, add64);
    pm = butterfly_all(pm, [](double x, double y) { return y > x ? y : x; });
    any_nan = butterfly_all(any_nan, [](int x, int y) { return x | y; });
    const double mean_db = pd / (double)n;
    double pa = 0.0;
    for (int k = lane; k < n; k += 64) {
        const double d = db10(cell(k)) - mean_db;
        pa += d * d;
    }
    pa = butterfly_all(pa, add64);
    RunStatsT<double> r;
    r.max_p = any_nan ? (double)NAN : pm;
    r.mean_p = ps / (double)n;
    r.std_db = sqrt(pa / (double)n);
    return r;
}

// One workgroup per stream: statistics, then rank in (fi, start) order and the shadow verdict against the unfiltered list
// (analyze.py:315-328; maxima as float64 dBW figures), written packed behind the records of the streams before it.
__global__ __launch_bounds__(256) void finalize_f64(const F64DetectArgs a) {
    __shared__ int sh_off;
    __shared__ int sh_part[256];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int wanted = a.raw_count[s];
    const int n = wanted < a.rec_cap ? wanted : a.rec_cap;
    // this stream's place in `out`: the records of the streams before it (their counts are final: detect_f64 ran before)
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
    const int off = sh_off;
    if (n == 0) return;
    const DetectParams64 dp = f64_stream_params(a, s);
    const int F = a.n_bins;
    rt_record_f64 *raw = a.raw + (int64_t)s * a.rec_cap;
    const double *sp = a.spec + (int64_t)s * dp.n_seg * F;
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
    __threadfence_block();
    __syncthreads();
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

// The raw counters back to zero for the slot's next call (behind finalize_f64, which reads all of them)
__global__ __launch_bounds__(256) void clear_counts_f64(int32_t *raw_count, int n_streams) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n_streams) raw_count[i] = 0;
}

}  // namespace rt
#endif
