// rt_record_spectrum.h -- device side of rt_fetch_record_spectrum (include/rt_analyze.h): record_spectrum<P, HW>, one row of
// rt_record_spectrum per record, and the record's mean and peak per column, from the frames record_band left in the slot's band
// pool, [n_frames][B] with B = 2 w + 1 (P: float or double frames).  The plan is the host's (rt_record_stft_book.h: EstimatesWork):
// the frame prefix, lp and each part's run of inside frames.
//
// One wave per record, kStftWaves waves a workgroup, as record_estimates.  Everything is float64, whatever P, and the library is
// built without contraction, so every product and sum below rounds once -- tests/record_spectrum_cases.py restates the order.
//   p        re * re + im * im of a column's value, the components widened first
//   frames   the inside frames are numbered i = 0, 1, ...: part 0's run, then part 1's.  Lane l takes i = l, l + 64, ... in
//            increasing i, so a lane's accumulator is the canonical partial l (partial i mod 64) of every column.  The lanes of a
//            wave read neighbouring frames: one block of 64 B values of the pool a round, each lane a run of B values at a stride of
//            B values, the block's cache lines met again by every column of the loop.
//   columns  the sums and the maxima are arrays of 2 HW + 1 with every index a constant after unrolling (registers, no scratch);
//            HW = 0, 2 or 8 is the smallest bound that holds w (stft_band_bound), and the columns from B on are not loaded.
//   fold     est_wave_sum's butterfly (xor 32 ... 1) for the sums, the same butterfly for the maxima: every lane holds the same
//            bits.  A maximum takes the other value where that is larger or NaN, so a NaN stays (numpy.max's rule).
//   mean     sum / n_inside; a NaN mean or peak is stored as the one quiet NaN
//   scalars  from the means, left to right with d_j = j - w: see rt_analyze.h; log is the device library's
// Lane 0 stores the 48-byte row; lanes 0 .. B - 1 store the row's B means and B peaks, one value a lane.  No LDS, no scratch, no
// atomics (profiles/record_spectrum_kernel_resources.txt).
#ifndef RT_RECORD_SPECTRUM_H
#define RT_RECORD_SPECTRUM_H

#include "rt_record_band.h"
#include "rt_record_estimates.h"

namespace rt {

template <class P>
struct SpectrumArgs {
    const typename stft_types<P>::C *values;  // the band pool: [n_frames][2 w + 1]
    const int64_t *frame_first;  // [n_records + 1]
    const int32_t *range;        // [n_records][4]
    const int32_t *lp;           // [n_records]
    int32_t n_records;
    int32_t hop_div;
    int32_t half_width;          // w: 0 .. 8
    int64_t n_frames;            // frame_first[n_records]: no frame is read behind it
    rt_record_spectrum *rows;    // [n_records]
    double *mean;                // [n_records][2 w + 1]
    double *peak;                // [n_records][2 w + 1]
};

// the larger of two, a NaN before either (numpy.max)
__device__ __forceinline__ double spec_max(double a, double b) { return (b > a || b != b) ? b : a; }

__device__ __forceinline__ double spec_wave_max(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = spec_max(v, __shfl_xor(v, m, 64));
    return v;
}

template <class P, int HW>
__global__ __launch_bounds__(kStftBlock) void record_spectrum(SpectrumArgs<P> a) {
    using C = typename stft_types<P>::C;
    constexpr int BT = 2 * HW + 1;  // columns this instantiation carries
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = (int)(threadIdx.x & 63u);
    const int64_t r = (int64_t)blockIdx.x * kStftWaves + wave;
    if (r >= a.n_records) return;
    const int w = a.half_width, B = 2 * w + 1, k = a.hop_div;
    if (w < 0 || w > HW || k < 1) return;
    const int64_t f0 = a.frame_first[r], f1 = a.frame_first[r + 1];
    const int F = (int)(f1 - f0);
    const int Lp = a.lp[r], Fp = Lp > 0 ? (Lp - 1) * k + 1 : 0;
    const int lo0 = a.range[4 * r], hi0 = a.range[4 * r + 1], lo1 = a.range[4 * r + 2], hi1 = a.range[4 * r + 3];
    // (the host refuses such a plan: estimates_build_work)
    if (f0 < 0 || f1 < f0 || f1 > a.n_frames || f1 - f0 > 0x7fffffffll || Fp > F || lo0 < 0 || lo0 > hi0 || hi0 > Fp || lo1 < Fp || lo1 > hi1 || hi1 > F) return;
    const C *const v = a.values + f0 * (int64_t)B;
    const double nan = __builtin_nan("");
    const int n0 = hi0 - lo0, n_in = n0 + (hi1 - lo1);

    // ---- the partials: lane l is partial l of every column
    double sum[BT], top[BT];
#pragma unroll
    for (int c = 0; c < BT; ++c) {
        sum[c] = 0.0;
        top[c] = -__builtin_inf();
    }
    for (int64_t i = lane; i < n_in; i += 64) {
        const int64_t frame = i < n0 ? lo0 + i : lo1 + (i - n0);  // inside number -> frame
        const C *const f = v + frame * (int64_t)B;
#pragma unroll
        for (int c = 0; c < BT; ++c) {
            if (c < B) {
                const C x = f[c];
                const double re = (double)x.x, im = (double)x.y;
                const double p = re * re + im * im;
                sum[c] += p;
                top[c] = spec_max(top[c], p);
            }
        }
    }
    // ---- the fold, the means
    double m[BT];
    bool any_nan = false;
#pragma unroll
    for (int c = 0; c < BT; ++c) {
        if (c < B) {
            const double s = est_wave_sum(sum[c]);
            top[c] = spec_wave_max(top[c]);
            m[c] = n_in > 0 ? s / (double)n_in : nan;
            if (m[c] != m[c]) m[c] = nan;
            if (top[c] != top[c] || n_in == 0) top[c] = nan;
            any_nan |= m[c] != m[c];
        } else {
            m[c] = 0.0;
            top[c] = 0.0;
        }
    }
    // ---- the scalars, left to right
    rt_record_spectrum row;
    row.total = row.centre_share = row.centroid = row.width = row.peak_bins = nan;
    row.peak_col = -1;
    row.n_inside = n_in;
    if (!any_nan) {
        double total = 0.0, moment = 0.0, centre = 0.0, best = m[0];
        int col = 0;
#pragma unroll
        for (int c = 0; c < BT; ++c) {
            if (c < B) {
                total += m[c];
                moment += m[c] * (double)(c - w);
                if (c == w) centre = m[c];
                if (c > 0 && m[c] > best) {
                    best = m[c];
                    col = c;
                }
            }
        }
        const double centroid = moment / total;
        double spread = 0.0, left = 0.0, right = 0.0;
#pragma unroll
        for (int c = 0; c < BT; ++c) {
            if (c < B) {
                const double t = (double)(c - w) - centroid;
                spread += m[c] * (t * t);
                if (c == col - 1) left = m[c];
                if (c == col + 1) right = m[c];
            }
        }
        row.total = total;
        row.centre_share = centre / total;
        row.centroid = centroid;
        row.width = sqrt(spread / total);
        row.peak_col = col;
        const auto usable = [](double x) { return x > 0.0 && x < __builtin_inf(); };
        if (col > 0 && col < 2 * w && usable(left) && usable(best) && usable(right)) {
            const double la = log(left), lb = log(best), lc = log(right);
            row.peak_bins = (double)(col - w) + 0.5 * (la - lc) / ((la - 2.0 * lb) + lc);
        }
    }
    if (lane == 0) a.rows[r] = row;
    // ---- the row's means and peaks: lane c holds column c
    double mine = m[0], high = top[0];
#pragma unroll
    for (int c = 1; c < BT; ++c) {
        if (lane == c) {
            mine = m[c];
            high = top[c];
        }
    }
    if (lane < B) {
        a.mean[r * (int64_t)B + lane] = mine;
        a.peak[r * (int64_t)B + lane] = high;
    }
}

}  // namespace rt
#endif
