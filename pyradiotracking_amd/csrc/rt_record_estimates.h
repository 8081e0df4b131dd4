// rt_record_estimates.h -- device side of rt_fetch_record_estimates (include/rt_analyze.h): record_estimates<P>, one row of
// rt_record_estimate per record from the frames record_stft_hop left in the slot's hop pool (P: float or double frames).  The plan
// is the host's (rt_record_stft_book.h: EstimatesWork): the frame prefix, lp, each part's run of inside frames, each part's
// position base and fi mod k; the turn-back table sits in front of it.
//
// One wave per record, kStftWaves waves a workgroup.  Everything is float64, whatever P, and the library is built without
// contraction, so every product and sum below rounds once -- tests/record_estimates_cases.py restates the order in NumPy.
//   |c|      sqrt(re * re + im * im); +inf where a component is infinite, whatever the other (hypot's rule: numpy.abs gives that)
//   pairs    a part's run [lo, hi) has the pairs (t, t + 1), lo <= t < hi - 1.  Lane l takes t = lo + l, lo + l + 64, ... of part 0,
//            then of part 1, into three accumulators (re, im of c[t + 1] conj(c[t]), and |c[t + 1]| |c[t]|); a butterfly
//            (xor 32 ... 1) folds them, so every lane holds the same bits.  No pair spans the parts: the runs are apart.
//   R        re + 0 * im, im: record_fine's re + 1j * im, whose real part is NaN where im is infinite or NaN
//   turn     R (cos - i sin) with the table entry of fi mod k; left out at k == 1, as record_fine leaves it out.
//   level    the inside frames are numbered part 0's run, then part 1's; lane l holds |c| of the numbers l, l + 64, l + 128,
//            l + 192 in registers and reads the rest again (L1 / L2).  |c| >= +0, so the bit patterns order as uint64: the value
//            of rank r is found bit by bit from the top, 63 steps of "how many lie below the candidate", each a ballot and a
//            population count per 64 frames.  An even count runs it for both middle ranks and takes (a + b) / 2.  A NaN inside makes
//            the level NaN, as numpy.median does.
//   edges    half = level / 2.  up0 / upN: the first / last inside frame with |c| >= half (ballots).  The walk down from up0 (up
//            from upN) takes 64 frames of the same part a step, all delivered frames and not only the inside ones; the first step
//            with a frame below half has it as the lowest set lane.  NaN compares false and is passed.  Then record_edges' line,
//            (pos[q] + t * (+-h)) + N / 2 with t = (half - a[q]) / (a[p] - a[q]), p the neighbour on the pulse's side.
// No LDS and no scratch (profiles/record_estimates_kernel_resources.txt).
#ifndef RT_RECORD_ESTIMATES_H
#define RT_RECORD_ESTIMATES_H

#include "rt_record_stft.h"

namespace rt {

constexpr int kEstHold = 4;          // inside magnitudes a lane keeps in registers: records of up to 256 inside frames read once
constexpr int kEstTurnBytes = 256;   // the turn-back table in front of the plan: kStftHopMaxDiv (cos, sin) pairs of float64

template <class P>
struct EstimatesArgs {
    const typename stft_types<P>::C *values;  // the hop pool: [n_frames]
    const double *turn;          // [k][2] cos, sin of 2 pi m / k
    const int64_t *frame_first;  // [n_records + 1]
    const int64_t *base;         // [n_records][2]
    const int32_t *range;        // [n_records][4]
    const int32_t *lp;           // [n_records]
    const int32_t *fmod;         // [n_records]
    int32_t n_records;
    int32_t nperseg;
    int32_t hop_div;
    int64_t n_frames;            // frame_first[n_records]: no frame is read behind it
    rt_record_estimate *out;     // [n_records]
};

__device__ __forceinline__ double est_wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

template <class C>
__device__ __forceinline__ double est_mag(const C c) {
    const double re = (double)c.x, im = (double)c.y;
    if (isinf(re) || isinf(im)) return __builtin_inf();
    return sqrt(re * re + im * im);
}

template <class P>
__global__ __launch_bounds__(kStftBlock) void record_estimates(EstimatesArgs<P> a) {
    using C = typename stft_types<P>::C;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = (int)(threadIdx.x & 63u);
    const int64_t r = (int64_t)blockIdx.x * kStftWaves + wave;
    if (r >= a.n_records) return;
    const int64_t f0 = a.frame_first[r], f1 = a.frame_first[r + 1];
    const int N = a.nperseg, k = a.hop_div, h = N / k;
    const int F = (int)(f1 - f0);
    const int Lp = a.lp[r], Fp = Lp > 0 ? (Lp - 1) * k + 1 : 0;
    const int lo0 = a.range[4 * r], hi0 = a.range[4 * r + 1], lo1 = a.range[4 * r + 2], hi1 = a.range[4 * r + 3];
    // (the host refuses such a plan: estimates_build_work)
    if (f0 < 0 || f1 < f0 || f1 > a.n_frames || f1 - f0 > 0x7fffffffll || Fp > F || lo0 < 0 || lo0 > hi0 || hi0 > Fp || lo1 < Fp || lo1 > hi1 || hi1 > F) return;
    const C *const v = a.values + f0;
    const double nan = __builtin_nan("");

    // ---- pairs
    double re = 0.0, im = 0.0, mg = 0.0;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int lo = p ? lo1 : lo0, hi = p ? hi1 : hi0;
        for (int t = lo + lane; t < hi - 1; t += 64) {
            const C c0 = v[t], c1 = v[t + 1];
            const double x0 = (double)c0.x, y0 = (double)c0.y, x1 = (double)c1.x, y1 = (double)c1.y;
            re += x1 * x0 + y1 * y0;
            im += y1 * x0 - x1 * y0;
            mg += est_mag(c1) * est_mag(c0);
        }
    }
    re = est_wave_sum(re);
    im = est_wave_sum(im);
    mg = est_wave_sum(mg);
    re += 0.0 * im;  // record_fine forms R as re + 1j * im: the product's real part, 0 * im, is NaN for an infinite or NaN im
    const int n0 = hi0 - lo0, n_in = n0 + (hi1 - lo1);
    const int n_pairs = (n0 > 1 ? n0 - 1 : 0) + (hi1 - lo1 > 1 ? hi1 - lo1 - 1 : 0);
    if (k != 1) {
        const double c = a.turn[2 * a.fmod[r]], s = a.turn[2 * a.fmod[r] + 1];
        const double tr = re * c + im * s, ti = im * c - re * s;
        re = tr;
        im = ti;
    }
    rt_record_estimate row;
    row.r_re = re;
    row.r_im = im;
    row.pair_mag = mg;
    row.n_pairs = n_pairs;
    row.n_inside = n_in;
    row.offset_bins = n_pairs ? atan2(im, re) / (2.0 * 3.141592653589793) * (double)k : nan;
    row.coherence = n_pairs ? sqrt(re * re + im * im) / mg : nan;
    row.level = row.rise = row.fall = nan;

    // ---- level: the exact median of the inside magnitudes
    const auto frame_of = [&](int i) { return i < n0 ? lo0 + i : lo1 + (i - n0); };  // inside number -> frame
    double held[kEstHold];
    bool any_nan = false;
#pragma unroll
    for (int j = 0; j < kEstHold; ++j) {
        const int i = j * 64 + lane;
        held[j] = i < n_in ? est_mag(v[frame_of(i)]) : 0.0;
        any_nan |= held[j] != held[j];
    }
    for (int b = kEstHold * 64; b < n_in; b += 64) {
        const int i = b + lane;
        const double m = i < n_in ? est_mag(v[frame_of(i)]) : 0.0;
        any_nan |= m != m;
    }
    any_nan = __ballot(any_nan) != 0;
    if (n_in > 0 && !any_nan) {
        // how many inside magnitudes have bits below `cand`: the same number on every lane
        const auto below = [&](unsigned long long cand) {
            int cnt = 0;
#pragma unroll
            for (int j = 0; j < kEstHold; ++j) {
                const int i = j * 64 + lane;
                cnt += __popcll(__ballot(i < n_in && (unsigned long long)__double_as_longlong(held[j]) < cand));
            }
            for (int b = kEstHold * 64; b < n_in; b += 64) {
                const int i = b + lane;
                const double m = i < n_in ? est_mag(v[frame_of(i)]) : 0.0;
                cnt += __popcll(__ballot(i < n_in && (unsigned long long)__double_as_longlong(m) < cand));
            }
            return cnt;
        };
        // the magnitude of rank `rank` (0-based): the largest pattern with at most `rank` magnitudes below it
        const auto select = [&](int rank) {
            unsigned long long res = 0;
            for (int bit = 62; bit >= 0; --bit) {
                const unsigned long long cand = res | (1ull << bit);
                if (below(cand) <= rank) res = cand;
            }
            return __longlong_as_double((long long)res);
        };
        const double upper = select(n_in / 2);
        row.level = (n_in & 1) ? upper : (select(n_in / 2 - 1) + upper) / 2.0;

        // ---- edges
        const double half = 0.5 * row.level;
        if (half > 0) {
            int up0 = 0x7fffffff, upN = -1;  // inside numbers
            const auto note = [&](int base, bool reach) {
                const unsigned long long m = __ballot(reach);
                if (m) {
                    if (up0 == 0x7fffffff) up0 = base + (int)__ffsll((long long)m) - 1;
                    upN = base + 63 - (int)__clzll((long long)m);
                }
            };
#pragma unroll
            for (int j = 0; j < kEstHold; ++j) note(j * 64, j * 64 + lane < n_in && held[j] >= half);
            for (int b = kEstHold * 64; b < n_in; b += 64) {
                const int i = b + lane;
                const double m = i < n_in ? est_mag(v[frame_of(i)]) : 0.0;
                note(b, i < n_in && m >= half);
            }
            if (upN >= 0) {
                const double dh = (double)h;
                {   // rise: the nearest frame below up0, in its part, with |c| < half
                    const int q0 = frame_of(up0), pb = q0 < Fp ? 0 : Fp;
                    for (int top = q0; top > pb; top -= 64) {
                        const int q = top - 1 - lane;
                        const double aq = q >= pb ? est_mag(v[q]) : 0.0;
                        const unsigned long long m = __ballot(q >= pb && aq < half);
                        if (m) {
                            const int qq = top - (int)__ffsll((long long)m);
                            const double a_q = est_mag(v[qq]), a_p = est_mag(v[qq + 1]);
                            const double pos = (double)(a.base[2 * r + (q0 < Fp ? 0 : 1)] + (int64_t)(qq - pb) * h);
                            const double t = (half - a_q) / (a_p - a_q);
                            row.rise = (pos + t * dh) + 0.5 * (double)N;
                            break;
                        }
                    }
                }
                {   // fall: the nearest frame above upN, in its part, with |c| < half
                    const int q0 = frame_of(upN), pb = q0 < Fp ? 0 : Fp, pe = q0 < Fp ? Fp : F;
                    for (int bot = q0 + 1; bot < pe; bot += 64) {
                        const int q = bot + lane;
                        const double aq = q < pe ? est_mag(v[q]) : 0.0;
                        const unsigned long long m = __ballot(q < pe && aq < half);
                        if (m) {
                            const int qq = bot + (int)__ffsll((long long)m) - 1;
                            const double a_q = est_mag(v[qq]), a_p = est_mag(v[qq - 1]);
                            const double pos = (double)(a.base[2 * r + (q0 < Fp ? 0 : 1)] + (int64_t)(qq - pb) * h);
                            const double t = (half - a_q) / (a_p - a_q);
                            row.fall = (pos + t * -dh) + 0.5 * (double)N;
                            break;
                        }
                    }
                }
            }
        }
    }
    if (lane == 0) a.out[r] = row;
}

}  // namespace rt
#endif
