// rt_tables.h -- the tables a handle uploads at creation, built on the host: twiddles, window orders, the window's three-bin
// fit, the general transform's twiddles and Bluestein's chirp tables.  Plain C++ (no HIP): rt_analyze.hip uploads what these
// return, and the CPU suite checks every entry against its definition through rt_hostcheck.cpp (tests/test_host_tables.py).
// Each builder's comment names the layout and the kernel that reads it; host and kernel must agree on it.
// Every entry is computed in the wider type (double for float32 tables, long double for float64 ones) with its exponent
// reduced in integers, and rounded once.
#ifndef RT_TABLES_H
#define RT_TABLES_H

#include <cmath>
#include <vector>

#include "rt_core.h"

namespace rt {

constexpr int kScan64TwiddleRows = 16;  // rows of stft_scan64's twiddle table in LDS (rt_scan64.h: kW64TwRows), 14 of them used

struct ScanTwiddles {
    std::vector<cf> tw1, tw2;
};

// The fused scans' twiddles (StftParams::tw1 / tw2) for nperseg N; LG = QS ? QS : 16 R3 lanes hold a segment.
//   stft_scan (rt_kernels.h), nperseg 256 ... 2048 and 32 / 64 / 128:
//     tw1 [LG][16]   W_N^(a k1) for lane a; with QS, register r = e QS + k1 of lane a holds A[n' = (16 / QS) a + e][k1] and takes
//                    W_N^(n' k1): entry [a][k] = W_N^(((16 / QS) a + k / QS) (k % QS))
//     tw2 [R3][16]   W_LG^(b q1), times the phase W16^(-s q1) that undoes the column rotation s = x1_rotation(R3, b) of exchange 1:
//                    together W_LG^((b - s R3) q1)
//   stft_scan64 (rt_scan64.h), nperseg 4096 (`wave64`): tw1 [16][64], W_N^(ka n1) with n1 = c + 8 d as W^(8 ka d) (rows 0..6,
//     d = 1..7) times W^(ka c) (rows 7..13, c = 1..7), lane ka; rows 14 and 15 are (1, 0).  tw2 as above.
//   stft_wg (rt_scan_wg.h), nperseg 8192 / 16 384 (`big` = threads of a workgroup): tw1 [5][big] = W_N^(t 2^i) as [i][t],
//     tw2 [big / 16][16] = W_big^(d p) as [d][p].
inline ScanTwiddles scan_twiddles(int N, int R3, int QS, int big, bool wave64) {
    const int LG = QS ? QS : 16 * R3;
    ScanTwiddles out;
    std::vector<cf> &tw1 = out.tw1, &tw2 = out.tw2;
    tw1.resize((size_t)LG * 16);
    tw2.resize((size_t)R3 * 16);
    const double two_pi = 6.283185307179586476925286766559;
    for (int a = 0; a < LG; ++a)
        for (int k1 = 0; k1 < 16; ++k1) {
            const int e = QS ? (((16 / QS) * a + k1 / QS) * (k1 % QS)) % N : (a * k1) % N;
            const double ang = -two_pi * (double)e / (double)N;
            tw1[(size_t)a * 16 + k1] = cf{(float)std::cos(ang), (float)std::sin(ang)};
        }
    if (big) {
        const int R = big / 16;
        tw1.assign((size_t)5 * big, cf{1.f, 0.f});
        for (int i = 0; i < 5; ++i)
            for (int t = 0; t < big; ++t) {
                const double ang = -two_pi * (double)(((long long)t << i) % N) / (double)N;
                tw1[(size_t)i * big + t] = cf{(float)std::cos(ang), (float)std::sin(ang)};
            }
        tw2.assign((size_t)R * 16, cf{1.f, 0.f});
        for (int d = 0; d < R; ++d)
            for (int pp = 0; pp < 16; ++pp) {
                const double ang = -two_pi * (double)((d * pp) % big) / (double)big;
                tw2[(size_t)d * 16 + pp] = cf{(float)std::cos(ang), (float)std::sin(ang)};
            }
    }
    if (wave64) {
        tw1.assign((size_t)kScan64TwiddleRows * 64, cf{1.f, 0.f});
        for (int row = 0; row < 14; ++row)
            for (int ka = 0; ka < 64; ++ka) {
                const int e = row < 7 ? 8 * ka * (row + 1) : ka * (row - 6);
                const double ang = -two_pi * (double)(e % N) / (double)N;
                tw1[(size_t)row * 64 + ka] = cf{(float)std::cos(ang), (float)std::sin(ang)};
            }
    }
    for (int b = 0; b < R3 && !big; ++b)
        for (int q1 = 0; q1 < 16; ++q1) {
            const int s1 = x1_rotation(R3, b);
            const int e = (((b - s1 * R3) * q1) % LG + LG) % LG;  // the exponent reduced in integers
            const double ang = -two_pi * (double)e / (double)LG;
            tw2[(size_t)b * 16 + q1] = cf{(float)std::cos(ang), (float)std::sin(ang)};
        }
    return out;
}

// |X|^2 * scale is computed as |X'|^2 with X' the transform of the segment under sqrt(scale) * window: one multiplication per
// output cell less in the scan kernels (each coefficient rounded once, from double).  StftParams::window, natural order.
inline std::vector<float> scaled_window(const float *window, int N, float scale) {
    std::vector<float> ws((size_t)N);
    const double root = std::sqrt((double)scale);
    for (int i = 0; i < N; ++i) ws[(size_t)i] = (float)((double)window[i] * root);
    return ws;
}

// stft_wg (rt_scan_wg.h) reads the window in thread order: [t][32] = window[t + BLK j], BLK = big
inline std::vector<float> window_thread_order(const std::vector<float> &ws, int N, int big) {
    std::vector<float> wt((size_t)N);
    for (int t = 0; t < big; ++t)
        for (int j = 0; j < 32; ++j) wt[(size_t)t * 32 + j] = ws[(size_t)t + (size_t)big * j];
    return wt;
}

// nperseg 4096 (R3 = 16, LG = 256 lanes) reads the window by lane: stft_scan as [l][16] = window[l + LG m]; stft_scan64 (`wave64`)
// in 16-byte pieces [n0][jq][lane] holding the elements m = n0 + 4 (4 jq + e), e < 4, of lane l: window[l + 64 m]
inline std::vector<float> window_lane_order(const std::vector<float> &ws, int N, int LG, bool wave64) {
    std::vector<float> wt((size_t)N);
    for (int l = 0; l < LG; ++l)
        for (int m = 0; m < 16; ++m) wt[(size_t)l * 16 + m] = ws[(size_t)l + (size_t)LG * m];
    if (wave64) {
        for (int n0 = 0; n0 < 4; ++n0)
            for (int jq = 0; jq < 4; ++jq)
                for (int l = 0; l < 64; ++l)
                    for (int e2 = 0; e2 < 4; ++e2)
                        wt[(((size_t)n0 * 4 + jq) * 64 + l) * 4 + e2] = ws[(size_t)l + 64 * (size_t)(n0 + 4 * (4 * jq + e2))];
    }
    return wt;
}

// Transform of the coefficients as the kernels use them, at bins 0, 1 and N - 1.  If it is real and confined to those bins
// (hamming, hann, boxcar: every cosine-sum window of order <= 1 in get_window's periodic form) the constant detrend can be
// applied to the transform (the LIN kernels, rt_kernels.h) and stft_wg can compute the window instead of loading it (WCOS,
// rt_scan_wg.h); any other window keeps the subtract-first kernels and the table.
struct CosineFit {
    double wr[3], wi[3];  // W[0], W[1], W[N-1]
    bool cosine_sum;
};
inline CosineFit fit_cosine_window(const std::vector<float> &ws, int N) {
    const double two_pi = 6.283185307179586476925286766559;
    CosineFit f{{0, 0, 0}, {0, 0, 0}, false};
    double *wr = f.wr, *wi = f.wi;
    const int ks[3] = {0, 1, N - 1};
    for (int j = 0; j < 3; ++j)
        for (int n = 0; n < N; ++n) {
            const double ang = -two_pi * (double)(((long long)ks[j] * n) % N) / (double)N;
            wr[j] += (double)ws[(size_t)n] * std::cos(ang);
            wi[j] += (double)ws[(size_t)n] * std::sin(ang);
        }
    // the window is of that form iff the three bins reproduce it:  w[n] = (W0 + W1 e^(+i t) + W_(N-1) e^(-i t)) / N
    double wmax = 0.0, dev = 0.0;
    for (int n = 0; n < N; ++n) {
        const double t = two_pi * (double)n / (double)N;
        const double fit = (wr[0] + (wr[1] + wr[2]) * std::cos(t) - (wi[1] - wi[2]) * std::sin(t)) / N;
        wmax = std::max(wmax, std::fabs((double)ws[(size_t)n]));
        dev = std::max(dev, std::fabs((double)ws[(size_t)n] - fit));
    }
    const double w0 = std::fabs(wr[0]);
    bool cosine_sum = w0 > 0.0 && dev <= 1e-6 * wmax;
    for (int j = 0; j < 3; ++j)
        if (std::fabs(wi[j]) > 1e-6 * w0) cosine_sum = false;  // real transform (w[n] = w[N-n])
    f.cosine_sum = cosine_sum;
    return f;
}

// ---- the general transform and Bluestein's algorithm (rt_general.h; float64 handles: rt_f64.h) ----
// Out = cf, Wide = double for a float32 handle; Out = cd, Wide = long double for a float64 one.

template <class Wide>
constexpr Wide pi_of() {
    return (Wide)3.141592653589793238462643383279502884L;
}

// W_M^j = exp(-2 pi i j / M), j < M / 2 (StftGeneralParams / F64StftParams::tw)
template <class Out, class Wide>
std::vector<Out> transform_twiddles(int M) {
    using S = decltype(Out{}.x);
    std::vector<Out> tw((size_t)M / 2);
    for (int j = 0; j < M / 2; ++j) {
        const Wide ang = (Wide)-2 * pi_of<Wide>() * (Wide)j / (Wide)M;
        tw[(size_t)j] = Out{(S)std::cos(ang), (S)std::sin(ang)};
    }
    return tw;
}

// W_N^j = exp(-2 pi i j / N) for every j < N (StftArgs::tw, rt_record_stft.h: record_stft reads entry (fi * n) mod N, reduced in
// integers, for bin fi and sample n -- any N, a power of two or not)
template <class Out, class Wide>
std::vector<Out> record_stft_twiddles(int N) {
    using S = decltype(Out{}.x);
    std::vector<Out> tw((size_t)N);
    for (int j = 0; j < N; ++j) {
        const Wide ang = (Wide)-2 * pi_of<Wide>() * (Wide)j / (Wide)N;
        tw[(size_t)j] = Out{(S)std::cos(ang), (S)std::sin(ang)};
    }
    return tw;
}

// FFT_M in place (iterative radix-2: bit reversal, then log2 M stages)
template <class Wide>
void host_fft(std::vector<Wide> &re, std::vector<Wide> &im) {
    const size_t M = re.size();
    for (size_t i = 1, j = 0; i < M; ++i) {
        size_t bit = M >> 1;
        for (; j & bit; bit >>= 1) j ^= bit;
        j ^= bit;
        if (i < j) {
            std::swap(re[i], re[j]);
            std::swap(im[i], im[j]);
        }
    }
    for (size_t len = 2; len <= M; len <<= 1)
        for (size_t i = 0; i < M; i += len)
            for (size_t k = 0; k < len / 2; ++k) {
                const Wide a = (Wide)-2 * pi_of<Wide>() * (Wide)k / (Wide)len;
                const Wide wr = std::cos(a), wi = std::sin(a);
                const size_t u = i + k, v = i + k + len / 2;
                const Wide xr = re[v] * wr - im[v] * wi, xi = re[v] * wi + im[v] * wr;
                re[v] = re[u] - xr;
                im[v] = im[u] - xi;
                re[u] += xr;
                im[u] += xi;
            }
}

// Bluestein's tables for nperseg N on a transform of length M = 2^log2m >= 2 N - 1:
//   cwin  [N]  window[n] * root * w[n] with the chirp w[n] = exp(-i pi n^2 / N), n^2 reduced mod 2 N in integers (root:
//              sqrt(scale) on a float32 handle, as every scan takes its window; 1 on a float64 one, which scales the powers)
//   bfilt [M]  FFT_M of the filter conj(w[m]) on -N < m < N wrapped to length M, divided by M, in bit-reversed order (the kernels'
//              first transform, decimation in frequency, leaves its values in that order)
template <class Out>
struct BluesteinTables {
    std::vector<Out> cwin, bfilt;
};
template <class Out, class Wide, class W>
BluesteinTables<Out> bluestein_tables(const W *window, int N, int M, int log2m, Wide root) {
    using S = decltype(Out{}.x);
    const Wide pi = pi_of<Wide>();
    auto chirp = [&](long long n, Wide sign, Wide *re, Wide *im) {
        const long long e = (n * n) % (2ll * N);
        const Wide ang = sign * pi * (Wide)e / (Wide)N;
        *re = std::cos(ang);
        *im = std::sin(ang);
    };
    BluesteinTables<Out> out;
    out.cwin.resize((size_t)N);
    for (int n = 0; n < N; ++n) {
        Wide cr, ci;
        chirp(n, (Wide)-1, &cr, &ci);
        const Wide wv = (Wide)window[n] * root;
        out.cwin[(size_t)n] = Out{(S)(wv * cr), (S)(wv * ci)};
    }
    std::vector<Wide> br((size_t)M, (Wide)0), bi((size_t)M, (Wide)0);
    for (int m = 0; m < N; ++m) {
        Wide cr, ci;
        chirp(m, (Wide)1, &cr, &ci);
        br[(size_t)m] = cr;
        bi[(size_t)m] = ci;
        if (m) {
            br[(size_t)(M - m)] = cr;
            bi[(size_t)(M - m)] = ci;
        }
    }
    host_fft(br, bi);
    out.bfilt.resize((size_t)M);
    for (int i = 0; i < M; ++i) {
        unsigned r = 0;
        for (int b = 0; b < log2m; ++b) r |= ((unsigned)(i >> b) & 1u) << (log2m - 1 - b);
        out.bfilt[(size_t)i] = Out{(S)(br[(size_t)r] / (Wide)M), (S)(bi[(size_t)r] / (Wide)M)};
    }
    return out;
}

}  // namespace rt

#endif  // RT_TABLES_H
