// Stand-alone sanitizer run of the host-only code of RT_FLAG_F64_RESCUE (rt_core.h: f64_rescue_rounds; rt_hostcheck.cpp:
// hc_extract_rescue_f64).  No Python, no GPU:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude \
//       -o san_f64_rescue tools/san_f64_rescue_main.cpp pyradiotracking_amd/csrc/rt_hostcheck.cpp && ./san_f64_rescue
// The round arithmetic over random calls (every overflowing stream in exactly one round, a round within the budget unless it is a
// single stream), and the planted maps of tools/san_f64_sparse_main.cpp -- plateaus inside the buffer, through t = 0, into the
// buffer's end, NaN cells -- through both twins with row sums folded in chunks, as the scan folds them: the rescue twin's records
// must be hc_extract_sparse_f64's byte for byte.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../include/rt_analyze.h"

extern "C" {
int hc_extract_sparse_f64(const uint32_t *, const double *, int, const double *, int, int, const double *, int, int, int, double, double,
                          double, double, double, double, rt_record_f64 *, int);
int hc_extract_rescue_f64(const double *, const double *, int, int, const double *, int, int, int, double, double, double, double, double,
                          double, rt_record_f64 *, int);
unsigned hc_f64_cell_key(int, int);
long long hc_f64_rescue_budget(void);
void hc_f64_rescue_rounds(int, int, int, long long, int *);
}

static int fails = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); \
            ++fails;                                               \
        }                                                          \
    } while (0)

int main() {
    std::mt19937_64 rng(418);
    // rounds
    const long long budget = hc_f64_rescue_budget();
    CHECK(budget == 256ll << 20);
    int r[2];
    hc_f64_rescue_rounds(0, 64, 4096, budget, r);
    CHECK(r[0] == 0 && r[1] == 0);
    hc_f64_rescue_rounds(128, 64, 4096, budget, r);
    CHECK(r[0] == 128 && r[1] == 1);
    hc_f64_rescue_rounds(129, 64, 4096, budget, r);
    CHECK(r[0] == 128 && r[1] == 2);
    hc_f64_rescue_rounds(7, 1 << 20, 4096, budget, r);
    CHECK(r[0] == 1 && r[1] == 7);
    long long n_rounds = 0;
    for (int i = 0; i < 2000; ++i) {
        const int n_bad = 1 + (int)(rng() % 5000), T = 2 + (int)(rng() % 4000), N = 32 << (rng() % 8);
        const long long b = 1 + (long long)(rng() % (1ull << 31));
        hc_f64_rescue_rounds(n_bad, T, N, b, r);
        const long long one = (long long)T * N * 8;
        CHECK(r[0] >= 1 && r[0] <= n_bad);
        CHECK(r[0] == 1 || r[0] * one <= b);
        CHECK(r[0] == n_bad || (r[0] + 1) * one > b);
        CHECK((long long)(r[1] - 1) * r[0] < n_bad && (long long)r[1] * r[0] >= n_bad);  // every stream in exactly one round, none empty
        n_rounds += r[1];
    }

    // the twin against the list twin
    std::uniform_real_distribution<double> u(0.0, 1.0);
    const double thr = 1e-9, snr = 3.1622776601683795, fs = 300000.0;
    long long n_rec = 0, n_back = 0, n_nan = 0;
    for (int round = 0; round < 200; ++round) {
        const int F = 1 + (int)(rng() % 24), T = 2 + (int)(rng() % 150), TL = (int)(rng() % 120);
        auto make = [&](int rows) {
            std::vector<double> m((size_t)rows * F);
            for (double &v : m) v = thr * std::pow(10.0, -4.0 + 2.0 * u(rng));
            for (int fi = 0; fi < F && rows > 0; ++fi) {
                const int t0 = (int)(rng() % (unsigned)(rows + 20)) - 20, ln = 4 + (int)(rng() % 46);
                for (int t = t0 < 0 ? 0 : t0; t < t0 + ln && t < rows; ++t) m[(size_t)t * F + fi] = thr * std::pow(10.0, 0.8 + 1.2 * u(rng));
                if (t0 + ln < rows && t0 + ln >= 0 && (rng() & 1)) m[(size_t)(t0 + ln) * F + fi] = (rng() & 1) ? std::nextafter(thr, 0.0) : thr;
            }
            return m;
        };
        std::vector<double> cur = make(T), last = make(TL);
        if (round % 5 == 0) {
            cur[(size_t)(rng() % (unsigned)T) * F + (rng() % (unsigned)F)] = NAN;
            ++n_nan;
        }
        const bool has_last = TL > 0 && round % 3 != 0;
        const int L = 1 + (int)(rng() % 40);  // the row sums as the scan forms them: per chunk of L segments, the chunks in order
        std::vector<uint32_t> keys;
        std::vector<double> vals, sums((size_t)F, 0.0);
        for (int fi = 0; fi < F; ++fi) {
            for (int c0 = 0; c0 < T; c0 += L) {
                double part = 0.0;
                for (int t = c0; t < c0 + L && t < T; ++t) part += cur[(size_t)t * F + fi];
                sums[(size_t)fi] += part;
            }
            for (int t = 0; t < T; ++t) {
                const double p = cur[(size_t)t * F + fi];
                if (!(p < thr) || (t + 1 < T && !(cur[(size_t)(t + 1) * F + fi] < thr))) {
                    keys.push_back(hc_f64_cell_key(fi, t));
                    vals.push_back(p);
                }
            }
        }
        std::vector<rt_record_f64> a(4096), b(4096);
        const double *lp = has_last ? last.data() : nullptr;
        const int na = hc_extract_sparse_f64(keys.data(), vals.data(), (int)keys.size(), sums.data(), T, F, lp, TL, TL, 256, fs, thr, snr, 1.5,
                                             0.008, 0.04, a.data(), (int)a.size());
        const int nb = hc_extract_rescue_f64(cur.data(), sums.data(), T, F, lp, TL, TL, 256, fs, thr, snr, 1.5, 0.008, 0.04, b.data(), (int)b.size());
        CHECK(na == nb);
        for (int i = 0; i < na && i < nb; ++i) {
            CHECK(std::memcmp(&a[i], &b[i], sizeof(rt_record_f64)) == 0);
            n_back += a[i].start < 0;
        }
        n_rec += na;
    }
    CHECK(n_rec > 50 && n_back > 5);
    std::printf("san_f64_rescue: 2000 calls in %lld rounds, 200 maps (%lld with a NaN cell), %lld records (%lld with look-back), %d failures\n",
                n_rounds, n_nan, n_rec, n_back, fails);
    return fails ? 1 : 0;
}
