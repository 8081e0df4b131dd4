// Stand-alone sanitizer run of the host-only code of the map-free float64 path (rt_core.h: the chunk geometry, the cell keys,
// hot_capacity's bounds, rt::sparse_run_at; rt_hostcheck.cpp: hc_extract_sparse_f64).  No Python, no GPU:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude \
//       -o san_f64_sparse tools/san_f64_sparse_main.cpp pyradiotracking_amd/csrc/rt_hostcheck.cpp && ./san_f64_sparse
// Planted maps with plateaus inside the buffer, through t = 0 (look-back into a previous map), into the buffer's end, NaN cells
// and shuffled lists go through the emission rule and the twin, and the records must be hc_extract_f64's on the dense map.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../include/rt_analyze.h"

extern "C" {
int hc_extract_f64(const double *, int, int, const double *, int, int, int, double, double, double, double, double, double, rt_record_f64 *, int);
int hc_extract_sparse_f64(const uint32_t *, const double *, int, const double *, int, int, const double *, int, int, int, double, double,
                          double, double, double, double, rt_record_f64 *, int);
unsigned hc_f64_cell_key(int, int);
int hc_f64_key_bin(unsigned);
int hc_f64_key_seg(unsigned);
int hc_f64_key_max_seg(void);
int hc_f64_sparse_nperseg_ok(int);
int hc_f64_sparse_hot_capacity(int);
int hc_f64_sparse_group(int);
int hc_f64_sparse_chunk(int, int, int, int);
int hc_f64_sparse_chunks(int, int);
int hc_f64_sparse_last_chunk(int, int);
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
    // geometry
    long long geo = 0;
    for (int n = 32; n <= 4096; n *= 2) {
        CHECK(hc_f64_sparse_nperseg_ok(n));
        const int g = hc_f64_sparse_group(n);
        for (int spc : {0, 1, 3, 4, 71})
            for (int S : {1, 16, 4096}) {
                const int tmax = hc_f64_key_max_seg();
                const int L = hc_f64_sparse_chunk(n, spc, S, tmax);
                CHECK(L >= 1 && (spc == 0 || L == spc));
                if (spc == 0) CHECK((L + 1) % (g < L + 1 ? g : L + 1) == 0);
                for (int T : {0, 2, L - 1 > 2 ? L - 1 : 2, L, L + 1, 2 * L + 1, tmax}) {
                    const int c = hc_f64_sparse_chunks(T, L), last = hc_f64_sparse_last_chunk(T, L);
                    CHECK(T == 0 ? (c == 0 && last == 0) : ((c - 1) * L + last == T && last >= 1 && last <= L));
                    ++geo;
                }
            }
    }
    for (int n : {0, 8, 16, 48, 8192}) CHECK(!hc_f64_sparse_nperseg_ok(n));
    CHECK(hc_f64_sparse_hot_capacity(0) == 4096 && hc_f64_sparse_hot_capacity(1024) == 1024 && hc_f64_sparse_hot_capacity(8192) == 8192);
    CHECK(hc_f64_sparse_hot_capacity(1023) == -1 && hc_f64_sparse_hot_capacity(8193) == -1 && hc_f64_sparse_hot_capacity(-5) == -1);
    for (int fi : {0, 1, 4095})
        for (int t : {0, 1, hc_f64_key_max_seg() - 1}) {
            const unsigned k = hc_f64_cell_key(fi, t);
            CHECK(hc_f64_key_bin(k) == fi && hc_f64_key_seg(k) == t);
        }

    // records from cell lists against records from the dense map
    std::mt19937_64 rng(417);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    const double thr = 1e-9, snr = 3.1622776601683795, fs = 300000.0;
    long long n_rec = 0, n_back = 0, n_cells = 0, n_nan = 0;
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
        if (round % 5 == 0) {  // a non-finite cell: hot, and its row's mean is NaN
            cur[(size_t)(rng() % (unsigned)T) * F + (rng() % (unsigned)F)] = NAN;
            ++n_nan;
        }
        const bool has_last = TL > 0 && round % 3 != 0;
        std::vector<uint32_t> keys;
        std::vector<double> vals, sums((size_t)F, 0.0);
        for (int fi = 0; fi < F; ++fi)
            for (int t = 0; t < T; ++t) {
                const double p = cur[(size_t)t * F + fi];
                sums[(size_t)fi] += p;  // (hc_extract_f64 sums a row in this order)
                const bool hot = !(p < thr) || (t + 1 < T && !(cur[(size_t)(t + 1) * F + fi] < thr));
                if (hot) {
                    keys.push_back(hc_f64_cell_key(fi, t));
                    vals.push_back(p);
                }
            }
        for (size_t i = keys.size(); i > 1; --i) {  // the list's order is arbitrary
            const size_t j = (size_t)(rng() % i);
            std::swap(keys[i - 1], keys[j]);
            std::swap(vals[i - 1], vals[j]);
        }
        n_cells += (long long)keys.size();
        std::vector<rt_record_f64> a(4096), b(4096);
        const double *lp = has_last ? last.data() : nullptr;
        const int na = hc_extract_f64(cur.data(), T, F, lp, TL, TL, 256, fs, thr, snr, 1.5, 0.008, 0.04, a.data(), (int)a.size());
        const int nb = hc_extract_sparse_f64(keys.data(), vals.data(), (int)keys.size(), sums.data(), T, F, lp, TL, TL, 256, fs, thr, snr, 1.5,
                                             0.008, 0.04, b.data(), (int)b.size());
        CHECK(na == nb);
        for (int i = 0; i < na && i < nb; ++i) {
            CHECK(std::memcmp(&a[i], &b[i], sizeof(rt_record_f64)) == 0);  // the same cells in the same order: the same bits
            n_back += a[i].start < 0;
        }
        n_rec += na;
    }
    CHECK(n_rec > 50 && n_back > 5);  // (both kinds occur)
    std::printf("san_f64_sparse: %lld geometry cases, 200 maps (%lld with a NaN cell), %lld candidate cells, %lld records (%lld with look-back), %d failures\n",
                geo, n_nan, n_cells, n_rec, n_back, fails);
    return fails ? 1 : 0;
}
