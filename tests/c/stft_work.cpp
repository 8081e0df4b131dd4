// stft_work.cpp -- a stand-alone run of rt_fetch_record_stft's host arithmetic for a sanitizer build (tests/test_record_stft_contract.py
// compiles it with the host compiler and -fsanitize=address,undefined and runs it; build with -I <the package's csrc directory>).
// 300 seeded record lists -- records without a segment among them -- go through iq_build_descs and stft_build_work at every kind of
// nperseg (a power of two or not); every delivered segment is looked up with stft_record_of; broken lists must be refused; the
// twiddle table is built at each size.  Exit status 0 and nothing on stderr: every segment found its record, the prefix is the
// sample offsets divided by nperseg, and every refusal came.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rt_record_iq_book.h"
#include "rt_record_stft_book.h"
#include "rt_tables.h"

using namespace rt;

namespace {

struct Lcg {
    unsigned long long x;
    unsigned next(unsigned n) {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        return (unsigned)((x >> 33) % n);
    }
};

[[noreturn]] void fail(int seed, const char *what) {
    std::fprintf(stderr, "stft_work: seed %d: %s\n", seed, what);
    std::exit(1);
}

}  // namespace

int main() {
    const int sizes[] = {8, 32, 256, 300, 1000, 1024, 8192};
    for (int seed = 0; seed < 300; ++seed) {
        Lcg rng{(unsigned long long)seed * 2654435761ull + 17};
        const int N = sizes[seed % 7], S = 1 + (int)rng.next(4), T = 2 + (int)rng.next(40), m = (int)rng.next(3);
        IqCall call;
        call.on = true;
        call.T = T;
        call.margin = m;
        call.lead_D.assign((size_t)S, 0);
        call.lead_kind.assign((size_t)S, (int32_t)kIqFromTail);
        call.lead_row.assign((size_t)S, 0);
        call.lead_buf.assign((size_t)S, 0);
        call.lead_held.assign((size_t)S, 0);
        for (int s = 0; s < S; ++s) {
            call.lead_D[(size_t)s] = (int32_t)rng.next(6);
            call.lead_held[(size_t)s] = call.lead_D[(size_t)s] + (int32_t)rng.next(3);
            call.lead_row[(size_t)s] = s;
        }
        const size_t n = rng.next(30);
        std::vector<int32_t> rec(4 * n);
        for (size_t i = 0; i < n; ++i) {
            const int s = (int)rng.next((unsigned)S);
            const int start = (int)rng.next((unsigned)(T + 4)) - 4, len = (int)rng.next(6);  // (len 0: a record without a cell)
            rec[4 * i] = s;
            rec[4 * i + 1] = (int32_t)rng.next((unsigned)N);
            rec[4 * i + 2] = start;
            rec[4 * i + 3] = start + len < T ? start + len : T;
        }
        std::vector<int64_t> offsets(n + 1);
        std::vector<int32_t> first(n), fi(n);
        std::vector<IqDesc> descs;
        const int64_t total = iq_build_descs(call, N, rec.data(), 4 * sizeof(int32_t), n, offsets.data(), first.data(), &descs);
        for (size_t i = 0; i < n; ++i) fi[i] = rec[4 * i + 1];
        StftWork w;
        const int64_t cells = stft_build_work(offsets.data(), fi.data(), n, N, &w);
        if (cells != total / N || total % N != 0) fail(seed, "cells are not the samples divided by nperseg");
        if (w.seg_first.size() != n + 1 || w.fi.size() != n) fail(seed, "list sizes");
        for (size_t i = 0; i <= n; ++i)
            if (w.seg_first[i] * N != offsets[i]) fail(seed, "prefix entry");
        for (int64_t g = 0; g < cells; ++g) {
            const int r = stft_record_of(w.seg_first.data(), (int)n, g);
            if (r < 0 || r >= (int)n || w.seg_first[(size_t)r] > g || w.seg_first[(size_t)r + 1] <= g) fail(seed, "a segment's record");
            if (w.fi[(size_t)r] != fi[(size_t)r]) fail(seed, "a record's bin");
        }
        if (n) {  // broken lists are refused, and the null forms
            std::vector<int64_t> bad = offsets;
            bad[n] += 1;
            if (N > 1 && stft_build_work(bad.data(), fi.data(), n, N, &w) != -1) fail(seed, "an offset that is no multiple of nperseg");
            bad = offsets;
            bad[n] = -(int64_t)N;
            if (stft_build_work(bad.data(), fi.data(), n, N, &w) != -1) fail(seed, "offsets running backwards");
            std::vector<int32_t> bad_fi = fi;
            bad_fi[n - 1] = N;
            if (stft_build_work(offsets.data(), bad_fi.data(), n, N, &w) != -1) fail(seed, "a bin past the last");
            bad_fi[n - 1] = -1;
            if (stft_build_work(offsets.data(), bad_fi.data(), n, N, nullptr) != -1) fail(seed, "a negative bin");
            if (stft_build_work(offsets.data(), nullptr, n, N, &w) != -1) fail(seed, "no bins");
        }
        if (stft_build_work(offsets.data(), fi.data(), n, N, nullptr) != cells) fail(seed, "counting without a list");
        if (stft_build_work(nullptr, fi.data(), n, N, &w) != -1) fail(seed, "no offsets");
        const std::vector<cf> tw = record_stft_twiddles<cf, double>(N);
        const std::vector<cd> tw64 = record_stft_twiddles<cd, long double>(N);
        if (tw.size() != (size_t)N || tw64.size() != (size_t)N || tw[0].x != 1.0f || tw64[0].x != 1.0) fail(seed, "twiddle table");
        for (int j = 0; j < N; ++j)
            if (std::fabs((double)tw[(size_t)j].x * tw[(size_t)j].x + (double)tw[(size_t)j].y * tw[(size_t)j].y - 1.0) > 1e-6) fail(seed, "a twiddle off the circle");
    }
    if (stft_root_f32(4.0f) != 2.0f || stft_root_f64(9.0) != 3.0) fail(-1, "sqrt(scale)");
    return 0;
}
