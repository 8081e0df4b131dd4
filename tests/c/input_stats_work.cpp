// input_stats_work.cpp -- a stand-alone run of rt_fetch_input_stats' host form for a sanitizer build
// (tests/test_input_stats_contract.py compiles it with the host compiler and -fsanitize=address,undefined and runs it; build with
// -I <the repository's include directory> -I <the package's csrc directory>).  Seeded rows of every format, at lengths around the
// chunk length, at every sample alignment of the row inside a 16-byte piece and in heap blocks of exactly the row's size (a read
// past either end is an error), go through input_stats_host -- the kernels' chunks, threads, butterfly and fold -- and must give,
// field for field, what the per-component rule gives sample after sample (integer formats; the float formats' counts and peak,
// their sums within float64 round-off).  Every byte value goes through the packed 8-bit form in every position of a word.
// Exit status 0 and nothing on stderr.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "rt_analyze.h"
#include "rt_input_stats.h"

using namespace rt;

namespace {

struct Lcg {
    unsigned long long x;
    unsigned next() {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        return (unsigned)(x >> 33);
    }
};

[[noreturn]] void fail(int fmt, long long n, int shift, const char *what) {
    std::fprintf(stderr, "input_stats_work: format %d, %lld samples, shift %d: %s\n", fmt, n, shift, what);
    std::exit(1);
}

template <int FMT>
void fill(char *row, int64_t n, Lcg &rng, int kind) {
    constexpr int bps = stats_sample_bytes(FMT);
    for (int64_t j = 0; j < n; ++j) {
        if constexpr (FMT == kStatsC64 || FMT == kStatsC128) {
            double c[2];
            for (double &v : c) {
                const unsigned r = rng.next();
                v = ((double)(r & 0xffffu) / 32768.0 - 1.0) * 1.25;
                if (kind == 1 && r % 97 == 0) v = std::numeric_limits<double>::quiet_NaN();
                if (kind == 1 && r % 101 == 0) v = (r & 1) ? INFINITY : -INFINITY;
                if (kind == 1 && r % 103 == 0) v = -0.0;
            }
            if constexpr (FMT == kStatsC64) {
                const float f[2] = {(float)c[0], (float)c[1]};
                std::memcpy(row + j * bps, f, 8);
            } else {
                std::memcpy(row + j * bps, c, 16);
            }
        } else {
            for (int b = 0; b < bps; ++b) {
                const unsigned r = rng.next();
                row[j * bps + b] = kind == 0 ? (char)(r >> 3) : kind == 1 ? (char)((r & 1) ? 0xff : 0x00) : (char)0x80;
            }
        }
    }
}

// the rule, sample after sample
template <int FMT>
rt_input_stats plain(const char *row, int64_t n) {
    rt_input_stats r;
    if constexpr (FMT == kStatsC64 || FMT == kStatsC128) {
        InputStatsPart<double> t;
        stats_clear(t);
        for (int64_t j = 0; j < n; ++j) {
            double c[2];
            if constexpr (FMT == kStatsC64) {
                float f[2];
                std::memcpy(f, row + j * 8, 8);
                c[0] = f[0], c[1] = f[1];
            } else {
                std::memcpy(c, row + j * 16, 16);
            }
            stats_component(t, c[0], 0);
            stats_component(t, c[1], 1);
        }
        stats_row(r, t, n, FMT);
    } else {
        InputStatsPart<int64_t> t;
        stats_clear(t);
        stats_samples_int<FMT>(t, row, n);
        stats_row(r, t, n, FMT);
    }
    return r;
}

template <int FMT>
void run(Lcg &rng) {
    constexpr int bps = stats_sample_bytes(FMT);
    constexpr int64_t C = kInputStatsChunk;
    const int64_t sizes[] = {0, 1, 2, 7, 255, 511, 512, 513, C - 1, C, C + 1, 2 * C + 9};
    for (int64_t n : sizes) {
        for (int shift = 0; shift * bps < 16 && shift < 8; ++shift) {
            for (int kind = 0; kind < 3; ++kind) {
                // the row begins `shift` samples into a 16-byte piece and its block ends with it
                const size_t bytes = (size_t)(n + shift) * bps;
                char *block = static_cast<char *>(std::aligned_alloc(16, bytes ? (bytes + 15) / 16 * 16 : 16));
                std::vector<char> exact(bytes ? bytes : 1);
                char *row = block + (size_t)shift * bps;
                fill<FMT>(row, n, rng, kind);
                // (a second copy whose END is exact: the vector's last byte is the row's last)
                std::memcpy(exact.data(), block, bytes);
                rt_input_stats got, again, want = plain<FMT>(row, n);
                if (!input_stats_host(FMT, row, n, &got)) fail(FMT, n, shift, "format refused");
                if (!input_stats_host(FMT, exact.data() + (size_t)shift * bps, n, &again)) fail(FMT, n, shift, "format refused");
                if (got.n_samples != n || got.format != stats_public_format(FMT) || got.unit != stats_unit(FMT)) fail(FMT, n, shift, "n_samples / format / unit");
                if (got.n_rail != want.n_rail || got.n_nonfinite != want.n_nonfinite || got.peak != want.peak) fail(FMT, n, shift, "counts or peak");
                if (stats_is_float(FMT)) {
                    // any two orders of m terms differ by at most 2 m u sum|terms|; sum|raw| <= 1.25 * m here
                    const double u = std::ldexp(1.0, -53), m = (double)(2 * n);
                    if (std::fabs(got.sum_i - want.sum_i) > 2 * m * u * 1.25 * m || std::fabs(got.sum_q - want.sum_q) > 2 * m * u * 1.25 * m ||
                        std::fabs(got.sum_sq - want.sum_sq) > 2 * m * u * 1.5625 * m)
                        fail(FMT, n, shift, "a float sum beyond round-off");
                    // the same samples at another address: the same bytes
                    if (std::memcmp(&got, &again, sizeof got) != 0) fail(FMT, n, shift, "bytes depend on the address");
                } else if (std::memcmp(&got, &want, sizeof got) != 0 || std::memcmp(&got, &again, sizeof got) != 0) {
                    fail(FMT, n, shift, "not the rule's row");
                }
                std::free(block);
            }
        }
    }
}

template <int FMT>
void every_byte() {
    for (int pos = 0; pos < 4; ++pos)
        for (int b = 0; b < 256; ++b)
            for (uint32_t rest : {0x00000000u, 0xffffffffu, 0x807f807fu, 0x7f807f80u, 0x01fe5aa5u}) {
                const uint32_t x = (rest & ~(0xffu << (8 * pos))) | ((uint32_t)b << (8 * pos));
                InputStatsPart<int64_t> packed, rule;
                stats_clear(packed);
                stats_clear(rule);
                StatsWords8 w;
                stats_word8<FMT>(w, x);
                stats_word8<FMT>(w, rest);
                stats_words8_close<FMT>(packed, w);
                const uint32_t words[2] = {x, rest};
                stats_samples_int<FMT>(rule, reinterpret_cast<const char *>(words), 4);
                if (std::memcmp(&packed, &rule, sizeof packed) != 0) fail(FMT, b, pos, "the packed form differs from the rule");
            }
}

}  // namespace

int main() {
    Lcg rng{2463534242ull};
    run<kStatsC64>(rng);
    run<kStatsU8>(rng);
    run<kStatsI16>(rng);
    run<kStatsI8>(rng);
    run<kStatsC128>(rng);
    every_byte<kStatsU8>();
    every_byte<kStatsI8>();
    rt_input_stats r;
    if (input_stats_host(5, nullptr, 0, &r) || input_stats_host(-1, nullptr, 0, &r)) fail(5, 0, 0, "an unknown format was taken");
    return 0;
}
