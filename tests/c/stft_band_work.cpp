// stft_band_work.cpp -- a stand-alone run of rt_fetch_record_band's host arithmetic for a sanitizer build
// (tests/test_record_band_contract.py compiles it with the host compiler and -fsanitize=address,undefined and runs it; build with
// -I <the package's csrc directory>).  300 seeded record lists go through iq_build_descs and stft_hop_build_work -- the band has no
// list of its own -- at every kind of nperseg, every k of 1 .. 16 that divides it and every half width of -1 .. 9: the argument
// rule, every column's bin of every record (inside 0 .. N - 1, one step from its neighbour on the circle, the centre column the
// record's own bin), the pool's element count, and a host pool of that many values written frame by frame, each column's run inside
// it.  The overflow product must return -1.  Exit status 0 and nothing on stderr.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rt_record_iq_book.h"
#include "rt_record_stft_book.h"

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
    std::fprintf(stderr, "stft_band_work: seed %d: %s\n", seed, what);
    std::exit(1);
}

}  // namespace

int main() {
    const int sizes[] = {8, 16, 32, 256, 300, 1000, 4096};
    for (int seed = 0; seed < 300; ++seed) {
        Lcg rng{(unsigned long long)seed * 2654435761ull + 31};
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
            const int start = (int)rng.next((unsigned)(T + 6)) - 6, len = (int)rng.next(6);
            rec[4 * i] = s;
            rec[4 * i + 1] = i % 3 == 0 ? (int32_t)(i % 2 ? N - 1 : 0) : (int32_t)rng.next((unsigned)N);  // (the circle's seam among them)
            rec[4 * i + 2] = start;
            rec[4 * i + 3] = start + len < T ? start + len : T;
        }
        std::vector<int64_t> offsets(n + 1);
        std::vector<int32_t> first(n), fi(n);
        std::vector<IqDesc> descs;
        (void)iq_build_descs(call, N, rec.data(), 4 * sizeof(int32_t), n, offsets.data(), first.data(), &descs);
        for (size_t i = 0; i < n; ++i) fi[i] = rec[4 * i + 1];
        for (int k = 0; k <= kStftHopMaxDiv + 1; ++k) {
            for (int w = -1; w <= kStftBandMaxHalf + 1; ++w) {
                const bool want = k >= 1 && k <= kStftHopMaxDiv && N % k == 0 && w >= 0 && w <= kStftBandMaxHalf && 2 * w + 1 <= N;
                if (stft_band_ok(N, k, w) != want) fail(seed, "the argument rule");
                if (!want) {
                    if ((w < 0 || w > kStftBandMaxHalf) && stft_band_elems(10, w) != -1) fail(seed, "elements of a width outside 0 .. 8");
                    continue;
                }
                StftHopWork work;
                const int64_t frames = stft_hop_build_work(offsets.data(), first.data(), fi.data(), n, N, k, &work);
                if (frames < 0) fail(seed, "a good list refused");
                const int B = stft_band_columns(w);
                const int64_t elems = stft_band_elems(frames, w);
                if (B != 2 * w + 1 || elems != frames * B) fail(seed, "the pool's element count");
                std::vector<int32_t> pool((size_t)elems, -1);  // the bin each value of the pool belongs to
                for (int64_t g = 0; g < frames; ++g) {
                    const StftHopFrame f = stft_hop_frame_at(work, g);
                    const int at = work.fi[(size_t)f.record];
                    for (int j = 0; j < B; ++j) {
                        const int b = stft_band_bin(at, j, w, N);
                        if (b < 0 || b >= N || b != ((at + j - w) % N + N) % N) fail(seed, "a column's bin");
                        if (j && b != (stft_band_bin(at, j - 1, w, N) + 1) % N) fail(seed, "neighbouring columns are not neighbouring bins");
                        pool[(size_t)(g * B + j)] = b;
                    }
                    if (pool[(size_t)(g * B + w)] != at) fail(seed, "the centre column is not the record's bin");
                }
                for (int32_t b : pool)
                    if (b < 0) fail(seed, "a value of the pool that no frame writes");
            }
        }
    }
    // the checked product: the last count that fits, the first that does not, and the counts no list can have
    for (int w = 0; w <= kStftBandMaxHalf; ++w) {
        const int64_t B = 2 * w + 1, most = (INT64_MAX / 16) / B;
        if (stft_band_elems(most, w) != most * B) fail(-1, "the largest pool that fits");
        if (stft_band_elems(most + 1, w) != -1 || stft_band_elems(INT64_MAX, w) != -1 || stft_band_elems(-1, w) != -1) fail(-1, "an overflowing pool");
    }
    if (stft_band_elems(0, 0) != 0 || stft_band_elems(7, 8) != 119) fail(-1, "small pools");
    return 0;
}
