// stft_hop_work.cpp -- a stand-alone run of rt_fetch_record_stft_hop's host arithmetic for a sanitizer build
// (tests/test_record_stft_hop_contract.py compiles it with the host compiler and -fsanitize=address,undefined and runs it; build with
// -I <the package's csrc directory>).  300 seeded record lists -- records without a segment, records wholly in the predecessor
// part and records without one among them -- go through iq_build_descs and stft_hop_build_work at every kind of nperseg and every
// k of 1 .. 16 that divides it; every frame is looked up with stft_hop_frame_at and must lie inside its part of its record; lists
// that iq_build_descs cannot have written and hops that do not divide nperseg must be refused.  Exit status 0 and nothing on stderr.
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
    std::fprintf(stderr, "stft_hop_work: seed %d: %s\n", seed, what);
    std::exit(1);
}

}  // namespace

int main() {
    const int sizes[] = {8, 32, 256, 300, 1000, 1024, 8192};
    for (int seed = 0; seed < 300; ++seed) {
        Lcg rng{(unsigned long long)seed * 2654435761ull + 29};
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
            const int start = (int)rng.next((unsigned)(T + 6)) - 6, len = (int)rng.next(6);  // (len 0: a record without a cell)
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
        for (int k = -1; k <= kStftHopMaxDiv + 1; ++k) {
            StftHopWork w;
            const int64_t frames = stft_hop_build_work(offsets.data(), first.data(), fi.data(), n, N, k, &w);
            if (k < 1 || k > kStftHopMaxDiv || N % k != 0) {
                if (frames != -1 || stft_hop_div_ok(N, k)) fail(seed, "a hop that does not divide nperseg, or lies outside 1 .. 16");
                continue;
            }
            if (frames < 0) fail(seed, "a good list refused");
            if (w.frame_first.size() != n + 1 || w.pool_seg.size() != n || w.lp.size() != n || w.fi.size() != n) fail(seed, "list sizes");
            if (k == 1 && frames != total / N) fail(seed, "k = 1: the frames are the delivered segments");
            const int64_t h = N / k;
            int64_t g = 0;
            for (size_t i = 0; i < n; ++i) {
                const int64_t L = (offsets[i + 1] - offsets[i]) / N;
                const int64_t Lp = first[i] < 0 ? ((int64_t)-first[i] < L ? (int64_t)-first[i] : L) : 0;
                if (w.lp[i] != Lp || w.pool_seg[i] * N != offsets[i] || w.fi[i] != fi[i] || w.frame_first[i] != g) fail(seed, "a record's entry");
                for (int part = 0; part < 2; ++part) {
                    const int64_t Lx = part ? L - Lp : Lp, base = offsets[i] + (part ? Lp * N : 0);
                    for (int64_t j = 0; j < stft_hop_part_frames(Lx, k); ++j, ++g) {
                        const StftHopFrame f = stft_hop_frame_at(w, g);
                        if (f.record != (int)i || f.part != part || f.sample != base + j * h) fail(seed, "a frame's record, part or sample");
                        if (f.sample < base || f.sample + N > base + Lx * N || f.sample + N > total) fail(seed, "a frame outside its part");
                    }
                }
            }
            if (g != frames || w.frame_first[n] != frames) fail(seed, "the frame count");
            if (stft_hop_build_work(offsets.data(), first.data(), fi.data(), n, N, k, nullptr) != frames) fail(seed, "counting without a list");
            if (n) {  // broken lists are refused, and the null forms
                std::vector<int64_t> bad = offsets;
                bad[n] += 1;
                if (N > 1 && stft_hop_build_work(bad.data(), first.data(), fi.data(), n, N, k, &w) != -1) fail(seed, "an offset that is no multiple of nperseg");
                bad = offsets;
                bad[n] = -(int64_t)N;
                if (stft_hop_build_work(bad.data(), first.data(), fi.data(), n, N, k, &w) != -1) fail(seed, "offsets running backwards");
                std::vector<int32_t> bad_fi = fi;
                bad_fi[n - 1] = N;
                if (stft_hop_build_work(offsets.data(), first.data(), bad_fi.data(), n, N, k, &w) != -1) fail(seed, "a bin past the last");
                if (stft_hop_build_work(offsets.data(), nullptr, fi.data(), n, N, k, &w) != -1) fail(seed, "no first segments");
                if (stft_hop_build_work(offsets.data(), first.data(), nullptr, n, N, k, &w) != -1) fail(seed, "no bins");
            }
            if (stft_hop_build_work(nullptr, first.data(), fi.data(), n, N, k, &w) != -1) fail(seed, "no offsets");
        }
    }
    return 0;
}
