// estimates_work.cpp -- a stand-alone run of rt_fetch_record_estimates' host arithmetic for a sanitizer build
// (tests/test_record_estimates_contract.py compiles it with the host compiler and -fsanitize=address,undefined and runs it; build
// with -I <the package's csrc directory>).  300 seeded record lists -- records without a segment, records wholly in the predecessor
// part, records without one and records whose cells begin below what was delivered among them -- go through iq_build_descs and
// estimates_build_work at every kind of nperseg and every k of 1 .. 16 that divides it; every run of inside frames must lie in its
// part and hold exactly the frames whose position lies inside the record's cells; the turn-back table is filled for every k; lists
// the plan must refuse are refused.  Exit status 0 and nothing on stderr.
#include <cmath>
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
    std::fprintf(stderr, "estimates_work: seed %d: %s\n", seed, what);
    std::exit(1);
}

}  // namespace

int main() {
    const int sizes[] = {8, 32, 256, 300, 1000, 1024, 8192};
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
            const int start = (int)rng.next((unsigned)(T + 6)) - 6, len = (int)rng.next(6);  // (len 0: a record without a cell)
            rec[4 * i] = s;
            rec[4 * i + 1] = (int32_t)rng.next((unsigned)N);
            rec[4 * i + 2] = start;
            rec[4 * i + 3] = start + len < T ? start + len : T;
        }
        std::vector<int64_t> offsets(n + 1);
        std::vector<int32_t> first(n), fi(n), start(n), end(n);
        std::vector<IqDesc> descs;
        (void)iq_build_descs(call, N, rec.data(), 4 * sizeof(int32_t), n, offsets.data(), first.data(), &descs);
        for (size_t i = 0; i < n; ++i) {
            fi[i] = rec[4 * i + 1];
            start[i] = rec[4 * i + 2];
            end[i] = rec[4 * i + 3] > rec[4 * i + 2] ? rec[4 * i + 3] : rec[4 * i + 2];
        }
        for (int k = -1; k <= kStftHopMaxDiv + 1; ++k) {
            EstimatesWork w;
            const int64_t frames = estimates_build_work(offsets.data(), first.data(), fi.data(), start.data(), end.data(), n, N, k, &w);
            if (k < 1 || k > kStftHopMaxDiv || N % k != 0) {
                if (frames != -1) fail(seed, "a hop that does not divide nperseg, or lies outside 1 .. 16");
                continue;
            }
            StftHopWork hw;
            if (frames < 0 || frames != stft_hop_build_work(offsets.data(), first.data(), fi.data(), n, N, k, &hw)) fail(seed, "a good list refused, or other frames than the hop plan's");
            if (w.frame_first != hw.frame_first || w.lp != hw.lp || w.range.size() != 4 * n || w.base.size() != 2 * n || w.fmod.size() != n) fail(seed, "list sizes");
            const int64_t h = N / k;
            for (size_t i = 0; i < n; ++i) {
                const int64_t F = w.frame_first[i + 1] - w.frame_first[i], Fp = stft_hop_part_frames(w.lp[i], k);
                const int32_t *r = &w.range[4 * i];
                if (r[0] < 0 || r[0] > r[1] || r[1] > Fp || r[2] < Fp || r[2] > r[3] || r[3] > F) fail(seed, "a run outside its part");
                if (w.fmod[i] != fi[i] % k || w.base[2 * i] != (int64_t)first[i] * N || w.base[2 * i + 1] != (first[i] > 0 ? (int64_t)first[i] * N : 0)) fail(seed, "a record's entry");
                for (int64_t j = 0; j < F; ++j) {
                    const int64_t pos = j < Fp ? w.base[2 * i] + j * h : w.base[2 * i + 1] + (j - Fp) * h;
                    const bool inside = (int64_t)start[i] * N <= pos && pos + N <= (int64_t)end[i] * N;
                    const bool listed = (j >= r[0] && j < r[1]) || (j >= r[2] && j < r[3]);
                    if (inside != listed) fail(seed, "a run is not the frames inside the record's cells");
                }
            }
            if (estimates_build_work(offsets.data(), first.data(), fi.data(), start.data(), end.data(), n, N, k, nullptr) != frames) fail(seed, "counting without a list");
            double cs[2 * kStftHopMaxDiv];
            estimates_turn_table(k, cs);
            for (int j = 0; j < k; ++j)
                if (std::fabs(cs[2 * j] * cs[2 * j] + cs[2 * j + 1] * cs[2 * j + 1] - 1.0) > 1e-15) fail(seed, "the turn-back table");
            if (n) {  // broken lists are refused, and the null forms
                std::vector<int32_t> bad = start;
                bad[n - 1] = end[n - 1] + 1;
                if (estimates_build_work(offsets.data(), first.data(), fi.data(), bad.data(), end.data(), n, N, k, &w) != -1) fail(seed, "start behind end");
                std::vector<int64_t> bad_off = offsets;
                bad_off[n] += 1;
                if (N > 1 && estimates_build_work(bad_off.data(), first.data(), fi.data(), start.data(), end.data(), n, N, k, &w) != -1) fail(seed, "an offset that is no multiple of nperseg");
                std::vector<int32_t> bad_fi = fi;
                bad_fi[n - 1] = N;
                if (estimates_build_work(offsets.data(), first.data(), bad_fi.data(), start.data(), end.data(), n, N, k, &w) != -1) fail(seed, "a bin past the last");
                if (estimates_build_work(offsets.data(), first.data(), fi.data(), nullptr, end.data(), n, N, k, &w) != -1) fail(seed, "no starts");
                if (estimates_build_work(offsets.data(), first.data(), fi.data(), start.data(), nullptr, n, N, k, &w) != -1) fail(seed, "no ends");
                if (estimates_build_work(offsets.data(), nullptr, fi.data(), start.data(), end.data(), n, N, k, &w) != -1) fail(seed, "no first segments");
            }
            if (estimates_build_work(nullptr, first.data(), fi.data(), start.data(), end.data(), n, N, k, &w) != -1) fail(seed, "no offsets");
        }
    }
    return 0;
}
