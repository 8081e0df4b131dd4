// ledger_walk.cpp -- a stand-alone walk over rt_ledger.h for a sanitizer build (tests/test_stream_ledger.py compiles it with the host
// compiler and -fsanitize=address,undefined and runs it; build with -I <the package's csrc directory>).  200 seeded schedules of
// {call, reset_stream, mark_changed, rollback of the newest call, forget_all}, each driven through two ledgers -- one in lock-step,
// one with the per-stream rows on and every stream present -- and, on top, with record-IQ and chaining on so that every book's
// vectors are walked.  Exit status 0 and nothing on stderr: both regimes saw the same look-back rows and rotation in every call,
// any_reset() always said what reset_pending holds, and every rollback put the ledger back.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rt_ledger.h"

using namespace rt;

namespace {

constexpr int S = 5, K = 3;

struct Lcg {
    unsigned long long x;
    unsigned next(unsigned n) {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        return (unsigned)((x >> 33) % n);
    }
};

struct Side {
    StreamLedger led;
    LedgerCall slot[2];
    unsigned long long n_calls = 0;
    bool can_undo = false;  // the newest call has not been rolled back or forgotten
    bool touched = false;   // ... and a reset has been asked for since
};

[[noreturn]] void fail(int seed, int step, const char *what) {
    std::fprintf(stderr, "ledger_walk: seed %d step %d: %s\n", seed, step, what);
    std::exit(1);
}

bool any_pending(const StreamLedger &l) {
    for (uint8_t v : l.reset_pending)
        if (v) return true;
    return false;
}

struct Saved {
    int tail_cur, n_seg_last;
    std::vector<uint8_t> reset_pending;
    std::vector<int32_t> per_stream, iq_cur, chain_idx;
};
Saved save(const StreamLedger &l) { return Saved{l.tail_cur, l.n_seg_last, l.reset_pending, l.pres.n_seg_last, l.iq.cur, l.chain.last_idx}; }
bool same(const Saved &a, const Saved &b) {
    return a.tail_cur == b.tail_cur && a.n_seg_last == b.n_seg_last && a.reset_pending == b.reset_pending && a.per_stream == b.per_stream &&
           a.iq_cur == b.iq_cur && a.chain_idx == b.chain_idx;
}

void walk(int seed, bool with_books) {
    static const int kT[4] = {0, 2, 3, 7};
    Lcg rng{(unsigned long long)seed * 2654435761ull + 12345ull};
    Side side[2];
    for (Side &sd : side) sd.led.configure(S);
    side[1].led.activate_presence();
    if (with_books)
        for (Side &sd : side) sd.led.set_iq_margin(K, 1);
    if (with_books && (seed & 1)) side[1].led.set_chain(S);  // (one run of all streams: only side 1 is per-stream; rows then differ by design)
    const bool compare = !(with_books && (seed & 1));
    Saved before[2];
    const int steps = 1 + (int)rng.next(12);
    for (int step = 0; step < steps; ++step) {
        const unsigned op = rng.next(8);
        const int T = kT[rng.next(4)], s = (int)rng.next(S);
        std::vector<uint8_t> changed((size_t)S);
        for (uint8_t &v : changed) v = rng.next(3) == 0;
        const int32_t *rows[2] = {nullptr, nullptr};
        for (int i = 0; i < 2; ++i) {
            Side &sd = side[i];
            if (op < 4) {
                before[i] = save(sd.led);
                const int idx = (int)(sd.n_calls % 2);
                const LedgerCall &o = sd.slot[1 - idx];
                LedgerCall &c = sd.slot[idx];
                sd.led.begin_call(T, 0, sd.n_calls && o.live && o.iq_on ? &o.iq : nullptr, c);
                ++sd.n_calls;
                sd.can_undo = true;
                sd.touched = false;
                rows[i] = sd.led.look_back_rows(c);
                if (c.masked != (i == 1) || c.iq_on != with_books) fail(seed, step, "a call's regime flags");
            } else if (op == 4) {
                sd.led.reset_stream(s);
                sd.touched = true;
            } else if (op == 5) {
                sd.led.mark_changed(changed);
                sd.touched = true;
            } else if (op == 6) {
                if (sd.can_undo) {
                    --sd.n_calls;
                    sd.led.rollback(sd.slot[sd.n_calls % 2]);
                    sd.can_undo = false;
                    if (!sd.touched && !same(before[i], save(sd.led))) fail(seed, step, "a rolled-back call left a trace");
                }
            } else {
                sd.led.forget_all();
                sd.can_undo = false;  // (a handle never rolls a call back across an rt_reset)
            }
            if (sd.led.any_reset() != any_pending(sd.led)) fail(seed, step, "any_reset() against reset_pending");
        }
        if (op < 4 && compare) {
            for (int k = 0; k < S; ++k)
                if (rows[0][k] != rows[1][k]) fail(seed, step, "look-back rows differ between the regimes");
            const LedgerCall &a = side[0].slot[(side[0].n_calls - 1) % 2], &b = side[1].slot[(side[1].n_calls - 1) % 2];
            if (a.tail_read != b.tail_read || a.tail_write != b.tail_write) fail(seed, step, "rotation differs between the regimes");
        }
        if (side[0].led.reset_pending != side[1].led.reset_pending && compare) fail(seed, step, "pending resets differ between the regimes");
    }
    // a call and its rollback at the end of every schedule: the ledger is exactly as before
    for (Side &sd : side) {
        const Saved was = save(sd.led);
        LedgerCall &c = sd.slot[sd.n_calls % 2];
        sd.led.begin_call(kT[1 + rng.next(3)], 0, nullptr, c);
        sd.led.rollback(c);
        if (!same(was, save(sd.led))) fail(seed, steps, "a rolled-back call left a trace");
        sd.led.rollback(c);  // (a second time: nothing)
        if (!same(was, save(sd.led))) fail(seed, steps, "rollback of a call the ledger does not hold");
    }
}

}  // namespace

int main() {
    for (int seed = 0; seed < 200; ++seed) {
        walk(seed, false);
        walk(seed, true);
    }
    return 0;
}
