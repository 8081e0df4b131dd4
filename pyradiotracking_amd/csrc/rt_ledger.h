// rt_ledger.h -- the look-back state of a handle and the one driver of its books.  Host-only (no HIP): rt_analyze.hip holds one
// StreamLedger per lane-less handle, float32 or float64 alike, and one LedgerCall per call slot; rt_hostcheck.cpp exports the same
// two types so that the CPU suite drives the driver itself (hc_presence_*, hc_chain_*, hc_iq_*, hc_ledger_*).
//
// What a handle has to remember, per stream, about the buffer the next call looks back into:
//   * the rotation of the three look-back tails (call k reads buffer tail_cur and writes the next one);
//   * the segment count of the previous buffer -- one per handle while all streams move in lock-step, one per stream from the
//     first rt_set_present on (PresenceBook; rt_set_chain rewrites those rows: ChainBook);
//   * the pending stream resets (rt_reset_stream, a changed threshold or setting), taken by a stream's next present call;
//   * which sample tails rt_set_record_iq holds (IqTailBook).
// begin_call takes all of it for one call and leaves the call's snapshot in a LedgerCall; the device side of a handle (pinned
// rows, uploads, launches) reads that snapshot and keeps no copy of the decisions.  rollback(c) of the NEWEST call puts the
// ledger back to what it was before that call, whatever the call took.
#ifndef RT_LEDGER_H
#define RT_LEDGER_H

#include "rt_core.h"
#include "rt_record_iq_book.h"

namespace rt {

// What a call was enqueued with; it stays in the call's slot until the slot's next call (every re-analysis inside rt_fetch reads it).
struct LedgerCall {
    bool live = false;                  // begin_call filled it and it has not been rolled back
    int T = 0, fmt = 0;
    int tail_read = 0, tail_write = 0;  // the rotation's buffers the call reads / writes
    int n_seg_last = -1;                // the handle's one count before the call (lock-step: what every stream looks back into)
    std::vector<int32_t> took;          // lock-step: [S] non-zero = the call took the stream's reset; empty: none was pending
    bool masked = false;                // per-stream regime: `pc` is this call's
    bool chained = false;               // ... and `cc`
    bool iq_on = false;                 // rt_set_record_iq was on: `iq` is this call's
    PresenceCall pc;
    ChainCall cc;
    IqCall iq;
    std::vector<int32_t> last;          // lock-step with record-IQ on: the row look_back_rows hands out
    // a call the ledger never saw (rt_extract) takes the slot
    void clear() {
        live = masked = chained = iq_on = false;
        took.clear();
    }
};

struct StreamLedger {
    int S = 0;
    int tail_cur = 0;     // the tail buffer holding the most recent buffer's columns
    int n_seg_last = -1;  // columns of the previous buffer, -1: none
    std::vector<uint8_t> reset_pending;  // [S] streams whose look-back is dropped at their next present call
    PresenceBook pres;    // inactive until activate_presence
    ChainBook chain;      // off until set_chain(links >= 2)
    IqTailBook iq;        // off until set_iq_margin(K, m >= 0)

    void configure(int n_streams) {
        S = n_streams;
        reset_pending.assign((size_t)S, (uint8_t)0);
        any_reset_ = false;
        chain.configure(S, 0);
        iq.configure(S, 0, -1);
    }
    bool any_reset() const { return any_reset_; }
    void reset_stream(int s) {
        reset_pending[(size_t)s] = 1;
        any_reset_ = true;
    }
    // `changed` [S]: non-zero = the stream's threshold or settings differ from before (it starts without look-back)
    void mark_changed(const std::vector<uint8_t> &changed) {
        for (int s = 0; s < S; ++s)
            if (changed[(size_t)s]) reset_stream(s);
    }
    // rt_reset: no look-back, no lead, nothing pending (the rotation goes on)
    void forget_all() {
        n_seg_last = -1;
        if (pres.active) pres.forget_all();
        chain.forget_all();
        iq.forget_all();
        std::fill(reset_pending.begin(), reset_pending.end(), (uint8_t)0);
        any_reset_ = false;
    }
    // rt_set_present, first use: every stream inherits the handle's one count; calls in flight keep their snapshots
    void activate_presence() {
        if (!pres.active) pres.activate(S, n_seg_last);
    }
    bool set_mask(const uint8_t *mask) { return pres.set_mask(mask); }
    // rt_set_chain: per-stream rows from here on (links >= 2), and a change of the grouping forgets all look-back
    void set_chain(int links) {
        if (links >= 2) activate_presence();
        chain.configure(S, links);
        forget_all();
    }
    // rt_set_record_iq (m < 0: off); the held tails are forgotten
    void set_iq_margin(int K, int m) { iq.configure(S, K, m); }

    // A call of T segments in format `fmt` is enqueued; `other`: the record-IQ snapshot of the other call in flight, or null.
    // Pure host code that cannot fail.  Lock-step with no reset pending and record-IQ off: no per-stream work, no allocation.
    void begin_call(int T, int fmt, const IqCall *other, LedgerCall &c) {
        c.T = T;
        c.fmt = fmt;
        c.tail_read = tail_cur;
        c.tail_write = (tail_cur + 1) % kTailBuffers;
        c.n_seg_last = n_seg_last;
        c.clear();
        c.live = true;
        if (pres.active) {
            // each stream's own previous count and the resets the present ones take, into the snapshot (absent ones keep theirs)
            pres.begin_call(T, tail_cur, reset_pending, c.pc);
            c.masked = true;
            recount();
            if (chain.on()) {  // who follows whom: the snapshot's n_seg_last row becomes the count of the buffer each stream follows
                chain.begin_call(T, c.pc, c.cc);
                c.chained = true;
            }
        } else if (any_reset_) {
            c.took.assign(reset_pending.begin(), reset_pending.end());
            std::fill(reset_pending.begin(), reset_pending.end(), (uint8_t)0);
            any_reset_ = false;
        }
        if (iq.on()) {
            iq.begin_call(T, fmt, look_back_rows(c), c.masked ? c.pc.absent.data() : nullptr, c.chained ? c.cc.src_buf.data() : nullptr,
                          c.chained ? c.cc.src_idx.data() : nullptr, other, c.iq);
            c.iq_on = true;
        }
        tail_cur = c.tail_write;
        n_seg_last = T;
    }
    // [S]: the segment count of the buffer each stream's detection looks back into in call `c` (-1: none), in either regime
    const int32_t *look_back_rows(LedgerCall &c) const {
        if (c.masked) return c.pc.n_seg_last.data();
        c.last.assign((size_t)S, (int32_t)c.n_seg_last);
        for (size_t s = 0; s < c.took.size(); ++s)
            if (c.took[s]) c.last[s] = -1;
        return c.last.data();
    }
    // The newest call is undone (its enqueue failed, or a later lane's did): rotation, counts, resets and books as before it.
    // Nothing for a snapshot the ledger does not hold (never begun, or rolled back already).
    void rollback(LedgerCall &c) {
        if (!c.live) return;
        if (c.iq_on) iq.rollback(c.iq);
        if (c.chained) chain.rollback(c.cc);
        if (c.masked) pres.rollback(c.pc, reset_pending);
        for (size_t s = 0; s < c.took.size(); ++s)
            if (c.took[s]) reset_pending[s] = 1;
        recount();
        tail_cur = c.tail_read;
        n_seg_last = c.n_seg_last;
        c.clear();
    }

private:
    bool any_reset_ = false;  // some reset_pending[s] is set
    void recount() { any_reset_ = std::find(reset_pending.begin(), reset_pending.end(), (uint8_t)1) != reset_pending.end(); }
};

}  // namespace rt
#endif
