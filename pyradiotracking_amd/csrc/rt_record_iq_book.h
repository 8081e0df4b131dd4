// rt_record_iq_book.h -- host side of rt_set_record_iq / rt_fetch_record_iq (include/rt_analyze.h): which sample tails a handle
// holds, and the copy list that cuts every record's IQ out of them and of the call's buffer.  Host-only (no HIP): a handle's
// look-back ledger (rt_ledger.h) drives it for every handle kind, and through rt_hostcheck.cpp for the CPU suite's NumPy model; the kernels
// that execute what it decides are in rt_record_iq.h.
//
// A record's `start` may be negative: it then counts whole segments back from the end of the buffer the detection looked back
// into.  The spectrogram columns of that buffer are in the look-back tails, its SAMPLES are gone by then -- unless the handle kept
// them.  So every call copies, at enqueue, the last min(T, K + m) whole segments of each present stream's row into a tail ROW of
// that stream (iq_tails), as raw bytes in the call's format; K = the handle's tail columns, m = the margin.
//   * three rows per stream.  A stream's next call must neither write the row that holds its latest tail (cur) nor a row a pending
//     call still reads at its fetch (two calls may be in flight: call k + 1's enqueue comes before fetch k); that leaves one.
//   * an absent stream writes nothing and keeps its row: no carry copy.
//   * a tail of D segments lies at the START of its row: segment -d of the predecessor is at sample (D - d) * N of the row,
//     whatever K + m is (a call shorter than K + m holds fewer segments).
//   * the predecessor's ragged remainder n_samples % N is never kept: the tail ends at sample T * N, as rt_record.start counts.
//   * a call's snapshot (IqCall, in its slot) is what its fetch works from, and what a rollback puts back.
#ifndef RT_RECORD_IQ_BOOK_H
#define RT_RECORD_IQ_BOOK_H

#include <stdint.h>

#include <algorithm>
#include <vector>

namespace rt {

constexpr int kIqRows = 3;               // tail rows per stream
constexpr int kIqMaxMargin = 1024;       // rt_set_record_iq: margin_segments <= this
constexpr int64_t kIqTileBytes = 16384;  // bytes of one descriptor a workgroup of record_iq_gather copies (rt_record_iq.h)

// where a descriptor's samples come from
enum : int32_t {
    kIqFromCall = 0,  // the record's own row of the call's IQ
    kIqFromRow = 1,   // another row of the same call (the predecessor of a chained stream)
    kIqFromTail = 2   // a tail row
};

// One contiguous copy: `len` samples from sample `src_sample` of the source to sample `dst_sample` of the call's pool.
struct IqDesc {
    int32_t kind;  // kIqFrom*
    int32_t row;   // the stream whose row is read
    int32_t buf;   // kIqFromTail: which of the stream's kIqRows rows
    int32_t reserved;
    int64_t src_sample;
    int64_t dst_sample;
    int64_t len;
};

// What a call was enqueued with, per stream.
struct IqCall {
    bool on = false;  // the feature was on when the call was enqueued
    int T = 0;        // the call's segment count
    int fmt = 0;      // its input format (the handle's code)
    int margin = 0;
    std::vector<int32_t> lead_kind;  // [S] kIqFromCall: no lead (D = 0); kIqFromRow / kIqFromTail: where segments < 0 come from
    std::vector<int32_t> lead_row;   // [S] the predecessor's stream
    std::vector<int32_t> lead_buf;   // [S] kIqFromTail: its row
    std::vector<int32_t> lead_D;     // [S] D(s): whole segments of the predecessor that can be delivered
    std::vector<int32_t> lead_held;  // [S] segments the source holds in all (kIqFromTail: the row's; kIqFromRow: T)
    std::vector<int32_t> write_buf;  // [S] the row the call's iq_tails writes for the stream, -1: none (absent)
    std::vector<int32_t> write_D;    // [S] ... and how many segments
    std::vector<int32_t> before_cur, before_held, before_fmt;  // the book before the call (rollback)
};

struct IqTailBook {
    int S = 0, K = 0;
    int margin = -1;  // < 0: the feature is off
    std::vector<int32_t> cur;   // [S] the row holding the stream's latest tail, -1: none
    std::vector<int32_t> held;  // [S] whole segments in it
    std::vector<int32_t> fmt;   // [S] the format they came in
    bool on() const { return margin >= 0; }
    int cols() const { return K + margin; }  // segments a row holds at most
    void configure(int n_streams, int tail_cols, int margin_segments) {
        S = n_streams;
        K = tail_cols;
        margin = margin_segments < 0 ? -1 : margin_segments;
        forget_all();
    }
    void forget_all() {
        cur.assign((size_t)S, (int32_t)-1);
        held.assign((size_t)S, (int32_t)0);
        fmt.assign((size_t)S, (int32_t)-1);
    }
    // A call of T segments in format `f` is enqueued.
    //   n_seg_last [S]: the segment count of the buffer each stream's detection looks back into, -1: none (per stream where the
    //                   handle keeps it per stream, else the handle's one count with the streams that take a reset set to -1);
    //   absent     [S] or null: non-zero = the stream sits the call out;
    //   src_buf / src_idx [S] or null: ChainCall's rows of a chained call (rt_core.h: 1 = a row of this call, 2 = the carried one);
    //   other: the snapshot of the other call in flight, or null.
    void begin_call(int T, int f, const int32_t *n_seg_last, const uint8_t *absent, const int32_t *src_buf, const int32_t *src_idx,
                    const IqCall *other, IqCall &c) {
        c.on = true;
        c.T = T;
        c.fmt = f;
        c.margin = margin;
        c.lead_kind.assign((size_t)S, (int32_t)kIqFromCall);
        c.lead_row.assign((size_t)S, (int32_t)-1);
        c.lead_buf.assign((size_t)S, (int32_t)-1);
        c.lead_D.assign((size_t)S, (int32_t)0);
        c.lead_held.assign((size_t)S, (int32_t)0);
        c.write_buf.assign((size_t)S, (int32_t)-1);
        c.write_D.assign((size_t)S, (int32_t)0);
        c.before_cur = cur;
        c.before_held = held;
        c.before_fmt = fmt;
        // rows a pending call still reads, and every stream's latest
        std::vector<uint8_t> busy((size_t)S, (uint8_t)0);
        if (other && other->on)
            for (int s = 0; s < S; ++s)
                if (other->lead_kind[(size_t)s] == kIqFromTail) busy[(size_t)other->lead_row[(size_t)s]] |= (uint8_t)(1u << other->lead_buf[(size_t)s]);
        for (int s = 0; s < S; ++s)
            if (cur[(size_t)s] >= 0) busy[(size_t)s] |= (uint8_t)(1u << cur[(size_t)s]);
        const int D_new = std::min(T, cols());
        // the leads first: they read the book as it stands before this call's own tails
        for (int s = 0; s < S; ++s) {
            const size_t i = (size_t)s;
            if (absent && absent[i]) continue;
            const int T_pred = n_seg_last[i];
            if (T_pred <= 0) continue;
            if (src_buf && src_buf[i] == 1) {  // the nearest present stream before it in its run, in this call
                c.lead_kind[i] = kIqFromRow;
                c.lead_row[i] = src_idx[i];
                c.lead_D[i] = std::min(T, cols());
                c.lead_held[i] = T;
                continue;
            }
            const int from = (src_buf && src_buf[i] == 2) ? src_idx[i] : s;
            if (from < 0 || cur[(size_t)from] < 0 || fmt[(size_t)from] != f) continue;
            const int D = std::min(T_pred, held[(size_t)from]);
            if (D <= 0) continue;
            c.lead_kind[i] = kIqFromTail;
            c.lead_row[i] = from;
            c.lead_buf[i] = cur[(size_t)from];
            c.lead_D[i] = D;
            c.lead_held[i] = held[(size_t)from];
        }
        for (int s = 0; s < S; ++s) {
            const size_t i = (size_t)s;
            if (absent && absent[i]) continue;
            int w = 0;
            while (w < kIqRows - 1 && (busy[i] >> w & 1)) ++w;
            c.write_buf[i] = w;
            c.write_D[i] = D_new;
            cur[i] = w;
            held[i] = D_new;
            fmt[i] = f;
        }
    }
    void rollback(const IqCall &c) {
        if (!c.on) return;
        cur = c.before_cur;
        held = c.before_held;
        fmt = c.before_fmt;
    }
};

// The delivered records of a call -> offsets [n + 1] (samples), first_seg [n] and the copy list (any of them may be null).
// `rec` points at the first record's `stream` field; `stride` bytes to the next record (rt_record and rt_record_f64 both start with
// int32 stream, fi, start, end).  Returns the samples of all records.
inline int64_t iq_build_descs(const IqCall &c, int N, const void *rec, size_t stride, size_t n, int64_t *offsets, int32_t *first_seg,
                              std::vector<IqDesc> *descs) {
    int64_t total = 0;
    if (offsets) offsets[0] = 0;
    for (size_t i = 0; i < n; ++i) {
        const int32_t *r = reinterpret_cast<const int32_t *>(static_cast<const char *>(rec) + i * stride);
        const int s = r[0], start = r[2], end = r[3];
        const size_t si = (size_t)s;
        const int D = c.lead_D[si];
        const int first = std::max(start - c.margin, -D);
        const int last = std::max(first, std::min(end + c.margin, c.T));  // one past the last segment
        if (first_seg) first_seg[i] = first;
        if (descs) {
            if (first < 0) {
                const int lead_end = std::min(last, 0);
                IqDesc d{};
                d.kind = c.lead_kind[si];
                d.row = c.lead_row[si];
                d.buf = d.kind == kIqFromTail ? c.lead_buf[si] : 0;
                d.src_sample = (int64_t)(c.lead_held[si] + first) * N;
                d.dst_sample = total;
                d.len = (int64_t)(lead_end - first) * N;
                if (d.len > 0) descs->push_back(d);
            }
            if (last > 0) {
                const int from = std::max(first, 0);
                IqDesc d{};
                d.kind = kIqFromCall;
                d.row = s;
                d.src_sample = (int64_t)from * N;
                d.dst_sample = total + (int64_t)(from - first) * N;
                d.len = (int64_t)(last - from) * N;
                if (d.len > 0) descs->push_back(d);
            }
        }
        total += (int64_t)(last - first) * N;
        if (offsets) offsets[i + 1] = total;
    }
    return total;
}

// Every descriptor stays inside its source and inside the pool: the last check in front of a launch (and of the CPU suite).
// `n_samples`: samples of a row of the call; `row_samples`: samples a tail row holds.
inline bool iq_descs_in_bounds(const std::vector<IqDesc> &descs, int S, int64_t n_samples, int64_t row_samples, int64_t total) {
    for (const IqDesc &d : descs) {
        if (d.len <= 0 || d.src_sample < 0 || d.dst_sample < 0 || d.dst_sample + d.len > total) return false;
        if (d.row < 0 || d.row >= S) return false;
        if (d.kind == kIqFromTail) {
            if (d.buf < 0 || d.buf >= kIqRows || d.src_sample + d.len > row_samples) return false;
        } else if (d.kind == kIqFromCall || d.kind == kIqFromRow) {
            if (d.src_sample + d.len > n_samples) return false;
        } else {
            return false;
        }
    }
    return true;
}

// tile -> descriptor: tile_first[i] = tiles of the descriptors before i, [n + 1] entries (bps = bytes per sample)
inline int64_t iq_tile_prefix(const std::vector<IqDesc> &descs, int bps, std::vector<int64_t> *tile_first) {
    tile_first->resize(descs.size() + 1);
    int64_t t = 0;
    for (size_t i = 0; i < descs.size(); ++i) {
        (*tile_first)[i] = t;
        t += (descs[i].len * bps + kIqTileBytes - 1) / kIqTileBytes;
    }
    (*tile_first)[descs.size()] = t;
    return t;
}

}  // namespace rt
#endif
