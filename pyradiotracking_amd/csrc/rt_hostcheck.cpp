// rt_hostcheck.cpp -- HOST build of the scalar decision logic in rt_core.h and of
// the table builders in rt_tables.h, for unit tests only (tests/test_host_core.py,
// tests/test_host_tables.py).  It lets the CPU test-suite drive the exact functions
// the detect kernels execute (predicate, start walk, float64 duration gate,
// statistics, microsecond rounding, ordering + shadow verdict) against the oracle
// and the golden vectors, and read the geometry and the tables a handle hands its
// kernels, without a GPU.
// It is NOT a fallback: the product library (rt_analyze.hip) never links or
// loads this file, and there is no STFT here at all.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <vector>

#include "../../include/rt_analyze.h"
#include "rt_core.h"
#include "rt_input_stats.h"
#include "rt_ledger.h"
#include "rt_record_stft_book.h"
#include "rt_tables.h"

using namespace rt;

extern "C" {

long long hc_timedelta_us(double seconds) { return (long long)timedelta_us(seconds); }

int hc_probe_stride(int nperseg, double fs, double min_d) { return probe_stride(nperseg, fs, min_d); }

double hc_seg_time(int k, int nperseg, double fs) { return seg_time(k, nperseg, fs); }

int hc_tail_cols(int nperseg, double fs, double max_d) { return tail_cols(nperseg, fs, max_d); }

// extract_signals + filter_shadow_signals for ONE stream on a dense,
// segment-major power map: spec[t*F + f].  last = previous map
// [n_seg_last][F] or NULL; tail_cols limits how far back `last` may be read
// (pass n_seg_last for the reference's unlimited look-back).
// Returns the number of records (written up to cap, ordered by (fi, start)).
int hc_extract(const float *spec, int n_seg, int n_bins, const float *last, int n_seg_last, int tail_cols,
               int nperseg, double fs, float thr, float snr, float cal_db, double min_d, double max_d,
               rt_record *out, int cap) {
    DetectParams p;
    p.n_seg = n_seg;
    p.n_seg_last = last ? n_seg_last : -1;
    p.tail_cols = last ? tail_cols : 0;
    p.stride = probe_stride(nperseg, fs, min_d);
    p.nperseg = nperseg;
    p.thr = thr;
    p.snr = snr;
    p.cal_db = cal_db;
    p.fs = fs;
    p.min_d = min_d;
    p.max_d = max_d;
    std::vector<rt_record> rec;
    std::vector<long long> ts, du;
    for (int fi = 0; fi < n_bins; ++fi) {
        auto cur = [&](int t) -> float { return spec[(size_t)t * n_bins + fi]; };
        auto prev = [&](int d) -> float { return last[(size_t)(n_seg_last - d) * n_bins + fi]; };
        float avg = 0.f;
        auto emit = [&](int start, int end, const RunStats &st) {
            rt_record r;
            std::memset(&r, 0, sizeof r);
            r.fi = fi;
            r.start = start;
            r.end = end;
            r.max_p = st.max_p;
            r.mean_p = st.mean_p;
            r.std_db = st.std_db;
            r.row_mean = avg;
            rec.push_back(r);
            ts.push_back(timedelta_us(start_time(p, start)));
            du.push_back(timedelta_us(run_duration(p, start, end)));
        };
        auto on_run = [&](int b, int e, float av) {
            avg = av;
            finish_run(p, b, e, av, cur, prev, emit);
        };
        scan_dense_row(p, cur, -1.0, &avg, on_run);
    }
    const int n = (int)rec.size();
    std::vector<rt_record> ordered(n);
    for (int i = 0; i < n; ++i) {
        int rank, shadow;
        rank_and_shadow(i, n, rec.data(), ts.data(), du.data(), cal_db, &rank, &shadow);
        ordered[rank] = rec[i];
        ordered[rank].shadowed = shadow;
    }
    for (int i = 0; i < n && i < cap; ++i) out[i] = ordered[i];
    return n;
}

// RT_MODE_AUTO's level bookkeeping (rt_core.h)
int hc_level_up(int prefilter_ok, int runfilter_ok, int mode) { return level_up(AutoLevels{prefilter_ok != 0, runfilter_ok != 0}, mode); }
int hc_level_down(int prefilter_ok, int runfilter_ok, int mode) { return level_down(AutoLevels{prefilter_ok != 0, runfilter_ok != 0}, mode); }
int hc_level_rank(int mode) { return level_rank(mode); }
int hc_probe_ruled_out(int target, int level, int valid, unsigned long long abs_hot, unsigned long long list_cells, unsigned long long cells_per_stream) {
    return probe_ruled_out(target, level, valid != 0, abs_hot, list_cells, cells_per_stream) ? 1 : 0;
}

// ---- RT_MODE_AUTO's state machine (rt_core.h: AutoPolicy, overflow_step), operation by operation as rt_analyze.hip calls it ----
void *hc_auto_new(int prefilter_ok, int runfilter_ok) {
    AutoPolicy *p = new AutoPolicy();
    p->lv = AutoLevels{prefilter_ok != 0, runfilter_ok != 0};
    return p;
}
void hc_auto_free(void *p) { delete static_cast<AutoPolicy *>(p); }
// returns the mode the call is enqueued with; *restore_point = what hc_auto_restore takes to undo it
int hc_auto_begin_call(void *p, int cfg_mode, unsigned long long list_cells, unsigned long long cells_per_stream, int *restore_point) {
    AutoPolicy *a = static_cast<AutoPolicy *>(p);
    *restore_point = a->restore_point();
    return a->begin_call(cfg_mode, list_cells, cells_per_stream);
}
void hc_auto_restore(void *p, int restore_point) { static_cast<AutoPolicy *>(p)->restore(restore_point); }
int hc_auto_overflow_step(int mode, int thr_rerun, int thr_stale, int n_bad, int n_streams, int cfg_mode, int prefilter_ok, int runfilter_ok) {
    return overflow_step(mode, thr_rerun != 0, thr_stale != 0, n_bad, n_streams, cfg_mode, AutoLevels{prefilter_ok != 0, runfilter_ok != 0});
}
int hc_auto_climb(void *p, int from, int first) { return static_cast<AutoPolicy *>(p)->climb(from, first != 0); }
// (both halves of what fetch_one tells the policy about a call whose result stands)
void hc_auto_settle(void *p, int settled, int cfg_mode, int mode, int fell_back, int counts, long long n_hot, long long seg_total, long long n_took_part,
                    long long n_seg, long long N, int abs_counted, unsigned abs_hot, int n_dense_streams) {
    AutoPolicy *a = static_cast<AutoPolicy *>(p);
    a->settle(settled != 0, cfg_mode, mode, fell_back != 0, counts != 0, n_hot, seg_total, n_took_part, n_seg, N);
    a->keep_abs_hot(abs_counted != 0, abs_hot, mode, n_dense_streams);
}
// out[5]: level, dense_sticky, sticky_len, abs_hot_seen, abs_hot_valid
void hc_auto_state(void *p, long long *out) {
    const AutoPolicy *a = static_cast<AutoPolicy *>(p);
    out[0] = a->level;
    out[1] = a->dense_sticky;
    out[2] = a->sticky_len;
    out[3] = a->abs_hot_seen;
    out[4] = a->abs_hot_valid ? 1 : 0;
}

// how often a cell of a chunk of L segments is counted by the sampled absolute-threshold bits (rt_core.h: abs_sampled):
// the sampled steps of i = 1 .. L under `phase`, times the period
int hc_abs_sample_period(int L) { return abs_sample_period(L); }
int hc_abs_sampled_weight(int L, int phase) {
    const int P = abs_sample_period(L);
    int n = 0;
    for (int i = 1; i <= L; ++i) n += abs_sampled(i, phase, P) ? P : 0;
    return n;
}
int hc_abs_sampled_segment(int L, int phase, int k) {  // the k-th sampled step (0-based) as a segment offset inside the chunk (seg - c0), or -1
    const int P = abs_sample_period(L);
    for (int i = 1; i <= L; ++i)
        if (abs_sampled(i, phase, P) && k-- == 0) return L - i;
    return -1;
}

int hc_minsum_group(int L, int gpw) { return minsum_group(L, gpw); }
double hc_minsum_margin(int m) { return (double)minsum_margin(m); }

// The planner of the exact run-length pre-filter (rt_core.h: RunPlanner, plan_tile_column -- the arithmetic of the plan_runs
// kernel) on one stream's threshold words hot[n_seg][w] (64-bit words): need[n_seg][w], tiled exactly as the kernel tiles a call
// of n_seg rows of lg = 4 w lanes (tile_rows = 0) or with the given tile length.  Returns the number of counter planes used.
int hc_plan_runs(const unsigned long long *hot, unsigned long long *need, int n_seg, int w, int r_in, int tile_rows) {
    const int r = r_in < n_seg + 1 ? r_in : n_seg + 1;  // (as the host side of the launch clamps it)
    const int B = tile_rows > 0 ? tile_rows : plan_tile_rows(n_seg, 4 * w, r);
    const int planes = r <= 16 ? 4 : r <= 256 ? 8 : 16;
    for (int a = 0; a < n_seg; a += B)
        for (int c = 0; c < w; ++c) {
            auto row = [&](int u) { return hot[(size_t)u * w + c]; };
            auto emit = [&](int t, unsigned long long v) { need[(size_t)t * w + c] = v; };
            if (planes == 4) plan_tile_column<4>(a, B, n_seg, r, row, emit);
            else if (planes == 8) plan_tile_column<8>(a, B, n_seg, r, row, emit);
            else plan_tile_column<16>(a, B, n_seg, r, row, emit);
        }
    return planes;
}
int hc_plan_tile_rows(int n_seg, int lg, int r) { return plan_tile_rows(n_seg, lg, r); }

}  // extern "C"

extern "C" {

// hc_extract on a float64 map with float64 thresholds: the rt_core.h instantiations a float64 handle's kernels run
// (rt_create_f64), records as rt_record_f64.
int hc_extract_f64(const double *spec, int n_seg, int n_bins, const double *last, int n_seg_last, int tail_cols,
                   int nperseg, double fs, double thr, double snr, double cal_db, double min_d, double max_d,
                   rt_record_f64 *out, int cap) {
    DetectParams64 p;
    p.n_seg = n_seg;
    p.n_seg_last = last ? n_seg_last : -1;
    p.tail_cols = last ? tail_cols : 0;
    p.stride = probe_stride(nperseg, fs, min_d);
    p.nperseg = nperseg;
    p.thr = thr;
    p.snr = snr;
    p.cal_db = cal_db;
    p.fs = fs;
    p.min_d = min_d;
    p.max_d = max_d;
    std::vector<rt_record_f64> rec;
    std::vector<long long> ts, du;
    for (int fi = 0; fi < n_bins; ++fi) {
        auto cur = [&](int t) -> double { return spec[(size_t)t * n_bins + fi]; };
        auto prev = [&](int d) -> double { return last[(size_t)(n_seg_last - d) * n_bins + fi]; };
        double avg = 0.0;
        auto emit = [&](int start, int end, const RunStatsT<double> &st) {
            rt_record_f64 r;
            std::memset(&r, 0, sizeof r);
            r.fi = fi;
            r.start = start;
            r.end = end;
            r.max_p = st.max_p;
            r.mean_p = st.mean_p;
            r.std_db = st.std_db;
            r.row_mean = avg;
            rec.push_back(r);
            ts.push_back(timedelta_us(start_time(p, start)));
            du.push_back(timedelta_us(run_duration(p, start, end)));
        };
        auto on_run = [&](int b, int e, double av) {
            avg = av;
            finish_run(p, b, e, av, cur, prev, emit);
        };
        scan_dense_row(p, cur, -1.0, &avg, on_run);
    }
    const int n = (int)rec.size();
    std::vector<rt_record_f64> ordered(n);
    for (int i = 0; i < n; ++i) {
        int rank, shadow;
        rank_and_shadow(i, n, rec.data(), ts.data(), du.data(), cal_db, &rank, &shadow);
        ordered[rank] = rec[i];
        ordered[rank].shadowed = shadow;
    }
    for (int i = 0; i < n && i < cap; ++i) out[i] = ordered[i];
    return n;
}

}  // extern "C"

// The record-cells convention (include/rt_analyze.h: rt_fetch_record_cells) on an explicit map + previous map for ONE stream:
// rt::record_cell -- the indexing the gather kernels use (rt_cells.h) -- for the n records `rec` (hc_extract's).
// offsets[n + 1], cells[cap]; returns the number of cells (nothing is written to `cells` if cap is too small).
namespace {
template <class P, class Rec>
long long record_cells_host(const P *spec, int n_bins, const P *last, int n_seg_last, const Rec *rec, int n, long long *offsets, P *cells, long long cap) {
    long long total = 0;
    offsets[0] = 0;
    for (int i = 0; i < n; ++i) offsets[i + 1] = (total += rec[i].end - rec[i].start);
    if (total > cap) return total;
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < rec[i].end - rec[i].start; ++k)
            cells[offsets[i] + k] = record_cell(spec, last, last ? n_seg_last : 0, n_bins, rec[i].fi, rec[i].start + k);
    return total;
}
}  // namespace

extern "C" {
long long hc_record_cells(const float *spec, int n_bins, const float *last, int n_seg_last, const rt_record *rec, int n, long long *offsets,
                          float *cells, long long cap) {
    return record_cells_host(spec, n_bins, last, n_seg_last, rec, n, offsets, cells, cap);
}
long long hc_record_cells_f64(const double *spec, int n_bins, const double *last, int n_seg_last, const rt_record_f64 *rec, int n,
                              long long *offsets, double *cells, long long cap) {
    return record_cells_host(spec, n_bins, last, n_seg_last, rec, n, offsets, cells, cap);
}
}  // extern "C"

// The geometry and the tables of a handle (rt_core.h, rt_tables.h): thin wrappers, the functions rt_create[_f64] call.
extern "C" {

// out[6]: R3, QS, big, general, bluestein, supported
void hc_scan_family(int nperseg, int *out) {
    const ScanFamily f = scan_family(nperseg);
    const int v[6] = {f.R3, f.QS, f.big, f.general, f.bluestein, f.supported};
    std::memcpy(out, v, sizeof v);
}
// `block`: threads of a scan workgroup (the product passes rt_kernels.h: scan_block(R3))
int hc_choose_chunk(int nperseg, int block, double fs, double min_d, int segs_per_chunk, int n_streams, int n_seg) {
    const ScanFamily f = scan_family(nperseg);
    return choose_chunk(nperseg, f.R3, f.QS, block, fs, min_d, segs_per_chunk, n_streams, n_seg);
}
long long hc_min_run_cells(int nperseg, double fs, double min_d) { return min_run_cells(nperseg, fs, min_d); }
int hc_key_tbits(int n_seg) { return key_tbits(n_seg); }
// out[6]: kBuckets, kSmallBucket, kGroupCells, kGroupBins, kQuarters, kCandCapMax (the size edges of the sparse detection)
void hc_detect_order_constants(int *out) {
    const int v[6] = {kBuckets, kSmallBucket, kGroupCells, kGroupBins, kQuarters, kCandCapMax};
    std::memcpy(out, v, sizeof v);
}
int hc_next_pow2(int v) { return next_pow2(v); }

// n[2]: entries of tw1 / tw2; the tables are copied where the pointers are not null
void hc_scan_twiddles(int N, int R3, int QS, int big, int wave64, cf *tw1, cf *tw2, int *n) {
    const ScanTwiddles t = scan_twiddles(N, R3, QS, big, wave64 != 0);
    n[0] = (int)t.tw1.size();
    n[1] = (int)t.tw2.size();
    if (tw1) std::memcpy(tw1, t.tw1.data(), t.tw1.size() * sizeof(cf));
    if (tw2) std::memcpy(tw2, t.tw2.data(), t.tw2.size() * sizeof(cf));
}
void hc_scaled_window(const float *window, int N, float scale, float *ws) {
    const std::vector<float> v = scaled_window(window, N, scale);
    std::memcpy(ws, v.data(), v.size() * sizeof(float));
}
void hc_window_thread_order(const float *ws, int N, int big, float *out) {
    const std::vector<float> v = window_thread_order(std::vector<float>(ws, ws + N), N, big);
    std::memcpy(out, v.data(), v.size() * sizeof(float));
}
void hc_window_lane_order(const float *ws, int N, int LG, int wave64, float *out) {
    const std::vector<float> v = window_lane_order(std::vector<float>(ws, ws + N), N, LG, wave64 != 0);
    std::memcpy(out, v.data(), v.size() * sizeof(float));
}
int hc_fit_cosine_window(const float *ws, int N, double *wr, double *wi) {
    const CosineFit f = fit_cosine_window(std::vector<float>(ws, ws + N), N);
    std::memcpy(wr, f.wr, sizeof f.wr);
    std::memcpy(wi, f.wi, sizeof f.wi);
    return f.cosine_sum ? 1 : 0;
}
void hc_transform_twiddles_f32(int M, cf *out) {
    const std::vector<cf> v = transform_twiddles<cf, double>(M);
    std::memcpy(out, v.data(), v.size() * sizeof(cf));
}
void hc_transform_twiddles_f64(int M, cd *out) {
    const std::vector<cd> v = transform_twiddles<cd, long double>(M);
    std::memcpy(out, v.data(), v.size() * sizeof(cd));
}
void hc_bluestein_tables_f32(const float *window, int N, int M, int log2m, float scale, cf *cwin, cf *bfilt) {
    const BluesteinTables<cf> t = bluestein_tables<cf, double>(window, N, M, log2m, std::sqrt((double)scale));
    std::memcpy(cwin, t.cwin.data(), t.cwin.size() * sizeof(cf));
    std::memcpy(bfilt, t.bfilt.data(), t.bfilt.size() * sizeof(cf));
}
void hc_bluestein_tables_f64(const double *window, int N, int M, int log2m, cd *cwin, cd *bfilt) {
    const BluesteinTables<cd> t = bluestein_tables<cd, long double>(window, N, M, log2m, 1.0L);
    std::memcpy(cwin, t.cwin.data(), t.cwin.size() * sizeof(cd));
    std::memcpy(bfilt, t.bfilt.data(), t.bfilt.size() * sizeof(cd));
}

// ---- the look-back ledger (rt_ledger.h: StreamLedger, LedgerCall) ----
// The driver a handle runs, with a handle's two call slots (call k in slot k % 2): hc_presence_*, hc_chain_*, hc_iq_* and
// hc_ledger_* are views of this one object.  Only hc_iq_* use the members below `pending`: host-memory stand-ins for the tail
// area and the two kernels of rt_record_iq.h, which are not part of the driver.
struct HcLedger {
    StreamLedger led;
    LedgerCall slot[2];
    unsigned long long n_calls = 0;
    bool pending[2] = {false, false};
    int K = 0, N = 0;
    struct Source {  // the caller's arrays: they must stay alive until their call is fetched, as a handle's callers' must
        const char *data = nullptr;
        int64_t stride = 0;
        int bps = 0;
    } src[2];
    std::vector<char> tails;
    int64_t row_bytes = 0;
    int area_bps = 0;
};
static HcLedger *hc_led(void *h) { return static_cast<HcLedger *>(h); }
static void hc_put(int32_t *dst, const std::vector<int32_t> &v) {
    if (dst) std::memcpy(dst, v.data(), v.size() * sizeof(int32_t));
}
static void hc_presence_copy(const LedgerCall &c, uint8_t *absent, int32_t *n_seg_last, int32_t *tails) {
    if (absent) std::memcpy(absent, c.pc.absent.data(), c.pc.absent.size());
    hc_put(n_seg_last, c.pc.n_seg_last);
    if (tails) {
        tails[0] = c.tail_read;
        tails[1] = c.tail_write;
    }
}
static LedgerCall &hc_begin(HcLedger *p, int T, int fmt) {
    const int idx = (int)(p->n_calls++ % 2);
    const LedgerCall &o = p->slot[1 - idx];
    p->led.begin_call(T, fmt, p->pending[1 - idx] && o.iq_on ? &o.iq : nullptr, p->slot[idx]);
    return p->slot[idx];
}
static bool hc_in_slots(const HcLedger *p, unsigned long long k) { return k < p->n_calls && k + 2 >= p->n_calls; }

// `n_seg_last`: the handle's one segment count so far (-1: none)
void *hc_ledger_new(int n_streams, int n_seg_last) {
    HcLedger *p = new HcLedger();
    p->led.configure(n_streams);
    p->led.n_seg_last = n_seg_last;
    return p;
}
// one call of T segments: rows[S] = look_back_rows, tails[2] = buffer read / written, took[S] = the lock-step resets it took
// (all zero: none); returns the call's number
long long hc_ledger_call(void *h, int T, int32_t *rows, int32_t *tails, uint8_t *took) {
    HcLedger *p = hc_led(h);
    LedgerCall &c = hc_begin(p, T, 0);
    if (rows) std::memcpy(rows, p->led.look_back_rows(c), (size_t)p->led.S * sizeof(int32_t));
    tails[0] = c.tail_read;
    tails[1] = c.tail_write;
    for (int s = 0; took && s < p->led.S; ++s) took[s] = (size_t)s < c.took.size() && c.took[(size_t)s] ? 1 : 0;
    return (long long)p->n_calls - 1;
}
// what call `k` (one of the latest two) was enqueued with
int hc_ledger_snapshot(void *h, unsigned long long k, int32_t *rows, int32_t *tails) {
    HcLedger *p = hc_led(h);
    if (!hc_in_slots(p, k)) return -1;
    LedgerCall &c = p->slot[k % 2];
    std::memcpy(rows, p->led.look_back_rows(c), (size_t)p->led.S * sizeof(int32_t));
    tails[0] = c.tail_read;
    tails[1] = c.tail_write;
    return c.masked ? 1 : 0;
}
void hc_ledger_mark_changed(void *h, const uint8_t *changed) { hc_led(h)->led.mark_changed(std::vector<uint8_t>(changed, changed + hc_led(h)->led.S)); }
void hc_ledger_activate_presence(void *h) { hc_led(h)->led.activate_presence(); }
// scalars[4]: tail_cur, n_seg_last, any_reset(), the per-stream regime is on; reset_pending[S]; per_stream[S] (that regime only)
void hc_ledger_state(void *h, int32_t *scalars, uint8_t *reset_pending, int32_t *per_stream) {
    const StreamLedger &l = hc_led(h)->led;
    scalars[0] = l.tail_cur;
    scalars[1] = l.n_seg_last;
    scalars[2] = l.any_reset() ? 1 : 0;
    scalars[3] = l.pres.active ? 1 : 0;
    std::memcpy(reset_pending, l.reset_pending.data(), l.reset_pending.size());
    if (l.pres.active) hc_put(per_stream, l.pres.n_seg_last);
}
// every vector of slot `idx`'s LedgerCall as (data(), capacity()) in out[2 * n]; returns n
int hc_ledger_call_footprint(void *h, int idx, unsigned long long *out) {
    const LedgerCall &c = hc_led(h)->slot[idx];
    int n = 0;
    const auto put = [&](const auto &v) {
        out[2 * n] = (unsigned long long)reinterpret_cast<uintptr_t>(v.data());
        out[2 * n++ + 1] = (unsigned long long)v.capacity();
    };
    put(c.took), put(c.last);
    put(c.pc.absent), put(c.pc.n_seg_last), put(c.pc.before), put(c.pc.took_reset);
    put(c.cc.src_buf), put(c.cc.src_idx), put(c.cc.before_idx), put(c.cc.before_T);
    put(c.iq.lead_kind), put(c.iq.lead_row), put(c.iq.lead_buf), put(c.iq.lead_D), put(c.iq.lead_held);
    put(c.iq.write_buf), put(c.iq.write_D), put(c.iq.before_cur), put(c.iq.before_held), put(c.iq.before_fmt);
    return n;
}

// ---- streams that sit out a call (rt_core.h: PresenceBook, driven by the ledger) ----
// `all`: the one segment count the handle had when rt_set_present was first called.
void *hc_presence_new(int n_streams, int all) {
    void *h = hc_ledger_new(n_streams, all);
    hc_ledger_activate_presence(h);
    return h;
}
void hc_presence_free(void *h) { delete hc_led(h); }
int hc_presence_set(void *h, const uint8_t *mask) { return hc_led(h)->led.set_mask(mask) ? 1 : 0; }
void hc_presence_reset_stream(void *h, int s) { hc_led(h)->led.reset_stream(s); }
void hc_presence_reset_all(void *h) { hc_led(h)->led.forget_all(); }  // rt_reset
// one call of T segments: its snapshot (absent[S], n_seg_last[S], tails[2] = buffer read / written); returns the streams present
int hc_presence_call(void *h, int T, uint8_t *absent, int32_t *n_seg_last, int32_t *tails) {
    const LedgerCall &c = hc_begin(hc_led(h), T, 0);
    hc_presence_copy(c, absent, n_seg_last, tails);
    return c.pc.n_present;
}
// the snapshot call number `k` (0-based; one of the latest two) was enqueued with: what a re-analysis inside rt_fetch reads
int hc_presence_snapshot(void *h, unsigned long long k, uint8_t *absent, int32_t *n_seg_last, int32_t *tails) {
    HcLedger *p = hc_led(h);
    if (!hc_in_slots(p, k)) return -1;
    hc_presence_copy(p->slot[k % 2], absent, n_seg_last, tails);
    return p->slot[k % 2].pc.n_present;
}
// the newest call is undone
void hc_presence_rollback(void *h) {
    HcLedger *p = hc_led(h);
    if (p->n_calls == 0) return;
    --p->n_calls;
    p->led.rollback(p->slot[p->n_calls % 2]);
    p->pending[p->n_calls % 2] = false;
}
void hc_presence_state(void *h, int32_t *n_seg_last, uint8_t *reset_pending, uint8_t *present) {
    const StreamLedger &l = hc_led(h)->led;
    hc_put(n_seg_last, l.pres.n_seg_last);
    std::memcpy(reset_pending, l.reset_pending.data(), l.reset_pending.size());
    std::memcpy(present, l.pres.present.data(), l.pres.present.size());
}

// ---- consecutive buffers as the streams of one call (rt_core.h: ChainBook, driven by the ledger) ----
// `h` is an hc_presence_new handle.
void hc_chain_set(void *h, int links) { hc_led(h)->led.set_chain(links); }  // (a change forgets all look-back, as rt_set_chain does)
void hc_chain_reset_all(void *h) { hc_led(h)->led.forget_all(); }           // rt_reset
// one chained call of T segments: hc_presence_call's outputs (n_seg_last as the chain rewrites it) and each stream's source
// (src_buf[S]: 0 none, 1 the buffer the call writes, 2 the buffer it reads; src_idx[S])
int hc_chain_call(void *h, int T, uint8_t *absent, int32_t *n_seg_last, int32_t *tails, int32_t *src_buf, int32_t *src_idx, uint8_t *took_reset) {
    const LedgerCall &c = hc_begin(hc_led(h), T, 0);
    hc_presence_copy(c, absent, n_seg_last, tails);
    hc_put(src_buf, c.cc.src_buf);
    hc_put(src_idx, c.cc.src_idx);
    if (took_reset) std::memcpy(took_reset, c.pc.took_reset.data(), c.pc.took_reset.size());
    return c.pc.n_present;
}
int hc_chain_snapshot(void *h, unsigned long long k, int32_t *n_seg_last, int32_t *src_buf, int32_t *src_idx) {
    HcLedger *p = hc_led(h);
    if (!hc_in_slots(p, k)) return -1;
    hc_put(n_seg_last, p->slot[k % 2].pc.n_seg_last);
    hc_put(src_buf, p->slot[k % 2].cc.src_buf);
    hc_put(src_idx, p->slot[k % 2].cc.src_idx);
    return 0;
}
void hc_chain_rollback(void *h) { hc_presence_rollback(h); }
// the first run in which `v` ([S] floats) is not uniform, or -1 (rt_set_stream_params / rt_set_stream_settings on a chained handle)
int hc_chain_first_mixed_run(void *h, const float *v) { return hc_led(h)->led.chain.first_mixed_run(v); }

// ---- the samples behind every record (rt_record_iq_book.h: IqTailBook driven by the ledger, iq_build_descs) ----
// A handle in lock-step until hc_iq_present / hc_iq_chain move it to per-stream rows; three tail rows per stream in host memory,
// the two kernels of rt_record_iq.h restated as memcpy.
void *hc_iq_new(int n_streams, int tail_cols, int nperseg) {
    HcLedger *p = hc_led(hc_ledger_new(n_streams, -1));
    p->K = tail_cols;
    p->N = nperseg;
    p->led.set_iq_margin(tail_cols, -1);
    return p;
}
void hc_iq_free(void *h) { delete hc_led(h); }
// rt_set_record_iq: -1 = refused (calls pending, or m out of range)
int hc_iq_set_margin(void *h, int m) {
    HcLedger *p = hc_led(h);
    if (m > kIqMaxMargin || p->pending[0] || p->pending[1]) return -1;
    if ((m < 0 ? -1 : m) != p->led.iq.margin) {
        p->led.set_iq_margin(p->K, m);
        p->tails.clear();
        p->row_bytes = 0;
        p->area_bps = 0;
    }
    return 0;
}
void hc_iq_present(void *h, const uint8_t *mask) {
    hc_led(h)->led.activate_presence();
    hc_led(h)->led.set_mask(mask);
}
void hc_iq_reset_stream(void *h, int s) { hc_led(h)->led.reset_stream(s); }
void hc_iq_reset_all(void *h) { hc_led(h)->led.forget_all(); }  // rt_reset
int hc_iq_chain(void *h, int links) {  // rt_set_chain
    HcLedger *p = hc_led(h);
    if (p->pending[0] || p->pending[1] || (links >= 2 && p->led.S % links != 0)) return -1;
    p->led.set_chain(links);
    return 0;
}
// rt_process*: a call of T segments in format code `fmt`, `bps` bytes a sample, rows `stride` samples apart at `data`.  Fills, if
// given, the call's snapshot ([S] each) and returns the call's number.
long long hc_iq_call(void *h, int T, int fmt, int bps, const void *data, long long stride, int32_t *lead_kind, int32_t *lead_row, int32_t *lead_buf,
                     int32_t *lead_D, int32_t *write_buf) {
    HcLedger *p = hc_led(h);
    const int idx = (int)(p->n_calls % 2), S = p->led.S;
    p->src[idx] = HcLedger::Source{static_cast<const char *>(data), stride, bps};
    if (p->led.iq.on() && (p->tails.empty() || bps > p->area_bps)) {  // (rt_analyze.hip: iq_tail_area -- every row keeps its place and its bytes)
        const int64_t row = ((int64_t)p->led.iq.cols() * p->N * bps + 15) / 16 * 16;
        std::vector<char> area((size_t)(kIqRows * S) * (size_t)row);
        for (int64_t r = 0; !p->tails.empty() && r < (int64_t)kIqRows * S; ++r)
            std::memcpy(area.data() + r * row, p->tails.data() + r * p->row_bytes, (size_t)p->row_bytes);
        p->tails.swap(area);
        p->row_bytes = row;
        p->area_bps = bps;
    }
    const LedgerCall &c = hc_begin(p, T, fmt);
    p->pending[idx] = true;
    if (c.iq_on) {
        for (int s = 0; s < S; ++s) {  // iq_tails
            const int buf = c.iq.write_buf[(size_t)s], D = c.iq.write_D[(size_t)s];
            if (buf < 0 || D <= 0) continue;
            std::memcpy(p->tails.data() + ((int64_t)buf * S + s) * p->row_bytes, p->src[idx].data + ((int64_t)s * stride + (int64_t)(T - D) * p->N) * bps,
                        (size_t)((int64_t)D * p->N * bps));
        }
        hc_put(lead_kind, c.iq.lead_kind);
        hc_put(lead_row, c.iq.lead_row);
        hc_put(lead_buf, c.iq.lead_buf);
        hc_put(lead_D, c.iq.lead_D);
        hc_put(write_buf, c.iq.write_buf);
    }
    return (long long)p->n_calls - 1;
}
// the newest call is undone (a failed rt_process*, or a later lane's): -1 if there is none pending
int hc_iq_rollback(void *h) {
    HcLedger *p = hc_led(h);
    if (p->n_calls == 0 || !p->pending[(p->n_calls - 1) % 2]) return -1;
    hc_presence_rollback(h);
    return 0;
}
// rt_fetch + rt_fetch_record_iq of call `k`: `rec` = n records as int32 (stream, fi, start, end), in delivery order.  Writes
// offsets [n + 1] and first_seg [n], and -- when `cap_bytes` holds them -- the samples; the call is consumed.  Returns the bytes
// of the samples, -1: no such pending call, -2: the call was enqueued with the feature off, -3: a descriptor out of bounds.
long long hc_iq_fetch(void *h, unsigned long long k, const int32_t *rec, long long n, int64_t *offsets, int32_t *first_seg, void *out, long long cap_bytes,
                      long long *n_descs) {
    HcLedger *p = hc_led(h);
    if (!hc_in_slots(p, k) || !p->pending[k % 2]) return -1;
    const LedgerCall &c = p->slot[k % 2];
    const HcLedger::Source &src = p->src[k % 2];
    p->pending[k % 2] = false;
    if (!c.iq_on) return -2;
    std::vector<IqDesc> descs;
    const int64_t total = iq_build_descs(c.iq, p->N, rec, 4 * sizeof(int32_t), (size_t)n, offsets, first_seg, &descs);
    if (n_descs) *n_descs = (long long)descs.size();
    if (!iq_descs_in_bounds(descs, p->led.S, (int64_t)c.iq.T * p->N, (int64_t)p->led.iq.cols() * p->N, total)) return -3;
    std::vector<int64_t> tile_first;
    if (iq_tile_prefix(descs, src.bps, &tile_first) < (int64_t)descs.size()) return -3;  // (every descriptor holds a tile)
    if (out && cap_bytes >= total * src.bps)
        for (const IqDesc &d : descs) {  // record_iq_gather
            const char *from = d.kind == kIqFromTail ? p->tails.data() + ((int64_t)d.buf * p->led.S + d.row) * p->row_bytes + d.src_sample * src.bps
                                                     : src.data + ((int64_t)d.row * src.stride + d.src_sample) * src.bps;
            std::memcpy(static_cast<char *>(out) + d.dst_sample * src.bps, from, (size_t)(d.len * src.bps));
        }
    return (long long)(total * src.bps);
}

}  // extern "C"

// ---- the map-free float64 path (RT_FLAG_F64_SPARSE; rt_core.h, kernels in rt_f64_sparse.h) ----
extern "C" {

// The sequential twin of detect_sparse_f64 + finalize_sparse_f64 for ONE stream: records from a cell list.  keys[n] / vals[n]:
// the stream's candidate cells (f64_cell_key, power) in any order; row_sums[n_bins]: every row's float64 sum; last /
// n_seg_last / tail_cols as in hc_extract_f64.  Returns the number of records (written up to cap, ordered by (fi, start)).
int hc_extract_sparse_f64(const uint32_t *keys_in, const double *vals_in, int n, const double *row_sums, int n_seg, int n_bins,
                          const double *last, int n_seg_last, int tail_cols, int nperseg, double fs, double thr, double snr,
                          double cal_db, double min_d, double max_d, rt_record_f64 *out, int cap) {
    DetectParams64 p;
    p.n_seg = n_seg;
    p.n_seg_last = last ? n_seg_last : -1;
    p.tail_cols = last ? tail_cols : 0;
    p.stride = probe_stride(nperseg, fs, min_d);
    p.nperseg = nperseg;
    p.thr = thr;
    p.snr = snr;
    p.cal_db = cal_db;
    p.fs = fs;
    p.min_d = min_d;
    p.max_d = max_d;
    std::vector<int> order((size_t)n);
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [&](int a, int b) { return keys_in[a] < keys_in[b]; });
    auto keys = [&](int j) -> uint32_t { return keys_in[order[(size_t)j]]; };
    auto vals = [&](int j) -> double { return vals_in[order[(size_t)j]]; };
    std::vector<rt_record_f64> rec;
    std::vector<long long> ts, du;
    for (int j = 0; j < n; ++j) {
        const int fi = f64_key_bin(keys(j));
        if (fi >= n_bins) continue;
        const double avg = row_mean_of(row_sums[fi], n_seg, double());
        int b, e, start;
        if (!sparse_run_at(p, keys, vals, n, j, avg, &b, &e)) continue;
        auto prev = [&](int d) -> double { return last[(size_t)(n_seg_last - d) * n_bins + fi]; };
        if (!gate_run(p, b, e, avg, prev, &start)) continue;
        const int at0 = j - b;  // the list entry of the bin's segment 0, were it there
        auto cell = [&](int32_t k) -> double {
            const int32_t t = start + k;
            return t < 0 ? prev(-t) : vals(at0 + t);
        };
        const RunStatsT<double> st = run_stats(e - start, cell);
        rt_record_f64 r;
        std::memset(&r, 0, sizeof r);
        r.fi = fi;
        r.start = start;
        r.end = e;
        r.max_p = st.max_p;
        r.mean_p = st.mean_p;
        r.std_db = st.std_db;
        r.row_mean = avg;
        rec.push_back(r);
        ts.push_back(timedelta_us(start_time(p, start)));
        du.push_back(timedelta_us(run_duration(p, start, e)));
    }
    const int m = (int)rec.size();
    std::vector<rt_record_f64> ordered((size_t)m);
    for (int i = 0; i < m; ++i) {
        int rank, shadow;
        rank_and_shadow(i, m, rec.data(), ts.data(), du.data(), cal_db, &rank, &shadow);
        ordered[(size_t)rank] = rec[(size_t)i];
        ordered[(size_t)rank].shadowed = shadow;
    }
    for (int i = 0; i < m && i < cap; ++i) out[i] = ordered[(size_t)i];
    return m;
}

// the geometry rt_create_f64 derives for such a handle
unsigned hc_f64_cell_key(int fi, int t) { return f64_cell_key(fi, t); }
int hc_f64_key_bin(unsigned key) { return f64_key_bin(key); }
int hc_f64_key_seg(unsigned key) { return f64_key_seg(key); }
int hc_f64_key_max_seg(void) { return kF64KeyMaxSeg; }
int hc_f64_sparse_nperseg_ok(int n) { return f64_sparse_nperseg_ok(n) ? 1 : 0; }
int hc_f64_sparse_hot_capacity(int hot_capacity) { return f64_sparse_hot_capacity(hot_capacity); }
int hc_f64_sparse_group(int nperseg) { return f64_sparse_group(nperseg); }
int hc_f64_sparse_chunk(int nperseg, int segs_per_chunk, int n_streams, int max_seg) { return f64_sparse_chunk(nperseg, segs_per_chunk, n_streams, max_seg); }
int hc_f64_sparse_chunks(int n_seg, int L) { return f64_sparse_chunks(n_seg, L); }
int hc_f64_sparse_last_chunk(int n_seg, int L) { return f64_sparse_last_chunk(n_seg, L); }

// ---- RT_FLAG_F64_RESCUE (rt_core.h: f64_rescue_rounds; kernels in rt_f64_rescue.h) ----
long long hc_f64_rescue_budget(void) { return (long long)kF64RescueBudget; }
// out[2]: streams per round, rounds
void hc_f64_rescue_rounds(int n_bad, int n_seg, int nperseg, long long budget, int *out) {
    const F64RescueRounds r = f64_rescue_rounds(n_bad, n_seg, nperseg, (int64_t)budget);
    out[0] = r.per_round;
    out[1] = r.rounds;
}

// The sequential twin of detect_list_f64 + stats_list_f64 + finalize_sparse_f64 for ONE stream: the dense row walk over the
// stream's map spec[t * n_bins + f] with every row's sum GIVEN (row_sums[n_bins]: the scan's chunk-ordered fold, not a fresh
// sum of the row) and the look-back as in hc_extract_f64.  Returns the number of records (written up to cap, ordered by
// (fi, start)): byte for byte hc_extract_sparse_f64's on the list the emission rule makes of the same map.
int hc_extract_rescue_f64(const double *spec, const double *row_sums, int n_seg, int n_bins, const double *last, int n_seg_last,
                          int tail_cols, int nperseg, double fs, double thr, double snr, double cal_db, double min_d, double max_d,
                          rt_record_f64 *out, int cap) {
    DetectParams64 p;
    p.n_seg = n_seg;
    p.n_seg_last = last ? n_seg_last : -1;
    p.tail_cols = last ? tail_cols : 0;
    p.stride = probe_stride(nperseg, fs, min_d);
    p.nperseg = nperseg;
    p.thr = thr;
    p.snr = snr;
    p.cal_db = cal_db;
    p.fs = fs;
    p.min_d = min_d;
    p.max_d = max_d;
    std::vector<rt_record_f64> rec;
    std::vector<long long> ts, du;
    for (int fi = 0; fi < n_bins; ++fi) {
        auto cur = [&](int t) -> double { return spec[(size_t)t * n_bins + fi]; };
        auto prev = [&](int d) -> double { return last[(size_t)(n_seg_last - d) * n_bins + fi]; };
        double avg = 0.0;
        auto on_run = [&](int b, int e, double av) {
            int start;
            if (!gate_run(p, b, e, av, prev, &start)) return;
            auto cell = [&](int32_t k) -> double {
                const int32_t t = start + k;
                return t < 0 ? prev(-t) : cur(t);
            };
            const RunStatsT<double> st = run_stats(e - start, cell);
            rt_record_f64 r;
            std::memset(&r, 0, sizeof r);
            r.fi = fi;
            r.start = start;
            r.end = e;
            r.max_p = st.max_p;
            r.mean_p = st.mean_p;
            r.std_db = st.std_db;
            r.row_mean = av;
            rec.push_back(r);
            ts.push_back(timedelta_us(start_time(p, start)));
            du.push_back(timedelta_us(run_duration(p, start, e)));
        };
        scan_dense_row(p, cur, row_sums[fi], &avg, on_run);
    }
    const int m = (int)rec.size();
    std::vector<rt_record_f64> ordered((size_t)m);
    for (int i = 0; i < m; ++i) {
        int rank, shadow;
        rank_and_shadow(i, m, rec.data(), ts.data(), du.data(), cal_db, &rank, &shadow);
        ordered[(size_t)rank] = rec[(size_t)i];
        ordered[(size_t)rank].shadowed = shadow;
    }
    for (int i = 0; i < m && i < cap; ++i) out[i] = ordered[(size_t)i];
    return m;
}

}  // extern "C"

// ---- rt_fetch_record_stft: the work list, the twiddle table and sqrt(scale) (rt_record_stft_book.h, rt_tables.h) ----
extern "C" {

// offsets [n + 1] (samples) and fi [n] -> seg_first [n + 1], fi_out [n]; returns the delivered segments, -1: refused
long long hc_stft_work(const int64_t *offsets, const int32_t *fi, long long n, int nperseg, int64_t *seg_first, int32_t *fi_out) {
    StftWork w;
    const int64_t cells = stft_build_work(offsets, fi, (size_t)n, nperseg, &w);
    if (cells < 0) return -1;
    std::copy(w.seg_first.begin(), w.seg_first.end(), seg_first);
    std::copy(w.fi.begin(), w.fi.end(), fi_out);
    return (long long)cells;
}
int hc_stft_record_of(const int64_t *seg_first, int n, long long g) { return stft_record_of(seg_first, n, (int64_t)g); }
// rt_fetch_record_stft_hop's frame plan: -> frame_first [n + 1], pool_seg [n], lp [n], fi_out [n]; returns the frames, -1: refused
long long hc_stft_hop_work(const int64_t *offsets, const int32_t *first_seg, const int32_t *fi, long long n, int nperseg, int k, int64_t *frame_first,
                           int64_t *pool_seg, int32_t *lp, int32_t *fi_out) {
    StftHopWork w;
    const int64_t frames = stft_hop_build_work(offsets, first_seg, fi, (size_t)n, nperseg, k, &w);
    if (frames < 0) return -1;
    std::copy(w.frame_first.begin(), w.frame_first.end(), frame_first);
    std::copy(w.pool_seg.begin(), w.pool_seg.end(), pool_seg);
    std::copy(w.lp.begin(), w.lp.end(), lp);
    std::copy(w.fi.begin(), w.fi.end(), fi_out);
    return (long long)frames;
}
// out: record, part, pool sample of frame g
void hc_stft_hop_frame_at(const int64_t *frame_first, const int64_t *pool_seg, const int32_t *lp, int n, int nperseg, int k, long long g, int64_t *out) {
    const StftHopFrame f = stft_hop_frame_at(frame_first, pool_seg, lp, n, nperseg, k, (int64_t)g);
    out[0] = f.record;
    out[1] = f.part;
    out[2] = f.sample;
}
// rt_fetch_record_band: the argument rule, column j's bin, the pool's complex values (-1: the product leaves 64 bits)
int hc_stft_band_ok(int nperseg, int k, int w) { return stft_band_ok(nperseg, k, w) ? 1 : 0; }
int hc_stft_band_bin(int fi, int j, int w, int nperseg) { return stft_band_bin(fi, j, w, nperseg); }
long long hc_stft_band_elems(long long frames, int w) { return (long long)stft_band_elems((int64_t)frames, w); }
// rt_fetch_record_estimates' plan: -> frame_first [n + 1], lp [n], range [n][4], base [n][2], fmod [n], turn [k][2]; returns the
// frames, -1: refused (nothing is written then)
long long hc_estimates_work(const int64_t *offsets, const int32_t *first_seg, const int32_t *fi, const int32_t *start, const int32_t *end, long long n,
                            int nperseg, int k, int64_t *frame_first, int32_t *lp, int32_t *range, int64_t *base, int32_t *fmod, double *turn) {
    EstimatesWork w;
    const int64_t frames = estimates_build_work(offsets, first_seg, fi, start, end, (size_t)n, nperseg, k, &w);
    if (frames < 0) return -1;
    std::copy(w.frame_first.begin(), w.frame_first.end(), frame_first);
    std::copy(w.lp.begin(), w.lp.end(), lp);
    std::copy(w.range.begin(), w.range.end(), range);
    std::copy(w.base.begin(), w.base.end(), base);
    std::copy(w.fmod.begin(), w.fmod.end(), fmod);
    if (turn) estimates_turn_table(k, turn);
    return (long long)frames;
}
// The argument rules of rt_fetch_record_band and _spectrum (k, w) and of rt_fetch_record_stft_hop and _estimates (k): the refusal's
// text into `out` (cut to cap - 1 characters), its length; 0: accepted
static int refusal_out(const std::string &why, char *out, int cap) {
    if (out && cap > 0) {
        const size_t n = std::min(why.size(), (size_t)cap - 1);
        std::memcpy(out, why.data(), n);
        out[n] = 0;
    }
    return (int)why.size();
}
int hc_spectrum_refusal(int nperseg, int k, int w, char *out, int cap) { return refusal_out(spectrum_refusal(nperseg, k, w), out, cap); }
int hc_stft_hop_refusal(int nperseg, int k, char *out, int cap) { return refusal_out(stft_hop_refusal(nperseg, k), out, cap); }
long long hc_spectrum_pool_bytes(long long n, int w) { return (long long)spectrum_pool_bytes((size_t)n, w); }
float hc_stft_root_f32(float scale) { return stft_root_f32(scale); }
double hc_stft_root_f64(double scale) { return stft_root_f64(scale); }
// out: [nperseg] interleaved (re, im)
void hc_stft_twiddles_f32(int nperseg, float *out) {
    const std::vector<cf> tw = record_stft_twiddles<cf, double>(nperseg);
    std::memcpy(out, tw.data(), tw.size() * sizeof(cf));
}
void hc_stft_twiddles_f64(int nperseg, double *out) {
    const std::vector<cd> tw = record_stft_twiddles<cd, long double>(nperseg);
    std::memcpy(out, tw.data(), tw.size() * sizeof(cd));
}

// rt_fetch_input_stats (rt_input_stats.h): the chunk length, one stream's row as the kernels form it -- fmt 0 complex64, 1 uint8,
// 2 int16, 3 int8, 4 complex128; -1: no such format -- and the packed form of the 8-bit rule beside the rule itself on the same
// words: n_rail, sum_i, sum_q, sum_sq, peak each
int hc_input_stats_chunk() { return kInputStatsChunk; }
int hc_input_stats(int fmt, const void *ptr, long long n, rt_input_stats *out) { return input_stats_host(fmt, ptr, (int64_t)n, out) ? 0 : -1; }
}  // extern "C"
template <int FMT>
static void input_stats_words(const uint32_t *x, int n_words, long long *packed, long long *rule) {
    InputStatsPart<int64_t> a, b;
    stats_clear(a);
    stats_clear(b);
    StatsWords8 w;
    for (int i = 0; i < n_words; ++i) stats_word8<FMT>(w, x[i]);
    stats_words8_close<FMT>(a, w);
    stats_samples_int<FMT>(b, reinterpret_cast<const char *>(x), (int64_t)n_words * 2);
    const InputStatsPart<int64_t> *const both[2] = {&a, &b};
    long long *const out[2] = {packed, rule};
    for (int k = 0; k < 2; ++k) {
        out[k][0] = both[k]->n_rail;
        out[k][1] = both[k]->sum_i;
        out[k][2] = both[k]->sum_q;
        out[k][3] = both[k]->sum_sq;
        out[k][4] = both[k]->peak;
    }
}
extern "C" {
int hc_input_stats_words8(int fmt, const uint32_t *x, int n_words, long long *packed, long long *rule) {
    if (fmt == kStatsU8) input_stats_words<kStatsU8>(x, n_words, packed, rule);
    else if (fmt == kStatsI8) input_stats_words<kStatsI8>(x, n_words, packed, rule);
    else return -1;
    return 0;
}

}  // extern "C"
