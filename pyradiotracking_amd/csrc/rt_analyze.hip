// rt_analyze.hip -- host side of the C-ABI declared in include/rt_analyze.h:
// handle, device scratch, kernel launches.  gfx950 only; fails loudly when no
// GPU is usable (there is no CPU fallback in the product path).
//
// Execution model of one handle
//   * two "slots" of per-call scratch (candidate lists, partial row sums,
//     record pool, counters, pinned mirrors), used alternately: the scan of
//     call k+1 may run while call k is still being detected / fetched;
//   * scan, detect kernels and readback of a call run in order on one stream
//     (the caller's stream if one was given).  Overlapping detect k with scan
//     k+1 on a second stream was measured and rejected: the scan's 3 waves/SIMD
//     x 151 VGPRs leave no register space for co-resident detect waves, so they
//     starve until the scan drains (profiles/r01_d_*).  What the two slots buy
//     is host-side pipelining: call k+1 is enqueued before call k is fetched,
//     so the GPU never waits for the host;
//   * three look-back tail buffers in rotation: call k reads (k-1)%3 and writes
//     k%3, so the scan of call k+1 never overwrites what detect k still reads;
//   * rt_fetch returns calls in FIFO order (at most two are in flight).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "rt_kernels.h"
#include "rt_general.h"
#include "rt_f64.h"
#include "rt_f64_sparse.h"
#include "rt_f64_rescue.h"
#include "rt_cells.h"
#include "rt_present.h"
#include "rt_chain.h"
#include "rt_record_iq.h"
#include "rt_record_stft.h"
#include "rt_record_stft_hop.h"
#include "rt_record_band.h"
#include "rt_record_estimates.h"
#include "rt_record_spectrum.h"
#include "rt_input_stats.h"
#include "rt_record_stft_book.h"
#include "rt_ledger.h"
#include "rt_tables.h"

using namespace rt;

namespace {

thread_local std::string g_create_error;
// (diagnostic builds: RT_TRACE_FETCH=1 prints every decision of fetch_one's re-run loop)
#define RT_TRACE_FETCH(h, sl, what)                                                                                                          \
    do {                                                                                                                                     \
        if (RT_DIAG_ENV("RT_TRACE_FETCH"))                                                                                                   \
            std::fprintf(stderr, "fetch seq %llu mode %d: %s | flags %llx records %llu wanted/stream %llu rec_cap %d (ran with %d) pool %lld grown %d/%d\n", \
                         (unsigned long long)(sl).call.seq, (sl).call.mode_used, what, (unsigned long long)(sl).h_counters[2],                \
                         (unsigned long long)(sl).h_counters[0], (unsigned long long)(sl).h_counters[4], (h)->rec_cap, (sl).call.rec_cap_used, \
                         (long long)(sl).pool_cap, (sl).call.cap_grown, (int)(sl).call.pool_grown);                                          \
    } while (0)
constexpr uint32_t kFlagLaneOfLargeBatch = 0x40000000u;  // rt_config.flags of a lane's own handle (internal): the whole batch has >= 1 024 streams
thread_local bool g_creating_lane = false;  // rt_create of a laned handle is creating one of its lanes

// bytes of a sample on a float32 handle, by input format (rt_kernels.h: kFmt*)
constexpr size_t fmt_sample_bytes(int fmt) { return (fmt == kFmtU8 || fmt == kFmtI8) ? 2u : fmt == kFmtI16 ? 4u : sizeof(cf); }
constexpr int kTails = 3;  // (kSlots, kMaxPartial: rt_core.h)
constexpr int64_t kInitialPoolRecords = 4 << 20;  // pinned record pool per slot at rt_create unless rt_config.record_pool says otherwise
                                                  // (4 Mi records = 160 MiB); a call that needs more grows it (grow_pool), up to what
                                                  // n_streams * record_capacity can ever deliver
constexpr int64_t kInitialPoolCells = 4 << 20;    // RT_FLAG_RECORD_CELLS: device cell pool per slot at rt_create (or 16 cells per record of the record pool,
                                                  // if that is less); a call that needs more grows it (grow_cells) and is analysed again

struct CallCtx {
    bool pending = false;   // enqueued, not fetched yet
    uint64_t seq = 0;       // call number (0 = slot never used)
    const void *iq = nullptr;
    int64_t n_samples = 0;
    int64_t stream_stride = 0;
    int n_seg = 0;
    int tail_read = 0, tail_write = 0;
    int n_seg_last = -1;    // columns of the previous buffer (-1: none)
    int mode_used = 0;
    bool fell_back = false;
    bool is_extract = false;
    int fmt = kFmtC64;      // the format the IQ was enqueued in: complex64, interleaved uint8 (RTL-SDR wire format), int16 (CS16) or int8 (CS8)
    int n_dense_streams = 0;  // streams of this call that were re-run dense on their own (AUTO, partial fall-back)
    int pool_grown = 0;       // times the record pool was enlarged for this call and the call analysed again (fetch_one)
    int cap_grown = 0;        // times the handle's per-stream record capacity was enlarged for this call (fetch_one: grow_record_capacity)
    int rec_cap_used = 0;     // the per-stream record capacity its kernels ran with (a call in flight while ANOTHER call grew the capacity was still truncated at the old one)
    bool thr_rerun = false;   // analysed again on RT_MODE_RUNFILTER with thresholds from its own row means (once per call)
    bool abs_counted = false; // a MODE 4 / 6 scan of this call left the slot's h_abs_hot
    bool level_settled = false;  // AutoPolicy::settle has seen this call (fetch_one passes over a call twice: size query / peek, then delivery)
    bool ran_lin = false;     // its scans detrended by linearity (fetch_one: analysed again if the guard marks a stream)
    uint64_t sub_epoch = 0;   // rt_handle::sub_epoch when its kernels were enqueued
    int cells_grown = 0;      // times the slot's cell pool was enlarged for this call and the call analysed again (RT_FLAG_RECORD_CELLS)
    // handle state before this call (restored when the call is rolled back: a later lane failed to enqueue)
    int prev_auto = 0 /* AutoPolicy::restore_point */, prev_minsum_slot = -1;
};

constexpr int kRowMeansNone = -1, kRowMeansExtract = -2;  // rt_handle::rm_slot / F64State::rm_slot without valid row means

struct Slot {
    uint2 *d_hot = nullptr;
    uint32_t *d_hot_count = nullptr;
    uint32_t *d_hot_seen = nullptr;
    int32_t *d_items = nullptr;       // [S][max_blocks][GPW] chunks of pass B's workgroups, then [S] their number per stream (with d_full)
    int32_t *h_hot_total = nullptr;   // pinned, [S]
    float *d_psum = nullptr;
    uint16_t *d_full = nullptr;       // [S][max_chunks][LG] chunk bits of the run-length pre-filter, then [S][L][LG] bits of chunk 0 by segment (null: not available)
    uint16_t *d_cell_hot = nullptr, *d_cell_need = nullptr;  // [S][max_seg][LG] threshold bits of every cell / the cells to emit (RT_MODE_RUNFILTER)
    uint32_t *d_abs_hot = nullptr;    // [S] cells at or above the absolute threshold per stream (StftParams::abs_hot; zero between calls)
    uint32_t *h_abs_hot = nullptr;    // pinned: their maximum over the streams, of this slot's latest MODE 4 / 6 scan
    float *d_thr_bin = nullptr, *d_thr_nat = nullptr;  // [S][N] per-bin thresholds of the exact pre-filter for this slot's call, lane order / bin order
                                      // (make_bin_thresholds; per slot: the check of call k reads them beside the scan of call k + 1)
    int min_items = 0;                // rows per stream of the minima d_chunk_min holds (= the work items per stream of the scan that wrote them; 0: none)
    uint64_t min_seq = 0;             // ... and the number of the call they are of
    uint32_t *d_chunk_min = nullptr;  // [S][items][N] float bits: per work item and bin the smallest complete-chunk sum of this slot's latest call (StftParams::chunk_min)
    int32_t *d_seg_list = nullptr;    // [S][max_seg] segments holding such cells, then [S] their number per stream and [1] the batch's total
    int32_t *h_seg_total = nullptr;   // pinned: that total, copied behind plan_runs
    rt_record *d_raw = nullptr;
    int32_t *d_raw_count = nullptr;
    unsigned long long *d_counters = nullptr;  // 4 words (atomics: device memory)
    // Results are written by the finalize/detect kernels straight into pinned, device-visible
    // host memory (no copy kernels); only the counter words are copied (32 bytes).
    unsigned long long *h_counters = nullptr;
    int32_t *h_rec_offset = nullptr, *h_rec_count = nullptr;  // [S]
    rt_record *h_records = nullptr;                            // [pool_cap]
    int64_t pool_cap = 0;                                      // records the slot's pool holds (grows on demand, grow_pool)
    int32_t *h_no_last = nullptr;                              // pinned, [S]: streams without a previous buffer in this call
    int32_t *h_overflow = nullptr;                             // pinned, [S]: set by detect_bucket for a stream whose candidate lists overflowed
    int32_t *h_incons = nullptr;                               // pinned, [S]: ... and for one in which a run lacked its preceding cell
    int32_t *h_dc_flag = nullptr;                              // pinned, [S]: set by a LIN scan for a stream whose constant offset is too large for that form (StftParams::dc_flag)
    int32_t *h_list = nullptr;                                 // pinned, [kMaxPartial]: the streams of a partial dense re-run (read by the kernels)
    unsigned long long *h_total = nullptr;                     // pinned: records allocated so far, uploaded before a partial re-run
    float *d_row_means = nullptr;                              // [S][N] the call's row means (RT_FLAG_ROW_MEANS only; rt_fetch_row_means copies them)
    // RT_FLAG_RECORD_CELLS only (rt_cells.h; rt_fetch_record_cells copies the cells):
    float *d_cells = nullptr;                                  // the cells of the call's records, in delivery order
    int64_t cell_cap = 0;                                      // cells the pool holds (grows on demand, grow_cells)
    uint32_t *d_hot_kept = nullptr;                            // [S][kBuckets] the candidate counters as they were in front of finalize_records
    long long *d_stream_cells = nullptr, *d_stream_base = nullptr;  // [S] cells of each stream's records / its first cell in the pool
    unsigned long long *h_cells_info = nullptr;                // pinned: [0] cells the call wants, [1] a record's cells were not all found
    // rt_set_present only (allocated by the handle's first call of the entry).  The snapshot a call was enqueued with -- every
    // analysis of the call inside rt_fetch uses it again -- and its device form, kMaskRows rows of [S] (pinned copy beside it):
    int32_t *h_mask = nullptr, *d_mask = nullptr;
    int n_lin_present = 0, n_sub_present = 0, n_absent = 0;  // entries of the rows kMaskLinList / kMaskSubList / kMaskAbsentList
    // rt_set_chain only (allocated by the handle's first call of the entry with links >= 2).  The sources a call was enqueued with
    // (rt_core.h: ChainCall), their device form -- two rows of [S]: ChainCall::src_buf, src_idx (pinned copy beside it) -- and the
    // look-back columns its detection reads, [S][K][N] as a rotation buffer (rt_chain.h: chain_tails writes them):
    int32_t *h_chain_rows = nullptr, *d_chain_rows = nullptr;
    float *d_chain = nullptr;
    hipEvent_t ev_begin = nullptr, ev_first = nullptr, ev_scan = nullptr, ev_done = nullptr;  // first launch; end of the first scan; end of the scans; end of the call
    CallCtx call;
    LedgerCall lc;  // what the ledger decided for `call` (rt_ledger.h): the mask, chain and record-IQ rows above are its device form
};
// rows of Slot::d_mask
enum : int {
    kMaskAbsent = 0,      // non-zero: the stream sits the call out (DetectArgs::absent and its like)
    kMaskLinList = 1,     // the present streams the detrend guard has not marked, ascending (StftParams::stream_list of the LIN scan)
    kMaskList = 2,        // the present streams, ascending (StftParams::stream_list of the other scans)
    kMaskSubList = 3,     // the present ones among the marked streams (the subtract-first launch behind a LIN scan)
    kMaskNSegLast = 4,    // columns of each stream's own previous buffer (DetectArgs::n_seg_last_s)
    kMaskAbsentList = 5,  // the absent streams (carry_tails)
    kMaskRows = 6
};

// A float64 handle (rt_create_f64; kernels: rt_f64.h).  Its own two call slots, three look-back tails in rotation as on the
// float32 path, one float64 map shared by the calls (a call analysed again -- its records outgrew the capacity -- runs its
// transform again from its IQ, which stays valid until the call is fetched).
struct F64Slot {
    bool pending = false;
    uint64_t seq = 0;
    bool is_extract = false;
    int fmt = kFmtC64;  // (as CallCtx::fmt)
    const void *iq = nullptr;  // device IQ of the call (the caller's, or d_stage)
    int64_t stream_stride = 0;
    int n_seg = 0, n_seg_last = -1, tail_read = 0, tail_write = 0;
    const double *ex_spec = nullptr, *ex_last = nullptr;  // rt_extract_f64
    int ex_bins = 0, ex_last_cols = 0;
    int rec_cap = 0;                                   // records per stream the slot's areas hold
    rt_record_f64 *d_raw = nullptr;                    // [S][rec_cap]
    int32_t *d_raw_count = nullptr;                    // [S]
    int32_t *d_no_last = nullptr;                      // [S]
    rt_record_f64 *h_out = nullptr;                    // pinned, device-visible: [S * rec_cap] the call's records
    double *d_row_means = nullptr;                     // [S][N] the call's row means (RT_FLAG_ROW_MEANS only; rt_fetch_row_means_f64 copies them)
    int32_t *h_meta = nullptr;                         // pinned, device-visible: [S + 1] offsets + total, then [S] wanted
    void *d_stage = nullptr;                           // rt_process_host / rt_process_u8_host / rt_process_i16_host / rt_process_i8_host
    size_t stage_bytes = 0;
    // RT_FLAG_RECORD_CELLS only, as in Slot:
    double *d_cells = nullptr;
    int64_t cell_cap = 0;
    long long *d_stream_cells = nullptr, *d_stream_base = nullptr;
    unsigned long long *h_cells_info = nullptr;
    // rt_set_present only, as in Slot (rows kMaskAbsent, kMaskNSegLast and kMaskAbsentList are used)
    int32_t *h_mask = nullptr, *d_mask = nullptr;
    int n_absent = 0;
    // RT_FLAG_F64_SPARSE only: the call's candidate lists (rt_f64_sparse.h)
    uint32_t *d_keys = nullptr;    // [S][hot_cap]
    double *d_vals = nullptr;      // [S][hot_cap]
    int32_t *d_cell_count = nullptr;  // [S], zero between calls
    int32_t *h_hot = nullptr;      // pinned, device-visible: [S] cells each stream emitted
    int n_rescued = -1;            // RT_FLAG_F64_RESCUE: streams of the enqueued call rt_fetch_f64 has analysed again (-1: not looked at yet)
    hipEvent_t ev_done = nullptr;
    LedgerCall lc;                 // as Slot::lc
};
struct F64State {
    rt_config_f64 c{};
    int N = 0, M = 0, log2m = 0, SPB = 1, K = 1, stride = 1, max_seg = 0;
    bool blu = false;
    double *d_window = nullptr;
    cd *d_cwin = nullptr, *d_bfilt = nullptr, *d_tw = nullptr;
    double *d_map = nullptr;
    double *d_tail[kTails] = {nullptr, nullptr, nullptr};
    double *d_thr_s = nullptr, *d_cal_s = nullptr;
    std::vector<double> h_thr_s;
    StreamSettings64 *d_set_s = nullptr;  // [S] rt_set_stream_settings_f64, or null: rt_config's for every stream
    std::vector<StreamSettings64> h_set_s;
    int rec_cap = 1024;
    uint64_t n_calls = 0;
    F64Slot slot[kSlots];
    int rm_slot = -1;  // the slot of the call rt_fetch_f64 delivered last, while its row means are valid (kRowMeansNone / kRowMeansExtract)
    bool cells_full = false;  // ... and that call was delivered in full (rt_fetch_record_cells_f64)
    int64_t cells_want = 0;   // cells every slot's pool should hold: the largest size any call has needed so far
    // RT_FLAG_F64_SPARSE: no d_map; the scan's chunk geometry, the partial row sums (rewritten by every call) and the folded sums
    bool sparse = false;
    int group = 1, chunk = 1, chunk_cap = 0, hot_cap = 0, sort_cap = 0;
    double *d_partial = nullptr;   // [S][chunk_cap][N]
    double *d_row_sums = nullptr;  // [S][N]
    // RT_FLAG_F64_RESCUE: the scratch of rt_fetch_f64's re-analysis (rt_f64_rescue.h), allocated at first need and kept
    bool rescue = false;
    bool rs_attr = false;          // the map scans' dynamic LDS limit is set
    double *d_rs_map = nullptr;    // [per_round][T][N]
    double *d_rs_partial = nullptr;  // [per_round][n_chunks][N]
    size_t rs_map_bytes = 0, rs_partial_bytes = 0;
    int32_t *d_rs_list = nullptr;  // [S] the call's overflowing streams
};

// rt_set_record_iq (rt_record_iq_book.h, rt_record_iq.h): nothing of it exists until the entry is called with a margin >= 0.
// One per lane-less handle, float32 or float64; a laned handle's lanes each own theirs.
constexpr int kIqNone = -1, kIqExtract = -2, kIqTruncated = -3, kIqOff = -4;  // RecordIq::delivered without a slot
constexpr size_t kInitialIqPoolBytes = 1u << 20;  // a slot's byte pool at first need; a call that wants more grows it inside rt_fetch
// What an entry of the rt_fetch_record_* family leaves in a slot for its delivered call: an output pool, the work list its kernel
// ran from, and the (hop_div, half_width) key the output was built for.  Nothing of a product is allocated, uploaded or launched
// unless its entry is called (the estimates entry also makes the hop product, the spectrum entry the band product).
struct IqProduct {
    int k = 0, w = 0;       // `out` holds the delivered call's output for (k, w); k 0: it holds nothing
    char *out = nullptr;
    size_t out_bytes = 0;
    char *work = nullptr;
    size_t work_bytes = 0;
    bool holds(int k_, int w_) const { return k != 0 && k == k_ && w == w_; }
    void set(int k_, int w_) { k = k_, w = w_; }
};
// out / work of each product (cf: cd on a float64 handle):
//   kProdStft  rt_fetch_record_stft, key (1, 0): [offsets.back() / N] cf / StftWork: seg_first, fi
//   kProdHop   rt_fetch_record_stft_hop, key (k, 0): [frames] cf / StftHopWork: frame_first, pool_seg, lp, fi
//   kProdBand  rt_fetch_record_band: [frames][2 w + 1] cf / StftHopWork, as the hop product's
//   kProdEst   rt_fetch_record_estimates, key (k, 0): [records] rt_record_estimate / the turn-back table, then EstimatesWork
//   kProdSpec  rt_fetch_record_spectrum: [records] rt_record_spectrum, then mean and peak [records][2 w + 1] float64 /
//              EstimatesWork: frame_first, range, lp
enum { kProdStft, kProdHop, kProdBand, kProdEst, kProdSpec, kProducts };
struct IqSlot {
    int32_t *h_rows = nullptr, *d_rows = nullptr;    // [S] IqCall::write_buf, pinned / device (iq_tails reads it)
    char *d_pool = nullptr;                          // the snippets of the slot's delivered call, in record order
    size_t pool_bytes = 0;
    char *h_descs = nullptr, *d_descs = nullptr;     // the copy list and its tile prefix, pinned / device
    size_t desc_bytes = 0;
    std::vector<int64_t> offsets;                    // [records + 1] of the delivered call, in samples
    std::vector<int32_t> first_seg;                  // [records]
    int bps = 0;                                     // bytes per sample of the delivered call
    int state = RT_OK;                               // what the gather left: RT_OK, RT_E_NOMEM, RT_E_HIP
    std::string why;
    // the rt_fetch_record_* family: what the gather notes for it, and what each entry's first call for this delivered call leaves
    std::vector<int32_t> fi;                         // [records] the records' bins
    std::vector<int32_t> start, end;                 // [records] the records' cells
    int fmt = kFmtC64;                               // the delivered call's input format (bps does not tell uint8 from int8)
    IqProduct prod[kProducts];
};
struct RecordIq {
    char *d_tails = nullptr;   // [kIqRows][S][row_bytes]
    int64_t row_bytes = 0;     // (K + m) * N * area_bps, rounded up to 16
    int area_bps = 0;          // bytes per sample of the widest format seen so far
    hipStream_t s_gather = nullptr;  // the gather's own stream: a fetch must not queue behind the next call's scan
    IqSlot slot[kSlots];
    int delivered = kIqNone;   // the slot whose snippets rt_fetch_record_iq hands out, or kIq*
    void *d_stft_tw = nullptr;   // [N] cf / cd: record_stft's twiddles, made by the first rt_fetch_record_stft
    float *d_stft_win = nullptr; // [N] float32 handle: the window as the caller gave it (a float64 handle's is F64State::d_window)
};

// rt_set_input_stats (rt_input_stats.h): nothing of it exists until the entry turns the feature on.  One per lane-less handle,
// float32 or float64; a laned handle's lanes each own theirs.  A call slot's partial rows, its pinned rows, and the number of the
// call whose rows they are (0: none -- the slot's call was enqueued with the feature off, or failed to enqueue).
struct InputStatsSlot {
    void *d_parts = nullptr;            // [S][max_chunks] InputStatsPart
    rt_input_stats *h_rows = nullptr;   // [S] pinned, device-visible: input_stats_fold writes them
    uint64_t seq = 0;
};
struct InputStatsState {
    bool on = false;
    int max_chunks = 0;  // chunks of rt_config.max_samples
    InputStatsSlot slot[kSlots];
};

}  // namespace

struct rt_handle {
    rt_config cfg{};
    int R3 = 1, N = 256, LG = 16, GPW = 16;
    bool wcos = false;     // ... its window is a cosine sum of order <= 1: computed in the kernel from lin_c[0] + lin_c[1] cos(2 pi n / N) (stft_wg: WCOS)
    int big = 0;           // nperseg 8192 / 16 384: threads of the one-workgroup-per-segment scan (256 / 512; rt_scan_wg.h: stft_wg), else 0
    int QS = 0;            // nperseg 128 / 64 / 32: lanes of a lane group (8 / 4 / 2; R3 = 1 there), else 0 (rt_kernels.h: stft_scan<.., QS>)
    int K = 1;             // tail columns
    int stride = 1;        // probe stride
    int L = 32;            // segments per chunk
    int max_seg = 0;       // T for max_samples
    std::vector<float> h_thr_s;  // host copy of the per-stream thresholds (empty: rt_config's for every stream)
    int max_chunks = 0;
    bool two_level = false;  // stft_scan64 without the chunk-bit pre-filter: a stream's earliest chunks are half as long (rt_kernels.h: chunk_geometry)
    int max_blocks = 0;  // workgroups per stream at max_chunks
    hipStream_t s_scan = nullptr;
    bool own_scan_stream = false;
    hipStream_t s_detect = nullptr;  // the sparse detection's own (lower-priority) stream where the handle owns its streams, else = s_scan
    std::string err;

    bool general = false;      // nperseg is not one the fused scans cover: stft_general / stft_bluestein + detect_dense (rt_general.h), dense path only
    int log2n = 8;             // log2 of the LDS transform's length: nperseg (a power of two), or Bluestein's M
    cf *d_twg = nullptr;       // ... its twiddles W_M^j, j < M / 2
    bool bluestein = false;    // nperseg is not a power of two: Bluestein's algorithm with transforms of length gen_m >= 2 nperseg - 1
    int gen_m = 0;
    cf *d_cwin = nullptr;      // [nperseg] window * sqrt(scale) * exp(-i pi n^2 / nperseg)
    cf *d_bfilt = nullptr;     // [gen_m] transform of the chirp filter, divided by gen_m
    int n_cu = 256;            // compute units of the device (the scan's grid: launch_stft_lin)
    uint32_t *d_work = nullptr;  // the scan kernels' item counters (StftParams::work), zero between launches
    float *d_window = nullptr;
    float *d_window_t = nullptr;  // nperseg 4096: the window in lane order (StftParams::window_t)
    cf *d_tw1 = nullptr, *d_tw2 = nullptr;
    float *d_tail[kTails] = {nullptr, nullptr, nullptr};
    float *d_spec = nullptr;                   // lazily allocated dense spectrogram (shared)
    float *d_spec_part = nullptr;              // ... and one for min(S, kMaxPartial) streams (partial dense re-run)
    void *d_iq_stage[kSlots] = {nullptr, nullptr};  // for rt_process_host: one per call slot (a call's IQ must stay
    size_t iq_stage_bytes[kSlots] = {0, 0};         // in place until it is fetched -- AUTO mode may re-run it dense)
    int64_t pool_want = 0;  // records every slot's pool should hold: the largest size any call has needed so far
    int64_t pool_max = 0;   // ... and the most any call can deliver: (n_streams + partial re-runs) * record_capacity
    Slot slot[kSlots];

    int hot_cap = 8192, rec_cap = 1024, cand_cap = 32;
    bool group_detect = false;  // sparse detection of a whole stream by one wave (detect_group) is possible and wanted: many streams per launch ...
    bool group_light = true;    // ... and the streams of the call fetched last held few candidate cells on average (fetch_one); a call's launch looks at this
    bool group_forced = false;  // RT_FLAG_GROUP_DETECT: whatever the streams hold
    size_t lds_large = 0, lds_small = 0, lds_dense = 0;

    bool lin = false;      // constant detrend by linearity (cosine-sum window of order <= 1; rt_kernels.h: LIN)
    // ... except for the streams its guard has marked (StftParams::dc_flag / sub_first): per stream, for good (an SDR's offset is a
    // property of its hardware), so that a stream's results never depend on which other streams share its batch
    int32_t *d_sub_first = nullptr;        // [S] non-zero = marked
    std::vector<int32_t> h_sub_first;      // host copy
    int32_t *h_sub_list = nullptr;         // pinned, device-visible: the marked streams, ascending (n_sub of them)
    int n_sub = 0;
    uint64_t sub_epoch = 0;                // changes of the set so far (a call analysed under an older one is analysed again)
    float lin_c[3] = {0.f, 0.f, 0.f};

    AutoPolicy ap;              // RT_MODE_AUTO's level, probe counters and the levels that exist at this geometry (rt_core.h; `lv`: any mode)
    int minsum_slot = -1;       // the slot whose d_chunk_min holds the latest call's chunk minima (-1: none yet)
    int run_cells = 1;          // r: cells a plateau needs unless it runs through t = 0 (plan_runs)
    uint64_t n_calls = 0;  // calls enqueued so far
    uint64_t test_enqueues = 0;  // laned handle: rt_process calls seen (fault injection, read once at rt_create: RT_TEST_FAIL_LANE=<lane>:<n>)
    int test_fail_lane = -1, test_fail_nth = 0;
    int tail_mode = 0;     // 0: a call's planning kernels and second scan in order on s_scan; 1: on s_detect with the detection (enqueue_analysis)
    StreamLedger ledger;   // the look-back state, float32 and float64 handles alike (rt_ledger.h); a laned handle: its lanes hold theirs
    LedgerCall lc_saved;   // the snapshot of the call a new one displaced from its slot, while that call may still be put back (claim_slot)
    float *d_thr_s = nullptr, *d_cal_s = nullptr;  // [S] per-stream thresholds / calibration (rt_set_stream_params)
    // [S] per-stream snr_threshold, duration gates and probe stride (rt_set_stream_settings), or null: rt_config's for every stream.
    // K, prefilter_ok and run_cells stay derived from rt_config's durations, the envelope of every stream's.
    StreamSettings *d_set_s = nullptr;
    std::vector<StreamSettings> h_set_s;  // host copy (empty: none)

    rt_call_info info{};
    bool timing = false;

    // cfg.lanes > 1: this handle only owns `kids` (one complete handle per stream group, each with its own
    // HIP stream) and forwards every call to them; kid k analyses streams [kid_base[k], kid_base[k + 1])
    std::vector<rt_handle *> kids;
    std::vector<int> kid_base;

    // RT_FLAG_ROW_MEANS: the slot of the call rt_fetch delivered last, while its row means are valid (rt_fetch_row_means) --
    // or kRowMeansNone (none delivered, or an rt_process* / rt_extract / rt_reset since), or kRowMeansExtract
    int rm_slot = -1;
    bool cells_full = false;  // RT_FLAG_RECORD_CELLS: ... and that call was delivered in full: its cells can be fetched (rt_fetch_record_cells)
    int64_t cells_want = 0;   // cells every slot's pool should hold: the largest size any call has needed so far

    size_t chunk_min_bytes = 0;         // bytes of a slot's d_chunk_min (0: none)
    const Slot *launch_mask = nullptr;  // while a masked call's kernels are being enqueued: the slot whose mask rows its scans take (launch_stft)
    std::vector<float> h_cal_s;  // host copy of the per-stream calibration (empty: rt_config's for every stream): rt_set_chain's uniformity check

    F64State *f64 = nullptr;  // a float64 handle (rt_create_f64): nothing above but cfg, N, s_scan, err and info is used
    RecordIq *riq = nullptr;  // rt_set_record_iq (float32 and float64 handles; a laned handle: its lanes hold theirs)
    int iq_margin = -1;       // ... the margin in force, -1: off (the one thing a laned handle keeps itself)
    InputStatsState *ist = nullptr;  // rt_set_input_stats (float32 and float64 handles; a laned handle: its lanes hold theirs)
    std::vector<float> h_window;  // float32 handle: rt_config.window as given (the scans' d_window is times sqrt(scale)): rt_fetch_record_stft uploads it at first need
};

namespace {

#define RT_HIP(h, expr)                                                                       \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) {                                                               \
            (h)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                     \
            return RT_E_HIP;                                                                  \
        }                                                                                     \
    } while (0)

#ifdef RT_DIAG
// The diagnostic library reads a handful of environment switches (rt_diag.h).  A committed script that still sets one that no
// longer exists would A/B two identical configurations without a word (advisor, round 5): every RT_EXP_* / RT_TEST_* variable
// this build does not know is named on stderr, once per process.
extern "C" char **environ;
void warn_unknown_switches() {
    static bool done = false;
    if (done) return;
    done = true;
    static const char *const known[] = {"RT_EXP_ONE_LEVEL", "RT_EXP_TAIL", "RT_EXP_STREAMS", "RT_EXP_TAIL_PRIO", "RT_TEST_FAIL_LANE", "RT_STAMPS_DUMP"};
    for (char **e = environ; e && *e; ++e) {
        if (std::strncmp(*e, "RT_EXP_", 7) != 0 && std::strncmp(*e, "RT_TEST_", 8) != 0) continue;
        const char *eq = std::strchr(*e, '=');
        const std::string name(*e, eq ? (size_t)(eq - *e) : std::strlen(*e));
        bool ok = false;
        for (const char *k : known) ok = ok || name == k;
        if (!ok) std::fprintf(stderr, "librt_analyze_diag: environment variable %s is set but this build reads no such switch (known: RT_EXP_ONE_LEVEL, RT_EXP_TAIL, RT_EXP_STREAMS, RT_EXP_TAIL_PRIO, RT_TEST_FAIL_LANE, RT_STAMPS_DUMP)\n", name.c_str());
    }
}
#endif

// hipMalloc + upload, and hipMalloc + zero fill, at handle creation.  CHECK is the caller's error macro (RT_CREATE_HIP,
// RT_F64_CREATE): it sees each call as it is written here with the arguments put in, so a failure still reads
// "hipMalloc(&h->d_tw1, sizeof(cf) * ...): <hipGetErrorString>" and frees what that macro frees.
#define RT_DEVICE_COPY(CHECK, dst, src, bytes)                     \
    do {                                                           \
        CHECK(hipMalloc(&dst, bytes));                             \
        CHECK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));  \
    } while (0)
#define RT_DEVICE_ZEROS(CHECK, dst, bytes) \
    do {                                   \
        CHECK(hipMalloc(&dst, bytes));     \
        CHECK(hipMemset(dst, 0, bytes));   \
    } while (0)

int fail_create(int code, const std::string &msg) {
    g_create_error = msg;
    return code;
}

size_t rec_lds_bytes(int rec_cap) { return (size_t)std::min(rec_cap, kDenseLdsRecords) * (8 + 8 + sizeof(rt_record)) + 16; }

// The dense extractor over `grid` streams (all of them, or the list in a.stream_list).  While the handle's record capacity fits
// the kernel's LDS staging it orders, filters and publishes its records itself; beyond that (a capacity that has grown: the
// reference appends without limit, analyze.py:449-450) the list is staged in the streams' raw-record areas and finalize_records,
// the sparse path's last kernel, finishes the call.
void launch_detect_dense(rt_handle *h, int grid, hipStream_t st, const DetectArgs &a);

// `items` work items (one per stream and group of GPW chunks).  Every mode but the selective pass runs them on a grid
// that just fills the chip: CUs x the workgroups of this instantiation a CU holds (its __launch_bounds__), each
// workgroup drawing further items from p.work (rt_kernels.h: "Work items") -- more workgroups than that would only
// queue in the dispatcher and find the counter exhausted.
// the fused scans' template arguments of an input format (rt_kernels.h, scan_fmt): <.., MODE | kModeI16, false, ..> is int16 input, <.., MODE | kModeI8, false, ..> int8
#define RT_SCAN_KERNEL(R3_, QS_) (stft_scan<R3_, MODEF, FMT == kFmtU8, LIN, QS_>)
#define RT_WG_KERNEL(B_, W_) (stft_wg<B_, MODEF, FMT == kFmtU8, W_>)
template <int MODE, int FMT, bool LIN>
void launch_stft_lin(rt_handle *h, const StftParams &p, int items, hipStream_t st) {
    constexpr int MODEF = MODE | (FMT == kFmtI16 ? kModeI16 : FMT == kFmtI8 ? kModeI8 : 0);
    if (h->big) {
        // nperseg 8192 / 16 384: one workgroup per item (a chunk of one stream), a segment per step (rt_scan_wg.h)
        if constexpr (MODE <= 2) {
            if (h->big == 256) {
                if (h->wcos) hipLaunchKernelGGL(RT_WG_KERNEL(256, true), dim3(items), dim3(256), wg_lds_bytes(256), st, p);
                else hipLaunchKernelGGL(RT_WG_KERNEL(256, false), dim3(items), dim3(256), wg_lds_bytes(256), st, p);
            } else {
                if (h->wcos) hipLaunchKernelGGL(RT_WG_KERNEL(512, true), dim3(items), dim3(512), wg_lds_bytes(512), st, p);
                else hipLaunchKernelGGL(RT_WG_KERNEL(512, false), dim3(items), dim3(512), wg_lds_bytes(512), st, p);
            }
        }
        return;  // (the other modes do not exist at these sizes: rt_create refuses them)
    }
    if (scan_wave64(h->R3)) {
        // nperseg 4096: one wave per segment, items drawn per wave; one 8-wave workgroup (all of a CU's LDS) per CU
        const int wgs = std::min((items + kW64Waves - 1) / kW64Waves, h->n_cu);
        hipLaunchKernelGGL((stft_scan64<MODEF, FMT == kFmtU8, LIN>), dim3(wgs), dim3(kW64Block), 0, st, p);
        return;
    }
    const int blk = scan_block(h->R3);
    // workgroups a CU holds: three waves per SIMD by registers (four for the leaner uint8 / RT_WG4 instantiations), and at
    // nperseg 256 twelve one-wave workgroups by LDS whatever the registers allow
    const int per_cu = scan_dma(h->R3, FMT, h->QS) ? 2 : std::min(((h->R3 <= RT_WG4_MAX_R3 || (FMT == kFmtU8 && h->R3 == 1)) ? 4 : 3) * (kBlock / blk), blk == 64 ? 12 : 4);
    // (A/B on one box, whole path, profiles/r03_h_persistent_ab.txt: config 3 one lane 662 k -> 684 k MS/s, config 5 share +1 %)
    const bool persist = scan_persistent(h->R3, MODE);
    const int blocks = persist ? std::min(items, h->n_cu * per_cu) : items;
    switch (h->QS ? -h->QS : h->R3) {
        case -8: hipLaunchKernelGGL(RT_SCAN_KERNEL(1, 8), dim3(blocks), dim3(blk), 0, st, p); break;  // nperseg 128
        case -4: hipLaunchKernelGGL(RT_SCAN_KERNEL(1, 4), dim3(blocks), dim3(blk), 0, st, p); break;  // 64
        case -2: hipLaunchKernelGGL(RT_SCAN_KERNEL(1, 2), dim3(blocks), dim3(blk), 0, st, p); break;  // 32
        case 1: hipLaunchKernelGGL(RT_SCAN_KERNEL(1, 0), dim3(blocks), dim3(blk), 0, st, p); break;
        case 2: hipLaunchKernelGGL(RT_SCAN_KERNEL(2, 0), dim3(blocks), dim3(blk), 0, st, p); break;
        case 4: hipLaunchKernelGGL(RT_SCAN_KERNEL(4, 0), dim3(blocks), dim3(blk), 0, st, p); break;
        case 8: hipLaunchKernelGGL(RT_SCAN_KERNEL(8, 0), dim3(blocks), dim3(blk), 0, st, p); break;
#if !RT_WAVE64_4096
        default: hipLaunchKernelGGL(RT_SCAN_KERNEL(16, 0), dim3(blocks), dim3(blk), 0, st, p); break;
#else
        default: break;  // (nperseg 4096 is stft_scan64's, above)
#endif
    }
}
#undef RT_SCAN_KERNEL
#undef RT_WG_KERNEL

// MODE 3 (load stream only) has no detrend: one instantiation
// uint8 input keeps the subtract-first form: quantised samples make exact cancellations real (a saturated segment is
// constant, x - mean is exactly zero and so is every cell of it in the reference -> std = NaN over a plateau that holds
// one; the linearity form leaves a residue 140 dB under the offset there -- found by the round-2 soak).
// int16 input follows complex64 in this as in everything: its results are those of rt_process on the same values, bit for bit
template <int MODE, int FMT = kFmtC64>
void launch_stft(rt_handle *h, const StftParams &p, int blocks, hipStream_t st) {
    constexpr bool U8 = (FMT == kFmtU8);
    // A call with a presence mask (rt_set_present; not a launch over a list of its own): absent streams are left alone by what the
    // kernels have for that already, StftParams::stream_list: every scan runs over a list of present streams, so that neither a
    // launch nor its time grows with the absent ones -- the LIN scan over the present streams its guard has not marked, the
    // subtract-first launch behind it over the marked ones that are present, every other scan over all present streams.  A launch
    // holds no item of an absent stream, so no load and no store of any kind happens for it.  (Leaving the absent streams to
    // StftParams::sub_first in a launch over all streams was measured first: their items end at once, but only behind the
    // workgroup's tables -- profiles/present_bench_sub_first_variant.jsonl)
    const Slot *const mk = (MODE != 3 && !p.stream_list) ? h->launch_mask : nullptr;
    if (mk) {
        const int S = h->cfg.n_streams;
        const int n_present = mk->lc.pc.n_present;
        if (n_present == 0) return;
        StftParams q = p;
        if (h->lin && !U8) {
            if (mk->n_lin_present > 0) {
                q.sub_first = nullptr;
                q.stream_list = mk->d_mask + (size_t)kMaskLinList * S;
                q.n_streams = mk->n_lin_present;
                q.spec_by_stream = 1;
                launch_stft_lin<MODE, FMT, (MODE != 3 && !U8)>(h, q, q.n_streams * p.blocks_per_stream, st);
            }
            if (mk->n_sub_present == 0) return;
            q = p;
            q.stream_list = mk->d_mask + (size_t)kMaskSubList * S;
            q.n_streams = mk->n_sub_present;
        } else {
            q.stream_list = mk->d_mask + (size_t)kMaskList * S;
            q.n_streams = n_present;
        }
        q.sub_first = nullptr;
        q.dc_flag = h->lin && !U8 ? nullptr : p.dc_flag;
        q.spec_by_stream = 1;
        launch_stft_lin<MODE, FMT, false>(h, q, q.n_streams * p.blocks_per_stream, st);
        return;
    }
    if (h->lin && MODE != 3 && !U8) {
        if (p.stream_list || h->n_sub == 0 || !p.sub_first) {
            // (a launch over a list of its own -- AUTO's dense re-run of a few streams -- keeps the linearity form for all of them: its
            // dense spectrogram is indexed by position in that list, which a second launch over a sub-list cannot address)
            StftParams q = p;
            if (p.stream_list) q.sub_first = nullptr;
            launch_stft_lin<MODE, FMT, (MODE != 3 && !U8)>(h, q, blocks, st);
        } else {
            // the streams the guard of that form has marked (StftParams::dc_flag): the first launch leaves them alone, the
            // subtract-first instantiation takes them, by list
            launch_stft_lin<MODE, FMT, (MODE != 3 && !U8)>(h, p, blocks, st);
            StftParams q = p;
            q.sub_first = nullptr;
            q.dc_flag = nullptr;
            q.spec_by_stream = 1;
            q.stream_list = h->h_sub_list;
            q.n_streams = h->n_sub;
            launch_stft_lin<MODE, FMT, false>(h, q, h->n_sub * p.blocks_per_stream, st);
        }
    } else {
        launch_stft_lin<MODE, FMT, false>(h, p, blocks, st);
    }
}

// the general transform (rt_general.h): the dense spectrogram of an nperseg the fused scans do not cover (the caller runs
// row_sums_dense over the map)
void launch_general(rt_handle *h, const void *iq, int64_t stream_stride, int n_seg, float *spec, float *tail, int fmt, const int32_t *absent = nullptr) {
    if (h->bluestein) {
        BluesteinParams b{};
        b.absent = absent;
        b.iq = iq;
        b.stream_stride = stream_stride;
        b.n_streams = h->cfg.n_streams;
        b.n_seg = n_seg;
        b.nperseg = h->N;
        b.m = h->gen_m;
        b.log2m = h->log2n;
        b.tail_cols = h->K;
        b.cwin = h->d_cwin;
        b.bfilt = h->d_bfilt;
        b.tw = h->d_twg;
        b.spec = spec;
        b.tail = tail;
        const int blocks = h->cfg.n_streams * n_seg;
        const size_t lds = (size_t)h->gen_m * sizeof(cf);
        // (groups of a thread per trip of a double stage: rt_general.h, lds_fft_stages -- M / 4 a multiple of 256 U)
        // threads per workgroup and groups of a thread per trip of a double stage (rt_general.h, lds_fft_stages: M / 4 a multiple of threads x U).
        // From M = 4096 on 512 threads, at 16 384 (one workgroup per CU) 1 024: more waves to cover the LDS latency of the stages
        // where LDS leaves room for one or two workgroups per CU (16 384: 512 threads 27.4 k MS/s at nperseg 6000, 1 024 34 k).
#define RT_BLU(U_, B_)                                                                                                            \
    do {                                                                                                                          \
        if (fmt == kFmtU8) hipLaunchKernelGGL((stft_bluestein<kFmtU8, U_, B_>), dim3(blocks), dim3(B_), lds, h->s_scan, b);        \
        else if (fmt == kFmtI16) hipLaunchKernelGGL((stft_bluestein<kFmtI16, U_, B_>), dim3(blocks), dim3(B_), lds, h->s_scan, b); \
        else if (fmt == kFmtI8) hipLaunchKernelGGL((stft_bluestein<kFmtI8, U_, B_>), dim3(blocks), dim3(B_), lds, h->s_scan, b);   \
        else hipLaunchKernelGGL((stft_bluestein<kFmtC64, U_, B_>), dim3(blocks), dim3(B_), lds, h->s_scan, b);                     \
    } while (0)
        if (h->gen_m >= 16384) RT_BLU(4, 1024);
        else if (h->gen_m >= 8192) RT_BLU(4, 512);  // (8 groups x 256 threads: 31.8 k MS/s at nperseg 3000, this 41.6 k)
        else if (h->gen_m >= 4096) RT_BLU(2, 512);  // (4 x 256: 47.9 k at nperseg 1500, this 51.2 k)
        else if (h->gen_m >= 2048) RT_BLU(2, 256);  // (1 x 512: 56.7 k at nperseg 1000, this 72 k -- enough workgroups per CU as it is)
        else RT_BLU(1, 256);
#undef RT_BLU
        return;
    }
    GeneralParams g{};
    g.absent = absent;
    g.iq = iq;
    g.stream_stride = stream_stride;
    g.n_streams = h->cfg.n_streams;
    g.n_seg = n_seg;
    g.nperseg = h->N;
    g.log2n = h->log2n;
    g.segs_per_block = std::min(64, std::max(1, 1024 / h->N));  // (N / 4 four-element groups per segment and double stage: every thread has one at N <= 1024)
    g.tail_cols = h->K;
    g.window = h->d_window;
    g.tw = h->d_twg;
    g.spec = spec;
    g.tail = tail;
    const int blocks = h->cfg.n_streams * ((n_seg + g.segs_per_block - 1) / g.segs_per_block);
    const size_t lds = (size_t)g.segs_per_block * h->N * sizeof(cf);
    if (fmt == kFmtU8) hipLaunchKernelGGL((stft_general<kFmtU8>), dim3(blocks), dim3(kGeneralBlock), lds, h->s_scan, g);
    else if (fmt == kFmtI16) hipLaunchKernelGGL((stft_general<kFmtI16>), dim3(blocks), dim3(kGeneralBlock), lds, h->s_scan, g);
    else if (fmt == kFmtI8) hipLaunchKernelGGL((stft_general<kFmtI8>), dim3(blocks), dim3(kGeneralBlock), lds, h->s_scan, g);
    else hipLaunchKernelGGL((stft_general<kFmtC64>), dim3(blocks), dim3(kGeneralBlock), lds, h->s_scan, g);
}

// cells a run must have to pass the duration gate unless it runs through t = 0 (rt_core.h)
long long min_run_cells(const rt_handle *h) { return rt::min_run_cells(h->N, h->cfg.sample_rate, h->cfg.min_duration_s); }

// segments per chunk for a handle of `n_streams` streams (for a laned handle: of all lanes together -- the lanes take the
// parent's choice, so that a stream's row sums are added in the same order however the batch is split into lanes); rt_core.h
int choose_chunk(const rt_config &cfg, const ScanFamily &fam, int n_streams, int n_seg) {
    return rt::choose_chunk(cfg.nperseg, fam.R3, fam.QS, scan_block(fam.R3), cfg.sample_rate, cfg.min_duration_s, cfg.segs_per_chunk, n_streams, n_seg);
}


StftParams make_stft_params(rt_handle *h, Slot &sl, const void *iq, int64_t stream_stride, int n_seg, int tail_write) {
    StftParams p{};
    p.iq = iq;
    p.stream_stride = stream_stride;
    p.n_streams = h->cfg.n_streams;
    p.n_seg = n_seg;
    p.segs_per_chunk = h->L;
    p.chunks = (n_seg + h->L - 1) / h->L;
    if (h->two_level) {
        int n_short = 0, short_len = 0, chunks = 0;
        chunk_geometry(n_seg, h->L, true, &n_short, &short_len, &chunks);
        p.short_chunks = n_short;
        p.short_len = short_len;
        p.chunks = chunks;
    }
    p.blocks_per_stream = (p.chunks + h->GPW - 1) / h->GPW;
    p.tail_cols = h->K;
    p.work = h->d_work;
    p.window = h->d_window;
    p.window_t = h->d_window_t;
    p.tw1 = h->d_tw1;
    p.tw2 = h->d_tw2;
    p.scale = h->cfg.scale;
    p.thr = h->cfg.threshold;
    for (int i = 0; i < 3; ++i) p.lin_c[i] = h->lin_c[i];
    p.thr_s = h->d_thr_s;
    p.psum = sl.d_psum;
    p.tail = h->d_tail[tail_write];
    p.spec = h->d_spec;
    p.hot = sl.d_hot;
    p.hot_count = sl.d_hot_count;
    p.hot_cap = h->hot_cap;
    p.tbits = key_tbits(n_seg);
    p.full = sl.d_full;
    p.first = sl.d_full ? sl.d_full + (size_t)h->cfg.n_streams * h->max_chunks * h->LG : nullptr;
    p.item_chunks = sl.d_items;
    p.item_count = sl.d_items ? sl.d_items + (size_t)h->cfg.n_streams * h->max_blocks * h->GPW : nullptr;
    p.chunk_min = nullptr;  // (only the exact pre-filter's own scans keep chunk minima: enqueue_analysis)
    p.abs_hot = nullptr;
    p.thr_bin = nullptr;
    p.cell_hot = sl.d_cell_hot;
    p.cell_need = sl.d_cell_need;
    p.seg_list = sl.d_seg_list;
    p.seg_count = sl.d_seg_list ? sl.d_seg_list + (size_t)h->cfg.n_streams * h->max_seg : nullptr;
    p.dc_flag = h->lin ? sl.h_dc_flag : nullptr;
    p.sub_first = h->lin ? h->d_sub_first : nullptr;
    p.dc_limit = 1.0e6f * (float)h->N * (float)h->N * (float)h->cfg.sample_rate;  // 60 dB over the quietest bin's per-sample power
    p.dc_limit2 = 100.0f * (float)h->N * (float)h->cfg.sample_rate;               // ... and 20 dB over everything else in those segments
    return p;
}

DetectArgs make_detect_args(rt_handle *h, Slot &sl, int n_seg, int n_bins, int n_seg_last) {
    DetectArgs a{};
    a.dp.n_seg = n_seg;
    a.dp.n_seg_last = n_seg_last;
    a.dp.tail_cols = h->K;
    a.dp.stride = h->stride;
    a.dp.nperseg = h->N;
    a.dp.thr = h->cfg.threshold;
    a.dp.snr = h->cfg.snr_threshold;
    a.dp.cal_db = h->cfg.calibration_db;
    a.dp.fs = h->cfg.sample_rate;
    a.dp.min_d = h->cfg.min_duration_s;
    a.dp.max_d = h->cfg.max_duration_s;
    a.n_streams = h->cfg.n_streams;
    a.n_bins = n_bins;
    a.hot = sl.d_hot;
    a.hot_count = sl.d_hot_count;
    a.hot_count_rw = sl.d_hot_count;
    a.large_any = sl.d_hot_seen;  // (one word per stream of the array's S * 16; behind them detect_group's work list, then its counter)
    if (h->group_detect && (h->group_forced || h->group_light)) {
        a.work_list = reinterpret_cast<int32_t *>(sl.d_hot_seen) + h->cfg.n_streams;
        a.work_count = a.work_list + (size_t)h->cfg.n_streams * kQuarters;
    }
    a.hot_total = sl.h_hot_total;
    a.lds_cells = next_pow2(std::max(h->hot_cap, 64));
    a.cand_cap = h->cand_cap;
    a.hot_cap = h->hot_cap;
    a.tbits = key_tbits(n_seg);
    a.raw = sl.d_raw;
    a.raw_count = sl.d_raw_count;
    a.psum = sl.d_psum;
    a.records = sl.h_records;
    a.pool_cap = sl.pool_cap;
    a.rec_cap = h->rec_cap;
    a.rec_offset = sl.h_rec_offset;
    a.rec_count = sl.h_rec_count;
    a.counters = sl.d_counters;
    a.host_counters = sl.h_counters;
    a.thr_s = h->d_thr_s;
    a.cal_s = h->d_cal_s;
    a.set_s = h->d_set_s;
    a.no_last = sl.lc.took.empty() ? nullptr : sl.h_no_last;
    if (sl.lc.masked) {  // rt_set_present: each stream's own previous segment count (a reset taken: -1), and who sits the call out
        a.absent = sl.d_mask + (size_t)kMaskAbsent * h->cfg.n_streams;
        a.n_seg_last_s = sl.d_mask + (size_t)kMaskNSegLast * h->cfg.n_streams;
    }
    a.stream_overflow = sl.h_overflow;
    a.stream_incons = sl.h_incons;
    return a;
}

void launch_detect_dense(rt_handle *h, int grid, hipStream_t st, const DetectArgs &a) {
    if (h->rec_cap <= kDenseLdsRecords) {
        hipLaunchKernelGGL(detect_dense<false>, dim3(grid), dim3(kDetBlock), h->lds_dense, st, a);
    } else {
        hipLaunchKernelGGL(detect_dense<true>, dim3(grid), dim3(kDetBlock), 0, st, a);
        hipLaunchKernelGGL(finalize_records, dim3(grid), dim3(256), 0, st, a);
    }
}

// RT_FLAG_ROW_MEANS: every row's mean of the call (row_means_from_partials) into the slot's device buffer, on the stream of the
// call's ev_done behind its detection, which read the same partial sums: behind the last writer of d_psum on every level -- the
// first scan (MODE 0 / 1 / 4 / 6, and the subtract-first launch over the streams the detrend guard marked), row_sums_dense on the
// general path, the dense scan of a partial re-run; the selective second scans of the pre-filter levels (MODE 5 / 7) write none.
// Every analysis of a call rewrites all S rows, so the buffer holds those of the analysis whose records are delivered.
int enqueue_row_means(rt_handle *h, Slot &sl, int chunks, int n_seg, hipStream_t st) {
    if (!sl.d_row_means) return RT_OK;
    const int64_t cells = (int64_t)h->cfg.n_streams * h->N;
    hipLaunchKernelGGL(row_means_from_partials, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, sl.d_psum, chunks, h->cfg.n_streams, h->N,
                       n_seg, sl.d_row_means, sl.lc.masked ? sl.d_mask + (size_t)kMaskAbsent * h->cfg.n_streams : nullptr);
    RT_HIP(h, hipGetLastError());
    return RT_OK;
}

// ---- rt_set_chain: the look-back a call's detection (and its cell gather) reads, and the copy that fills it ----
// The slot's chained columns if the call is chained, else the rotation buffer the call reads.
const float *call_prev(rt_handle *h, const Slot &sl) { return sl.lc.chained ? sl.d_chain : h->d_tail[sl.call.tail_read]; }

// chain_tails for the call of `sl` on `st`: behind the scans of this analysis (they write the rotation buffer the copy reads for
// every stream that follows one of the same call), in front of its detection.  Every analysis of the call runs it again: a
// level-up or a subtract-first re-run rewrites the columns, some with other bits.  Nothing for a call that is not chained.
int enqueue_chain(rt_handle *h, Slot &sl, hipStream_t st) {
    const CallCtx &c = sl.call;
    const int64_t per = (int64_t)h->K * h->N;
    if (!sl.lc.chained || per <= 0) return RT_OK;
    const int S = h->cfg.n_streams, bps = chain_blocks<float>(per);
    hipLaunchKernelGGL((chain_tails<float>), dim3((unsigned)((int64_t)S * bps)), dim3(kChainBlock), 0, st, sl.d_chain_rows, sl.d_chain_rows + S, S, bps,
                       h->d_tail[c.tail_write], h->d_tail[c.tail_read], sl.d_chain, per);
    RT_HIP(h, hipGetLastError());
    return RT_OK;
}

// RT_FLAG_RECORD_CELLS: the cells of the call's final records (rt_cells.h) into the slot's pool -- where enqueue_row_means is
// called, on the same stream behind the call's detection: the dense map is one per handle and belongs to the next call as soon
// as this one's kernels are through, so the gather is never left to fetch time.  `spec`: the dense map the detection read
// (`stream_list` / `n_list`: the streams a partial re-run's map holds, the others keep their candidate lists), or null on the
// sparse levels.  Every analysis of a call gathers all its records again, so the pool follows the analysis that is delivered.
template <class P, class Rec>
void launch_record_cells(const CellsArgs<P, Rec> &a, hipStream_t st) {
    hipLaunchKernelGGL((cells_stream_totals<P, Rec>), dim3(a.n_streams), dim3(256), 0, st, a);
    hipLaunchKernelGGL(cells_stream_bases, dim3(1), dim3(kCellsScanBlock), 0, st, a.stream_cells, a.stream_base, a.n_streams, a.info);
    hipLaunchKernelGGL((cells_gather<P, Rec>), dim3(a.n_streams), dim3(256), 0, st, a);
}

int enqueue_record_cells(rt_handle *h, Slot &sl, const float *spec, const int32_t *stream_list, int n_list, hipStream_t st) {
    if (!sl.d_cells) return RT_OK;
    const CallCtx &c = sl.call;
    CellsArgs<float, rt_record> a{};
    a.records = sl.h_records;
    a.rec_off = sl.h_rec_offset;
    a.rec_cnt = sl.h_rec_count;
    a.stage = sl.d_raw;
    a.rec_cap = h->rec_cap;
    a.n_streams = h->cfg.n_streams;
    a.n_bins = h->N;
    a.n_seg = c.n_seg;
    a.spec = spec;
    a.stream_list = stream_list;
    a.n_list = n_list;
    a.prev = call_prev(h, sl);
    a.prev_cols = h->K;
    a.hot = sl.d_hot;
    a.hot_count = sl.d_hot_kept;
    a.hot_cap = h->hot_cap;
    a.tbits = key_tbits(c.n_seg);
    a.stream_cells = sl.d_stream_cells;
    a.stream_base = sl.d_stream_base;
    a.cells = sl.d_cells;
    a.cell_cap = sl.cell_cap;
    a.info = sl.h_cells_info;
    launch_record_cells(a, st);
    RT_HIP(h, hipGetLastError());
    return RT_OK;
}

// A call's records hold more cells than the slot's pool: a larger one (nothing to keep: the call is analysed again).  Only
// while none of the slot's kernels is in flight.  Failure leaves the old pool in place.
template <class P>
int grow_cells(rt_handle *h, P *&pool, int64_t &cap, int64_t want) {
    if (want <= cap) return RT_OK;
    P *p = nullptr;
    int64_t n = want + want / 4;
    hipError_t e = hipMalloc(&p, (size_t)n * sizeof(P));
    if (e != hipSuccess) {
        n = want;
        e = hipMalloc(&p, (size_t)n * sizeof(P));
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        h->err = "cell pool of " + std::to_string(n) + " cells: " + hipGetErrorString(e);
        return RT_E_NOMEM;
    }
    (void)hipFree(pool);
    pool = p;
    cap = n;
    return RT_OK;
}

int ensure_dense_spec(rt_handle *h) {
    if (h->d_spec) return RT_OK;
    const size_t bytes = (size_t)h->cfg.n_streams * (size_t)h->max_seg * (size_t)h->N * sizeof(float);
    hipError_t e = hipMalloc(&h->d_spec, bytes ? bytes : 4);
    if (e != hipSuccess) {
        h->err = "dense spectrogram scratch (" + std::to_string(bytes) + " bytes): " + hipGetErrorString(e);
        h->d_spec = nullptr;
        return RT_E_NOMEM;
    }
    return RT_OK;
}

// calls without a detect kernel (empty spectrogram): counter words -> pinned host memory by a copy
int enqueue_readback(rt_handle *h, Slot &sl, hipStream_t st) {
    RT_HIP(h, hipMemcpyAsync(sl.h_counters, sl.d_counters, kCounterWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    return RT_OK;
}

// (AUTO's levels and its policy: rt_core.h)
static_assert(kAutoAuto == RT_MODE_AUTO && kAutoDense == RT_MODE_DENSE && kAutoSparse == RT_MODE_SPARSE && kAutoPrefilter == RT_MODE_PREFILTER &&
                  kAutoRunfilter == RT_MODE_RUNFILTER,
              "rt_core.h mirrors rt_mode");

// (`st`: the handle's scan stream, or -- the selective second scans of the pre-filter levels -- the stream of what follows a call's first scan)
template <int MODE>
void launch_scan(rt_handle *h, const StftParams &sp, int blocks, int fmt, hipStream_t st = nullptr) {
    if (!st) st = h->s_scan;
    if (fmt == kFmtU8) launch_stft<MODE, kFmtU8>(h, sp, blocks, st);
    else if (fmt == kFmtI16) launch_stft<MODE, kFmtI16>(h, sp, blocks, st);
    else if (fmt == kFmtI8) launch_stft<MODE, kFmtI8>(h, sp, blocks, st);
    else launch_stft<MODE>(h, sp, blocks, st);
}

// ---- rt_set_present: a call's mask rows and the carry of the absent streams' look-back columns ----
// The scans enqueued while one of these is alive take the slot's mask (launch_stft)
struct MaskedLaunches {
    rt_handle *h;
    MaskedLaunches(rt_handle *h_, const Slot &sl) : h(h_) { h->launch_mask = sl.lc.masked ? &sl : nullptr; }
    ~MaskedLaunches() { h->launch_mask = nullptr; }
};

// the rows of kMask* from a call's snapshot; `sub_first` (or null): the streams the detrend guard has marked.  Returns the entries
// of the rows kMaskLinList / kMaskSubList / kMaskAbsentList.
void fill_mask_rows(const PresenceCall &pc, int S, const int32_t *sub_first, int32_t *rows, int *n_lin_present, int *n_sub_present, int *n_absent) {
    int n_list = 0, n_lin = 0, n_sub = 0, n_abs = 0;
    for (int s = 0; s < S; ++s) {
        const bool gone = pc.absent[(size_t)s] != 0, marked = sub_first && sub_first[s] != 0;
        rows[(size_t)kMaskAbsent * S + s] = gone ? 1 : 0;
        rows[(size_t)kMaskNSegLast * S + s] = pc.n_seg_last[(size_t)s];
        if (gone) rows[(size_t)kMaskAbsentList * S + n_abs++] = s;
        else rows[(size_t)kMaskList * S + n_list++] = s;
        if (!gone && marked) rows[(size_t)kMaskSubList * S + n_sub++] = s;
        if (!gone && !marked) rows[(size_t)kMaskLinList * S + n_lin++] = s;
    }
    *n_lin_present = n_lin;
    *n_sub_present = n_sub;
    *n_absent = n_abs;
}

// (again when the detrend guard's set has changed: fetch_one).  Nothing of the slot is in flight: the pinned rows may be rewritten.
int upload_mask(rt_handle *h, Slot &sl) {
    const int S = h->cfg.n_streams;
    fill_mask_rows(sl.lc.pc, S, h->lin ? h->h_sub_first.data() : nullptr, sl.h_mask, &sl.n_lin_present, &sl.n_sub_present, &sl.n_absent);
    RT_HIP(h, hipMemcpyAsync(sl.d_mask, sl.h_mask, (size_t)kMaskRows * S * sizeof(int32_t), hipMemcpyHostToDevice, h->s_scan));
    return RT_OK;
}

// rt_set_chain: the call's source rows to the device (once per call: a re-analysis reads them again).  As upload_mask.
int upload_chain_rows(rt_handle *h, Slot &sl) {
    const size_t S = (size_t)h->cfg.n_streams;
    std::memcpy(sl.h_chain_rows, sl.lc.cc.src_buf.data(), S * sizeof(int32_t));
    std::memcpy(sl.h_chain_rows + S, sl.lc.cc.src_idx.data(), S * sizeof(int32_t));
    RT_HIP(h, hipMemcpyAsync(sl.d_chain_rows, sl.h_chain_rows, 2 * S * sizeof(int32_t), hipMemcpyHostToDevice, h->s_scan));
    return RT_OK;
}

// The absent streams' K look-back columns from the rotation buffer the call reads to the one it writes, on the scan's stream, where
// the scan's own tail stores are (rt_present.h).  Once per call: a re-analysis finds them in place.
template <class P>
int enqueue_carry(rt_handle *h, const int32_t *d_absent_list, int n_absent, const P *src, P *dst, int K, int N) {
    const int64_t per = (int64_t)K * N;  // (K >= 1: rt_core.h tail_cols; N >= 8: rt_create)
    if (n_absent == 0 || per <= 0) return RT_OK;
    const int bps = carry_blocks(per);
    hipLaunchKernelGGL((carry_tails<P>), dim3((unsigned)((int64_t)n_absent * bps)), dim3(kCarryBlock), 0, h->s_scan, d_absent_list, n_absent, bps, src, dst, per);
    RT_HIP(h, hipGetLastError());
    return RT_OK;
}

// enqueue scan + detect + readback for the call described by sl.call, analysed the way `mode` says.
// `second_pass_only`: RT_MODE_PREFILTER for a call whose RT_MODE_SPARSE attempt has just overflowed -- that scan
// wrote the chunk bits, row sums and tail columns already, only the selective pass and the detection are repeated.
// `own_means`: RT_MODE_RUNFILTER for a call whose per-bin thresholds have just failed their check -- the thresholds of
// the re-run come from the row means the failed scan left (make_bin_thresholds_from_means).
int enqueue_analysis(rt_handle *h, Slot &sl, int mode, bool *launched = nullptr, bool second_pass_only = false, bool own_means = false) {
    sl.call.rec_cap_used = h->rec_cap;
    const CallCtx &c = sl.call;
    // A call whose thresholds failed their check once keeps the thresholds from its own row means through every further re-run
    // (record or pool growth, the detrend guard): taken from its own chunk minima again they fail the same check again, and
    // that re-run is granted once per call -- a pinned RT_MODE_RUNFILTER handle then refused the call (a NaN column: every row
    // mean NaN, so every positive threshold fails; thousands of NaN records: the record room grows behind the re-run).
    if (mode == RT_MODE_RUNFILTER && c.thr_rerun && !second_pass_only) own_means = true;
    if (launched) *launched = false;
    const MaskedLaunches masked_launches(h, sl);
    const int32_t *const absent = sl.lc.masked ? sl.d_mask + (size_t)kMaskAbsent * h->cfg.n_streams : nullptr;
    if (h->general) {
        // any other power-of-two nperseg: the general transform into the dense map, then the dense extractor (which sums the rows itself)
        int rc = ensure_dense_spec(h);
        if (rc != RT_OK) return rc;
        RT_HIP(h, hipEventRecord(sl.ev_begin, h->s_scan));
        if (launched) *launched = true;
        launch_general(h, c.iq, c.stream_stride, c.n_seg, h->d_spec, h->d_tail[c.tail_write], c.fmt, absent);
        {
            const int64_t cells = (int64_t)h->cfg.n_streams * h->N;
            hipLaunchKernelGGL(row_sums_dense, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, h->s_scan, h->d_spec, sl.d_psum, h->cfg.n_streams, c.n_seg, h->N);
        }
        RT_HIP(h, hipGetLastError());
        { const int rc2 = enqueue_chain(h, sl, h->s_scan); if (rc2 != RT_OK) return rc2; }
        RT_HIP(h, hipEventRecord(sl.ev_scan, h->s_scan));
        DetectArgs a = make_detect_args(h, sl, c.n_seg, h->N, c.n_seg_last);
        a.prev = call_prev(h, sl);
        a.prev_cols = h->K;
        a.spec = h->d_spec;
        a.psum = sl.d_psum;  // one partial row per stream (row_sums_dense)
        a.chunks = 1;
        launch_detect_dense(h, h->cfg.n_streams, h->s_scan, a);
        RT_HIP(h, hipGetLastError());
        { const int rc2 = enqueue_row_means(h, sl, 1, c.n_seg, h->s_scan); if (rc2 != RT_OK) return rc2; }
        { const int rc2 = enqueue_record_cells(h, sl, h->d_spec, nullptr, 0, h->s_scan); if (rc2 != RT_OK) return rc2; }
        RT_HIP(h, hipEventRecord(sl.ev_done, h->s_scan));
        return RT_OK;
    }
    StftParams sp = make_stft_params(h, sl, c.iq, c.stream_stride, c.n_seg, c.tail_write);
    if (sp.chunks > h->max_chunks) {
        h->err = "internal: chunk count exceeds scratch";
        return RT_E_INVALID;
    }
    const int blocks = h->cfg.n_streams * sp.blocks_per_stream;
    const int S = h->cfg.n_streams;
    const bool dense = (mode == RT_MODE_DENSE);
    // hot_count / raw_count and the four counter words are left zero by their last readers
    // (detect_bucket<true>, finalize_records / detect_dense: close_call)
    if (dense) {
        int rc = ensure_dense_spec(h);
        if (rc != RT_OK) return rc;
        sp.spec = h->d_spec;
    }
    if ((mode == RT_MODE_PREFILTER && !sl.d_full) || (mode == RT_MODE_RUNFILTER && !sl.d_cell_hot)) {
        h->err = "internal: pre-filter without its scratch";
        return RT_E_INVALID;
    }
    if (!second_pass_only) RT_HIP(h, hipEventRecord(sl.ev_begin, h->s_scan));
    if (launched) *launched = true;
    sl.call.ran_lin = h->lin && c.fmt != kFmtU8;
    sl.call.sub_epoch = h->sub_epoch;
    const int slot_index = (int)(&sl - h->slot);
    if (mode == RT_MODE_RUNFILTER) {
        // per-bin thresholds from the latest chunk minima (the previous call's; on a re-run this call's own), before they are reset
        const int64_t cells = (int64_t)S * h->N;
        if (own_means) {
            hipLaunchKernelGGL(make_bin_thresholds_from_means, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, h->s_scan, sl.d_psum, sp.blocks_per_stream,
                               c.n_seg, sl.d_thr_bin, sl.d_thr_nat, S, h->R3, h->LG, h->cfg.snr_threshold, h->d_set_s);
        } else {
        // Chunk minima are kept by this level's own scans only (round 5: the sparse scans of an AUTO handle paid for them in every
        // item's epilogue -- config 3 +1.8 % per launch -- for the one call in thousands that climbs here).  None on hand -- the handle's
        // first call on this level, or the first after calls on other levels (the minima must be the previous call's): a scan of this
        // buffer provides them (its bits, taken with the absolute threshold alone, are overwritten by the scan proper below).
        // "On hand" means: of the buffer immediately before this one (or of this very buffer: a call analysed again on this level).  An
        // AUTO handle that comes back here after thousands of sparse calls would otherwise build its thresholds from the minima of an
        // arbitrarily old buffer -- too high (a stale-threshold re-analysis and a host sync) or too low (an unselective filter, which
        // pushes AUTO on to the dense path for sticky_len calls): advisor, round 5.
        sp.chunk_min = sl.d_chunk_min;
        int src = h->minsum_slot;
        const bool on_hand = src >= 0 && h->slot[src].min_items > 0 && (h->slot[src].min_seq + 1 == c.seq || h->slot[src].min_seq == c.seq);
        if (!on_hand) {
            launch_scan<6>(h, sp, blocks, c.fmt);
            sl.min_items = sp.blocks_per_stream;
            sl.min_seq = sl.call.seq;
            src = slot_index;
            // (the LATEST buffer's minima set the next call's thresholds: a call analysed again from rt_fetch keeps that place for a later one)
            if (h->minsum_slot < 0 || sl.min_seq >= h->slot[h->minsum_slot].min_seq) h->minsum_slot = slot_index;
        }
        const Slot &ps = h->slot[src];
        hipLaunchKernelGGL(make_bin_thresholds, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, h->s_scan, ps.d_chunk_min, ps.min_items, sl.d_thr_bin,
                           sl.d_thr_nat, S, h->R3, h->LG, h->L * minsum_group(h->L, std::min(h->GPW, 16)), h->cfg.snr_threshold, h->d_set_s);
        }
    }
    if (mode == RT_MODE_RUNFILTER && !second_pass_only) {
        sp.chunk_min = sl.d_chunk_min;
        sl.min_items = sp.blocks_per_stream;  // (every item of the scan below writes its row of minima: nothing to reset)
        sl.min_seq = sl.call.seq;
        // the LATEST buffer's minima set the next call's thresholds: a call analysed again from rt_fetch (level-up, stale
        // thresholds, pool growth, the detrend guard) while a later one is in flight must not take that place back
        if (h->minsum_slot < 0 || sl.min_seq >= h->slot[h->minsum_slot].min_seq) h->minsum_slot = slot_index;
    }
    // `sd`: the stream of the call's detection (and, experimentally, of more of what follows its first scan).  Where the handle has
    // a second stream (rt_create: nperseg <= 512 without lanes) the first scan of the NEXT call, ready at the same moment on s_scan,
    // takes the chip while this call's detection runs beside it (config 2 one lane 0.79 -> 0.73 ms per step, profiles/r04_e_*).
    // What comes BETWEEN a call's two scans on the pre-filter levels -- planning kernels, the selective second scan -- stays in
    // order on s_scan (tail_mode 0): moved to `sd` as well (tail_mode 1, a diagnostic build's RT_EXP_TAIL=C) the second scan is
    // dispatched behind the next call's chip-filling first scan and gets no workgroup slot until that scan has handed out its last
    // workgroup -- it ends with it, 1.9 ms instead of 0.23, the detection behind it is exposed, rt_fetch returns a scan late and
    // the host enqueues late: 2.33 - 2.49 ms per step against 2.26 - 2.45 in order at the reference's default geometry, whatever
    // the stream's priority (profiles/r05_b_tail_on_second_stream.txt).  Safe by the slots: everything the tail reads or writes is
    // its call's slot's (per-bin thresholds included), the look-back tail it reads is two rotations from the one the next scan
    // writes, and a scan that reuses the slot waits for ev_done (claim_slot).  The dense path stays in order on the scan's stream:
    // its spectrogram is one per handle.
    hipStream_t sd = dense ? h->s_scan : h->s_detect;
    hipStream_t s2 = (h->tail_mode >= 1 && !dense) ? sd : h->s_scan;  // the stream of the planning kernels and the second scan
    auto behind_first_scan = [&]() -> int {
        if (s2 != h->s_scan) {
            RT_HIP(h, hipEventRecord(sl.ev_first, h->s_scan));
            RT_HIP(h, hipStreamWaitEvent(s2, sl.ev_first, 0));
        }
        return RT_OK;
    };
    if (dense) {
        launch_scan<1>(h, sp, blocks, c.fmt);
    } else if (mode == RT_MODE_RUNFILTER) {
        // threshold bits of every cell (+ row sums, tail) -> cells of runs long enough -> only their segments again
        sp.thr_bin = sl.d_thr_bin;
        sp.abs_hot = sl.d_abs_hot;
        launch_scan<6>(h, sp, blocks, c.fmt);
        sp.thr_bin = nullptr;
        sp.abs_hot = nullptr;
        { const int rc = behind_first_scan(); if (rc != RT_OK) return rc; }
        {
            // one launch behind the scan: the largest per-stream count of cells over the absolute threshold (AUTO's probes), the
            // check of the per-bin thresholds against this buffer's row means, the segment counters back to zero
            const int64_t cells = (int64_t)S * h->N;
            hipLaunchKernelGGL(after_bit_scan, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s2, sl.d_abs_hot, sl.h_abs_hot, sl.d_thr_nat, sl.d_psum, S, h->N,
                               sp.blocks_per_stream, c.n_seg, h->cfg.snr_threshold, h->d_set_s, sl.h_overflow, sl.d_counters, kFlagHotOverflow | kFlagThrStale,
                               const_cast<int32_t *>(sp.seg_count), absent);
        }
        sl.call.abs_counted = true;
        {
            // (a run needs r cells: more than the buffer holds means "only the run through t = 0", which r = n_seg + 1 says as well)
            const int r = (int)std::min<long long>(h->run_cells, (long long)c.n_seg + 1);
            const int tile = plan_tile_rows(c.n_seg, h->LG, r);
            const int tpw = 64 / (h->LG / 4);
            const int waves = (c.n_seg + tpw * tile - 1) / (tpw * tile);
            const size_t plan_lds = ((size_t)tpw * tile + 3) & ~(size_t)3;
            auto *kern = r <= 16 ? plan_runs<4> : r <= 256 ? plan_runs<8> : plan_runs<16>;
            hipLaunchKernelGGL(kern, dim3(S, waves), dim3(64), plan_lds, s2, sp.cell_hot, sl.d_cell_need,
                               sl.d_seg_list, const_cast<int32_t *>(sp.seg_count), c.n_seg, h->LG, r, tile, absent);
        }
        launch_scan<7>(h, sp, blocks, c.fmt, s2);
    } else if (mode == RT_MODE_PREFILTER) {
        if (!second_pass_only) {
            sp.abs_hot = sl.d_abs_hot;
            launch_scan<4>(h, sp, blocks, c.fmt);
            sp.abs_hot = nullptr;
        }
        { const int rc = behind_first_scan(); if (rc != RT_OK) return rc; }
        if (!second_pass_only) {
            hipLaunchKernelGGL(max_abs_hot, dim3(1), dim3(256), 0, s2, sl.d_abs_hot, S, sl.h_abs_hot);
            sl.call.abs_counted = true;
        }
        hipLaunchKernelGGL(plan_pass_b, dim3(S), dim3(256), sizeof(uint32_t) * ((sp.chunks + 31) / 32), s2, sp.full, sp.first,
                           sp.item_chunks, sp.item_count, h->LG, sp.segs_per_chunk, c.n_seg, sp.chunks, sp.blocks_per_stream, h->GPW, absent);
        launch_scan<5>(h, sp, blocks, c.fmt, s2);
    } else {
#ifdef RT_STAMPS  // diagnostic build: per-stage cycle sums of every wave of the sparse scan, averaged and printed (stderr)
        static uint32_t *d_dbg = nullptr;
        static size_t dbg_words = 0;
        const size_t words = (size_t)blocks * (scan_block(h->R3) / 64) * kStamps;
        if (words > dbg_words) {
            if (d_dbg) (void)hipFree(d_dbg);
            RT_HIP(h, hipMalloc(&d_dbg, words * sizeof(uint32_t)));
            dbg_words = words;
        }
        RT_HIP(h, hipMemsetAsync(d_dbg, 0, words * sizeof(uint32_t), h->s_scan));
        sp.dbg = d_dbg;
#endif
        launch_scan<0>(h, sp, blocks, c.fmt);
#ifdef RT_STAMPS
        {
            std::vector<uint32_t> hd(words);
            RT_HIP(h, hipStreamSynchronize(h->s_scan));
            RT_HIP(h, hipMemcpy(hd.data(), d_dbg, words * sizeof(uint32_t), hipMemcpyDeviceToHost));
            double sum[kStamps] = {};
            double waves = 0;
            for (size_t w = 0; w < words / kStamps; ++w) {
                if (hd[w * kStamps + 11] == 0) continue;
                waves += 1;
                for (int k = 0; k < kStamps; ++k) sum[k] += hd[w * kStamps + k];
            }
            if (const char *dump = RT_DIAG_ENV("RT_STAMPS_DUMP")) {  // raw per-wave words of the last launch, for timelines
                if (FILE *f = std::fopen(dump, "wb")) {
                    std::fwrite(hd.data(), sizeof(uint32_t), words, f);
                    std::fclose(f);
                }
            }
            uint32_t t_min = 0xFFFFFFFFu, t_max = 0;
            double resident = 0;  // wave lifetimes, 100-MHz ticks
            for (size_t w = 0; w < words / kStamps; ++w) {
                if (hd[w * kStamps + 11] == 0) continue;
                t_min = std::min(t_min, hd[w * kStamps + 14]);
                t_max = std::max(t_max, hd[w * kStamps + 15]);
                resident += (double)(hd[w * kStamps + 15] - hd[w * kStamps + 14]);
            }
            const double span = (double)(t_max - t_min);
            std::fprintf(stderr, "RT_STAMPS launch span %.1f us, %.2f waves resident per SIMD on average, %.1f %% of a wave's life inside the step loop; ",
                         span / 100.0, resident / span / 1024.0, 100.0 * sum[13] / resident);
            const double steps = sum[11];
            double tot = 0;
            for (int k = 0; k <= 10; ++k) tot += sum[k];
            std::fprintf(stderr, "RT_STAMPS nperseg %d: %.0f waves, %.1f steps per wave, %.0f cycles per step, in-kernel clock %.0f MHz:", h->N, waves,
                         steps / waves, tot / steps, sum[13] > 0 ? sum[12] / sum[13] * 100.0 : 0.0);
            for (int k = 0; k <= 10; ++k) std::fprintf(stderr, " [%d] %.0f", k, sum[k] / steps);
            std::fprintf(stderr, "\n");
        }
#endif
    }
    RT_HIP(h, hipGetLastError());
    // (ev_scan: the end of the call's scans -- on `sd` where a second scan ran there)
    const bool two_scans = !dense && (mode == RT_MODE_RUNFILTER || mode == RT_MODE_PREFILTER);
    // (rt_set_chain: behind the call's last scan, where ev_scan is recorded -- s2 is behind the first scan, which wrote the columns)
    { const int rc = enqueue_chain(h, sl, two_scans ? s2 : h->s_scan); if (rc != RT_OK) return rc; }
    RT_HIP(h, hipEventRecord(sl.ev_scan, two_scans ? s2 : h->s_scan));
    if (sd != (two_scans ? s2 : h->s_scan)) RT_HIP(h, hipStreamWaitEvent(sd, sl.ev_scan, 0));
    DetectArgs a = make_detect_args(h, sl, c.n_seg, h->N, c.n_seg_last);
    a.prev = call_prev(h, sl);
    a.prev_cols = h->K;
    a.chunks = sp.blocks_per_stream;
    a.spec = h->d_spec;
    a.filtered = (mode == RT_MODE_PREFILTER || mode == RT_MODE_RUNFILTER) ? 1 : 0;
    if (mode == RT_MODE_RUNFILTER) {
        a.seg_total = sp.seg_count + S;  // (the planner's batch total -> pinned host word, by the call's last finalize_records workgroup)
        a.host_seg_total = sl.h_seg_total;
    }
    if (dense) {
        launch_detect_dense(h, S, sd, a);
    } else {
        if (a.work_list) {
            // thousands of streams with a few hundred cells each: a wave per stream (detect_group), the per-list waves only for the
            // streams it leaves -- a looping grid that finds its work list empty as a rule
            hipLaunchKernelGGL(detect_group, dim3((S + 3) / 4), dim3(256), h->lds_small, sd, a);
            hipLaunchKernelGGL(detect_bucket_listed, dim3(std::min(S * kQuarters, 1024)), dim3(256), h->lds_small, sd, a);
        } else {
            const int waves = S * kBuckets;
            hipLaunchKernelGGL(detect_bucket<false>, dim3((waves + 3) / 4), dim3(256), h->lds_small, sd, a);
        }
        // (the large instantiation returns at once for a stream without a bucket over kSmallBucket cells; the per-bucket counters
        // are put back to zero by finalize_records)
        hipLaunchKernelGGL(detect_bucket<true>, dim3(S), dim3(256), h->lds_large, sd, a);  // one workgroup per stream: its 16 buckets in turn
        // (RT_FLAG_RECORD_CELLS: the gather needs the lists' lengths, which finalize_records puts back to zero)
        if (sl.d_cells) hipLaunchKernelGGL(cells_keep_counts, dim3((S * kBuckets + 255) / 256), dim3(256), 0, sd, sl.d_hot_count, sl.d_hot_kept, S * kBuckets);
        hipLaunchKernelGGL(finalize_records, dim3(S), dim3(256), 0, sd, a);
    }
    RT_HIP(h, hipGetLastError());
    { const int rc = enqueue_row_means(h, sl, sp.blocks_per_stream, c.n_seg, sd); if (rc != RT_OK) return rc; }
    { const int rc = enqueue_record_cells(h, sl, dense ? h->d_spec : nullptr, nullptr, 0, sd); if (rc != RT_OK) return rc; }
    // no readback: the call's last workgroup wrote the counter words to pinned host memory
    RT_HIP(h, hipEventRecord(sl.ev_done, sd));
    return RT_OK;
}

// AUTO: a few streams of the batch overflowed their candidate lists (one noisy SDR among hundreds): only they are
// analysed again, on the dense path, while the records of the others stand.  The scan and detect_dense take the
// list of streams; the records go behind the ones already in the pool (the counter word is put back first), the
// streams' offset / count entries are simply overwritten.
int enqueue_partial_dense(rt_handle *h, Slot &sl, int n_list, unsigned long long records_so_far) {
    const CallCtx &c = sl.call;
    const int n_part = std::min(h->cfg.n_streams, kMaxPartial);
    if (!h->d_spec_part) {
        const size_t bytes = (size_t)n_part * (size_t)h->max_seg * (size_t)h->N * sizeof(float);
        hipError_t e = hipMalloc(&h->d_spec_part, bytes ? bytes : 4);
        if (e != hipSuccess) {
            h->d_spec_part = nullptr;
            h->err = "dense spectrogram scratch for the partial re-run (" + std::to_string(bytes) + " bytes): " + hipGetErrorString(e);
            return RT_E_NOMEM;
        }
    }
    StftParams sp = make_stft_params(h, sl, c.iq, c.stream_stride, c.n_seg, c.tail_write);
    sp.n_streams = n_list;
    sp.stream_list = sl.h_list;  // pinned host memory, device-visible: a few dozen scalar loads per workgroup
    sp.spec = h->d_spec_part;
    *sl.h_total = records_so_far;
    RT_HIP(h, hipMemcpyAsync(sl.d_counters, sl.h_total, sizeof(unsigned long long), hipMemcpyHostToDevice, h->s_scan));
    launch_scan<1>(h, sp, n_list * sp.blocks_per_stream, c.fmt);
    RT_HIP(h, hipGetLastError());
    { const int rc = enqueue_chain(h, sl, h->s_scan); if (rc != RT_OK) return rc; }  // (the dense scan rewrote the listed streams' columns)
    DetectArgs a = make_detect_args(h, sl, c.n_seg, h->N, c.n_seg_last);
    a.prev = call_prev(h, sl);
    a.prev_cols = h->K;
    a.chunks = sp.blocks_per_stream;
    a.spec = h->d_spec_part;
    a.stream_list = sl.h_list;
    launch_detect_dense(h, n_list, h->s_scan, a);
    RT_HIP(h, hipGetLastError());
    // (the dense scan rewrote the listed streams' partial sums -- the same chunks --, the others stand: all S rows again)
    { const int rc = enqueue_row_means(h, sl, sp.blocks_per_stream, c.n_seg, h->s_scan); if (rc != RT_OK) return rc; }
    // (the listed streams' cells from this map, the others' from their candidate lists, whose kept counters stand)
    { const int rc = enqueue_record_cells(h, sl, h->d_spec_part, sl.h_list, n_list, h->s_scan); if (rc != RT_OK) return rc; }
    RT_HIP(h, hipEventRecord(sl.ev_done, h->s_scan));
    return RT_OK;
}

// A call needed more records than the slot's pinned pool holds: a larger pool (the reference appends without limit,
// analyze.py:449-450; here the limit is what the streams' record_capacity can deliver).  Only while none of the slot's
// kernels is in flight.  Failure leaves the old pool in place.
int grow_pool(rt_handle *h, Slot &sl, int64_t want) {
    want = std::min(want, h->pool_max);
    if (want <= sl.pool_cap) return RT_OK;
    int64_t cap = std::min(h->pool_max, std::max(want + want / 4, 2 * sl.pool_cap));
    rt_record *p = nullptr;
    hipError_t e = hipHostMalloc(&p, (size_t)cap * sizeof(rt_record));
    if (e != hipSuccess && cap > want) {
        cap = want;
        e = hipHostMalloc(&p, (size_t)cap * sizeof(rt_record));
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        h->err = "record pool of " + std::to_string(cap) + " records: " + hipGetErrorString(e);
        return RT_E_NOMEM;
    }
    (void)hipHostFree(sl.h_records);
    sl.h_records = p;
    sl.pool_cap = cap;
    h->pool_want = std::max(h->pool_want, cap);
    return RT_OK;
}

// A stream of the call wanted more records than the handle's per-stream capacity (word 4 of the counters): the capacity --
// rt_config.record_capacity is where it STARTS -- grows to hold them, for this call and every later one.  The reference appends
// signals without limit (analyze.py:449-450); here the limit is the memory: per stream and slot 40 bytes a record of raw-record
// area, and what the pinned pool may then be asked to hold.  Everything in flight is waited for first (the other slot's kernels
// write their own raw-record area, which is replaced as well).  Failure leaves the old capacity in place.
int grow_record_capacity(rt_handle *h, unsigned long long wanted) {
    if (wanted <= (unsigned long long)h->rec_cap) return RT_OK;
    if (wanted > (1ull << 24)) wanted = 1ull << 24;  // (a buffer of 2^24 records per stream is beyond any key space the scans have)
    const int cap = next_pow2((int)wanted);
    RT_HIP(h, hipStreamSynchronize(h->s_scan));
    RT_HIP(h, hipStreamSynchronize(h->s_detect));
    const size_t bytes = (size_t)h->cfg.n_streams * (size_t)cap * sizeof(rt_record);
    rt_record *fresh[kSlots] = {nullptr, nullptr};
    for (int i = 0; i < kSlots; ++i) {
        if (hipMalloc(&fresh[i], bytes) != hipSuccess) {
            (void)hipGetLastError();
            for (int j = 0; j < i; ++j) (void)hipFree(fresh[j]);
            h->err = "raw-record area for " + std::to_string(cap) + " records per stream (" + std::to_string(bytes) + " bytes per slot) does not fit the device";
            return RT_E_NOMEM;
        }
    }
    for (int i = 0; i < kSlots; ++i) {
        (void)hipFree(h->slot[i].d_raw);
        h->slot[i].d_raw = fresh[i];
    }
    h->rec_cap = cap;
    h->lds_dense = rec_lds_bytes(cap);
    h->pool_max = ((int64_t)h->cfg.n_streams + std::min(h->cfg.n_streams, kMaxPartial)) * cap;
    return RT_OK;
}

// claim the slot of the next call; the GPU work of the call that used it last must be over
// before its scratch is rewritten (its results, if never fetched, are dropped)
// ---- rt_set_record_iq: the sample tails and the gather (rt_record_iq.h; the decisions: rt_record_iq_book.h) ----
int iq_nperseg(const rt_handle *h) { return h->f64 ? h->f64->N : h->N; }
int iq_sample_bytes(const rt_handle *h, int fmt) { return (h->f64 && fmt == kFmtC64) ? 16 : (int)fmt_sample_bytes(fmt); }

// The tail area for samples of `bps` bytes: made at first need, and made again for a wider format.  Every row keeps its place
// and its bytes (a pending call's fetch may still read the narrow tails), so a wider format loses nothing.
int iq_tail_area(rt_handle *h, int bps) {
    RecordIq &q = *h->riq;
    if (q.d_tails && bps <= q.area_bps) return RT_OK;
    const int64_t row = ((int64_t)h->ledger.iq.cols() * iq_nperseg(h) * bps + 15) / 16 * 16;
    const size_t rows = (size_t)kIqRows * (size_t)h->cfg.n_streams;
    char *area = nullptr;
    if (hipMalloc(&area, std::max<size_t>(rows * (size_t)row, 16)) != hipSuccess) {
        (void)hipGetLastError();
        h->err = "rt_set_record_iq: no device memory for the sample tails (" + std::to_string(rows * (size_t)row) + " bytes)";
        return RT_E_NOMEM;
    }
    if (q.d_tails) {
        hipError_t e = hipStreamSynchronize(h->s_scan);  // (kernels in flight write and read the old rows)
        if (e == hipSuccess) e = hipStreamSynchronize(q.s_gather);
        if (e == hipSuccess) e = hipMemcpy2D(area, (size_t)row, q.d_tails, (size_t)q.row_bytes, (size_t)q.row_bytes, rows, hipMemcpyDeviceToDevice);
        if (e != hipSuccess) {
            (void)hipFree(area);
            h->err = std::string("rt_set_record_iq: moving the sample tails: ") + hipGetErrorString(e);
            return RT_E_HIP;
        }
        (void)hipFree(q.d_tails);
    }
    q.d_tails = area;
    q.row_bytes = row;
    q.area_bps = bps;
    return RT_OK;
}

// At enqueue, in front of the scan, on a float32 and a float64 handle alike: the ledger's decisions for the call that takes slot
// `idx` go into `lc` (they stay in the slot for the call's fetch and every re-analysis), and with rt_set_record_iq on the rows the
// call writes go to the device and iq_tails onto the scan's stream.  `other`: the other slot's snapshot while its call is pending,
// else null.  `slot_done`: the event behind the slot's previous call (null: it never held one) -- the pinned rows are rewritten.
// Everything that can fail comes before the ledger moves or puts it back: a failure leaves the ledger as it was.
int begin_ledger_call(rt_handle *h, int idx, LedgerCall &lc, const LedgerCall *other, hipEvent_t slot_done, int T, int fmt, const void *iq,
                      int64_t stream_stride) {
    StreamLedger &led = h->ledger;
    const int S = h->cfg.n_streams, N = iq_nperseg(h), bps = iq_sample_bytes(h, fmt);
    if (led.iq.on()) {
        const int rc = iq_tail_area(h, bps);
        if (rc != RT_OK) return rc;
        if (slot_done) RT_HIP(h, hipEventSynchronize(slot_done));
    }
    led.begin_call(T, fmt, other && other->iq_on ? &other->iq : nullptr, lc);
    if (!lc.iq_on) return RT_OK;
    RecordIq &q = *h->riq;
    IqSlot &qs = q.slot[idx];
    const int D = std::min(T, led.iq.cols());
    bool any = false;
    for (int s = 0; s < S; ++s) {
        qs.h_rows[s] = lc.iq.write_buf[(size_t)s];
        any = any || qs.h_rows[s] >= 0;
    }
    if (D <= 0 || !any) return RT_OK;
    IqTailsArgs a{};
    a.iq = static_cast<const char *>(iq);
    a.stream_stride = stream_stride;
    a.bps = bps;
    a.n_streams = S;
    a.src_sample = (int64_t)(T - D) * N;
    a.bytes = (int64_t)D * N * bps;  // (<= row_bytes: D <= K + m, bps <= area_bps)
    a.tiles_per_stream = (int32_t)((a.bytes + kIqTileBytes - 1) / kIqTileBytes);
    a.write_buf = qs.d_rows;
    a.tails = q.d_tails;
    a.row_bytes = q.row_bytes;
    hipError_t e = hipMemcpyAsync(qs.d_rows, qs.h_rows, (size_t)S * sizeof(int32_t), hipMemcpyHostToDevice, h->s_scan);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(iq_tails, dim3((unsigned)S * (unsigned)a.tiles_per_stream), dim3(kIqBlock), 0, h->s_scan, a);
        e = hipGetLastError();
    }
    if (e != hipSuccess) {
        led.rollback(lc);
        h->err = std::string("iq_tails: ") + hipGetErrorString(e);
        return RT_E_HIP;
    }
    return RT_OK;
}

// The argument check of rt_process* on a float32 and a float64 handle alike; *T = the call's whole segments.  `device_ptr`: the
// scan kernel loads whole samples from `iq` (8-byte complex64 -- 16-byte complex128 on a float64 handle -- / 2-byte uint8 or int8
// / 4-byte int16 I,Q pairs): a misaligned pointer would fault on the device, so it is refused here (a host buffer is staged).
int check_process_args(rt_handle *h, const void *iq, int64_t n_samples, int64_t stream_stride, int fmt, bool device_ptr, int *T) {
    if (!iq && n_samples > 0) {
        h->err = "null IQ pointer";
        return RT_E_INVALID;
    }
    if (n_samples < 0 || n_samples > h->cfg.max_samples || stream_stride < n_samples) {
        h->err = "n_samples/stream_stride out of range for this handle";
        return RT_E_INVALID;
    }
    if (device_ptr && reinterpret_cast<uintptr_t>(iq) % (size_t)iq_sample_bytes(h, fmt) != 0) {
        h->err = fmt == kFmtU8 ? "IQ pointer must be 2-byte aligned (uint8 I,Q pairs)"
                 : fmt == kFmtI16 ? "IQ pointer must be 4-byte aligned (int16 I,Q pairs)"
                 : fmt == kFmtI8 ? "IQ pointer must be 2-byte aligned (int8 I,Q pairs)"
                 : h->f64 ? "IQ pointer must be 16-byte aligned (complex128 on a float64 handle)" : "IQ pointer must be 8-byte aligned (complex64)";
        return RT_E_INVALID;
    }
    *T = (int)(n_samples / iq_nperseg(h));
    if (*T == 1) {
        h->err = "exactly one segment: the reference raises IndexError (times[1])";
        return RT_E_ONE_SEGMENT;
    }
    return RT_OK;
}

// Inside rt_fetch*, behind the delivery of the call in slot `idx` in full: its records -> offsets, first segments and the copy
// list; the pool grown to what they need; the gather, waited for (the call's IQ need not outlive the fetch).  What goes wrong is
// kept for rt_fetch_record_iq to report: the fetch itself has delivered.
void iq_gather(rt_handle *h, int idx, const IqCall &call, const void *rec, size_t rec_stride, size_t n, const void *iq, int64_t stream_stride) {
    RecordIq &q = *h->riq;
    IqSlot &qs = q.slot[idx];
    const int S = h->cfg.n_streams, N = iq_nperseg(h), bps = iq_sample_bytes(h, call.fmt);
    q.delivered = idx;
    qs.state = RT_OK;
    qs.bps = bps;
    qs.offsets.assign(n + 1, 0);
    qs.first_seg.assign(n, 0);
    qs.fmt = call.fmt;
    for (IqProduct &p : qs.prod) p.k = 0;
    qs.fi.resize(n);
    qs.start.resize(n);
    qs.end.resize(n);
    for (size_t i = 0; i < n; ++i) {
        const int32_t *const r = reinterpret_cast<const int32_t *>(static_cast<const char *>(rec) + i * rec_stride);
        qs.fi[i] = r[1];
        qs.start[i] = r[2];
        qs.end[i] = r[3];
    }
    std::vector<IqDesc> descs;
    const int64_t total = iq_build_descs(call, N, rec, rec_stride, n, qs.offsets.data(), qs.first_seg.data(), &descs);
    if (descs.empty()) return;
    const auto fail = [&](int code, const std::string &why) {
        (void)hipGetLastError();
        qs.state = code;
        qs.why = why;
    };
    if (!iq_descs_in_bounds(descs, S, (int64_t)call.T * N, (int64_t)h->ledger.iq.cols() * N, total) || !q.d_tails)
        return fail(RT_E_HIP, "internal: a record's samples lie outside the buffers the handle holds");
    const size_t bytes = (size_t)total * (size_t)bps;
    if (qs.pool_bytes < bytes) {
        (void)hipFree(qs.d_pool);
        qs.d_pool = nullptr;
        const size_t want = std::max(bytes, std::max(qs.pool_bytes * 2, kInitialIqPoolBytes));
        qs.pool_bytes = 0;
        if (hipMalloc(&qs.d_pool, want) != hipSuccess) {
            (void)hipGetLastError();
            if (want == bytes || hipMalloc(&qs.d_pool, bytes) != hipSuccess) return fail(RT_E_NOMEM, "no device memory for the call's samples (" + std::to_string(bytes) + " bytes)");
            qs.pool_bytes = bytes;
        } else {
            qs.pool_bytes = want;
        }
    }
    std::vector<int64_t> tile_first;
    const int64_t tiles = iq_tile_prefix(descs, bps, &tile_first);
    const size_t list_bytes = descs.size() * sizeof(IqDesc), need = list_bytes + tile_first.size() * sizeof(int64_t);
    if (qs.desc_bytes < need) {
        (void)hipHostFree(qs.h_descs);
        (void)hipFree(qs.d_descs);
        qs.h_descs = qs.d_descs = nullptr;
        qs.desc_bytes = 0;
        const size_t want = std::max(need, (size_t)1 << 16);
        if (hipHostMalloc(&qs.h_descs, want) != hipSuccess || hipMalloc(&qs.d_descs, want) != hipSuccess) return fail(RT_E_NOMEM, "no memory for the copy list");
        qs.desc_bytes = want;
    }
    std::memcpy(qs.h_descs, descs.data(), list_bytes);  // (sizeof(IqDesc) is a multiple of 8: the prefix behind it is aligned)
    std::memcpy(qs.h_descs + list_bytes, tile_first.data(), tile_first.size() * sizeof(int64_t));
    IqGatherArgs a{};
    a.descs = reinterpret_cast<const IqDesc *>(qs.d_descs);
    a.tile_first = reinterpret_cast<const int64_t *>(qs.d_descs + list_bytes);
    a.n_descs = (int32_t)descs.size();
    a.bps = bps;
    a.n_streams = S;
    a.iq = static_cast<const char *>(iq);
    a.stream_stride = stream_stride;
    a.tails = q.d_tails;
    a.row_bytes = q.row_bytes;
    a.pool = qs.d_pool;
    // (one copy for the list and its prefix; the call's own iq_tails and everything before it ended in front of the call's ev_done)
    hipError_t e = hipMemcpyAsync(qs.d_descs, qs.h_descs, need, hipMemcpyHostToDevice, q.s_gather);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(record_iq_gather, dim3((unsigned)tiles), dim3(kIqBlock), 0, q.s_gather, a);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(q.s_gather);
    if (e != hipSuccess) fail(RT_E_HIP, std::string("record_iq_gather: ") + hipGetErrorString(e));
}

// rt_destroy (the device is idle by then), and a failed first rt_set_record_iq
void iq_free(rt_handle *h) {
    RecordIq *q = h->riq;
    if (!q) return;
    for (IqSlot &qs : q->slot) {
        (void)hipHostFree(qs.h_rows);
        (void)hipFree(qs.d_rows);
        (void)hipFree(qs.d_pool);
        (void)hipHostFree(qs.h_descs);
        (void)hipFree(qs.d_descs);
        for (IqProduct &p : qs.prod) {
            (void)hipFree(p.out);
            (void)hipFree(p.work);
        }
    }
    (void)hipFree(q->d_stft_tw);
    (void)hipFree(q->d_stft_win);
    (void)hipFree(q->d_tails);
    if (q->s_gather) (void)hipStreamDestroy(q->s_gather);
    delete q;
    h->riq = nullptr;
}

// rt_fetch_record_iq and rt_fetch_record_stft hand out the same delivered call: the lanes that hold it, and what each refuses --
// `entry` names the caller in the message.  *records, *samples: over all lanes; *bps: of the delivered call.
int iq_delivered_call(rt_handle *h, const char *entry, std::vector<rt_handle *> *lanes, size_t *records, size_t *samples, int *bps) {
    const auto refuse = [&](const char *why) {
        h->err = std::string(entry) + ": " + why;
        return RT_E_INVALID;
    };
    if (h->iq_margin < 0) return refuse("rt_set_record_iq has not turned the feature on");
    if (h->kids.empty()) lanes->assign(1, h);
    else *lanes = h->kids;
    // every lane holds the samples of its streams' records: all of them are checked and counted before anything is written
    *records = *samples = 0;
    *bps = 0;
    for (rt_handle *l : *lanes) {
        const int d = l->riq ? l->riq->delivered : kIqNone;
        if (d == kIqExtract) return refuse("the call fetched last was an rt_extract: it has no samples");
        if (d == kIqTruncated) return refuse("the call fetched last was delivered truncated");
        if (d == kIqOff) return refuse("the call fetched last was enqueued before the feature was turned on");
        if (d < 0) return refuse("no samples: no call delivered by rt_fetch since the last rt_process*, rt_extract, rt_reset or rt_set_record_iq");
        const IqSlot &qs = l->riq->slot[d];
        if (qs.state != RT_OK) {
            h->err = std::string(entry) + ": " + qs.why;
            return qs.state;
        }
        *records += qs.first_seg.size();
        *samples += (size_t)qs.offsets.back();
        *bps = qs.bps;
    }
    return RT_OK;
}

// ---- the rt_fetch_record_* family on the delivered call's byte pool (the plans: rt_record_stft_book.h).  Three entries hand out
// frames -- rt_fetch_record_stft, _stft_hop, _band -- and two one row per record, reduced on the device from the hop and the band
// product: rt_fetch_record_estimates, _spectrum.  Each leaves an IqProduct in the slot; what they share stands here once. ----
// Every message starts with the entry's name and goes to `h`, the handle the caller holds; the work is done on `l`, the lane-less
// handle that holds the records.
inline int record_refuse(rt_handle *h, const char *entry, const std::string &why, int code = RT_E_INVALID) {
    h->err = std::string(entry) + ": " + why;
    return code;
}
inline int record_mismatch(rt_handle *h, const char *entry) {
    return record_refuse(h, entry, "internal: the delivered call's record list does not match its snippets", RT_E_HIP);
}
inline int record_nomem(rt_handle *h, const char *entry, const char *what, size_t bytes) {
    (void)hipGetLastError();
    return record_refuse(h, entry, std::string("no device memory for ") + what + " (" + std::to_string(bytes) + " bytes)", RT_E_NOMEM);
}

// The twiddle table and (float32: a float64 handle's is F64State::d_window) the window go to the device with the first call of any
// entry of the family that has something to compute, and are shared by all of them.
template <class P>
int record_tables(rt_handle *h, rt_handle *l, const char *entry) {
    using C = typename stft_types<P>::C;
    RecordIq &q = *l->riq;
    const int N = iq_nperseg(l);
    const auto upload = [&](const void *src, size_t bytes, const char *what, void **to) {
        void *d = nullptr;
        if (hipMalloc(&d, bytes) != hipSuccess) return record_nomem(h, entry, what, bytes);
        if (hipMemcpy(d, src, bytes, hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipFree(d);
            return record_refuse(h, entry, std::string("uploading ") + what + " failed", RT_E_HIP);
        }
        *to = d;
        return (int)RT_OK;
    };
    if (!q.d_stft_tw) {
        const std::vector<C> tw = record_stft_twiddles<C, typename std::conditional<sizeof(P) == 4, double, long double>::type>(N);
        const int rc = upload(tw.data(), tw.size() * sizeof(C), "the twiddle table", &q.d_stft_tw);
        if (rc != RT_OK) return rc;
    }
    if (!l->f64 && !q.d_stft_win) {
        void *d = nullptr;
        const int rc = upload(l->h_window.data(), (size_t)N * sizeof(float), "the window", &d);
        if (rc != RT_OK) return rc;
        q.d_stft_win = static_cast<float *>(d);
    }
    return RT_OK;
}

// a device pool that grows on demand, like the byte pool: at least `need` bytes in *p, doubling
inline bool product_grow(char **p, size_t *have, size_t need) {
    if (*have >= need) return true;
    (void)hipFree(*p);
    *p = nullptr;
    const size_t want = std::max(need, std::max(*have * 2, (size_t)1 << 16));
    *have = 0;
    if (hipMalloc(p, want) == hipSuccess) {
        *have = want;
        return true;
    }
    (void)hipGetLastError();
    if (want == need || hipMalloc(p, need) != hipSuccess) {
        (void)hipGetLastError();
        *p = nullptr;
        return false;
    }
    *have = need;
    return true;
}

// A product that does not hold the wanted key is built in two steps.  The first makes room: the key goes before either pool is
// touched -- a pool that grows loses what it held, and whatever it held is gone once the kernel writes -- so a call that fails from
// here on leaves a product that holds nothing, never one that names values it has lost.
inline int product_begin(rt_handle *h, const char *entry, IqProduct &p, size_t out_bytes, const char *out_what, size_t work_bytes, const char *work_what) {
    p.k = 0;
    if (!product_grow(&p.out, &p.out_bytes, out_bytes)) return record_nomem(h, entry, out_what, out_bytes);
    if (!product_grow(&p.work, &p.work_bytes, work_bytes)) return record_nomem(h, entry, work_what, work_bytes);
    return RT_OK;
}
// The second uploads the work list `packed` into p.work, runs `launch` behind it on the gather's stream and waits; the product
// holds (k, w) only where all of that went well.  `packed` is a pageable source: it lives until the stream has been waited for.
template <class Launch>
int product_finish(rt_handle *h, RecordIq &q, const char *entry, IqProduct &p, int k, int w, const std::vector<char> &packed, const char *kernel,
                   Launch launch) {
    hipError_t e = hipMemcpyAsync(p.work, packed.data(), packed.size(), hipMemcpyHostToDevice, q.s_gather);
    if (e == hipSuccess) {
        launch();
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(q.s_gather);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(q.s_gather);  // (`packed` must outlive whatever copy did start)
        (void)hipGetLastError();
        return record_refuse(h, entry, std::string(kernel) + ": " + hipGetErrorString(e), RT_E_HIP);
    }
    p.set(k, w);
    return RT_OK;
}

// `f` with the delivered call's input format as a compile-time constant: f(std::integral_constant<int, kFmt...>)
template <class F>
void with_record_format(int fmt, F f) {
    if (fmt == kFmtU8) f(std::integral_constant<int, kFmtU8>{});
    else if (fmt == kFmtI16) f(std::integral_constant<int, kFmtI16>{});
    else if (fmt == kFmtI8) f(std::integral_constant<int, kFmtI8>{});
    else f(std::integral_constant<int, kFmtC64>{});
}

// in front of a launch that reads the byte pool: the pool holds what the record list says, and the grid fits an unsigned
inline bool record_pool_ok(const IqSlot &qs, int64_t frames, int64_t per_block) {
    return (uint64_t)qs.offsets.back() * (uint64_t)qs.bps <= qs.pool_bytes && (frames == 0 || qs.d_pool) && (frames + per_block - 1) / per_block <= 0x7fffffffll;
}

// what the arguments of record_stft and record_stft_hop share: the byte pool, the tables and sqrt(scale)
template <class P, class Args>
void record_pool_args(rt_handle *l, Args &a) {
    const RecordIq &q = *l->riq;
    const IqSlot &qs = q.slot[q.delivered];
    a.pool = qs.d_pool;
    a.n_records = (int32_t)qs.first_seg.size();
    a.nperseg = iq_nperseg(l);
    a.tw = static_cast<const typename stft_types<P>::C *>(q.d_stft_tw);
    if constexpr (sizeof(P) == 4) {
        a.window = q.d_stft_win;
        a.root = stft_root_f32(l->cfg.scale);
    } else {
        a.window = l->f64->d_window;
        a.root = stft_root_f64(l->f64->c.scale);
    }
}

// ---- rt_fetch_record_stft: one complex STFT value per delivered segment (rt_record_stft.h) ----
template <class P, int FMT>
void launch_record_stft(const StftArgs<P> &a, hipStream_t st) {
    const int64_t blocks = (a.n_segs + kStftWaves - 1) / kStftWaves;
    hipLaunchKernelGGL((record_stft<P, FMT>), dim3((unsigned)blocks), dim3(kStftBlock), 0, st, a);
}

// The values of lane-less handle `l`'s delivered call into its slot's kProdStft, once per delivered call, under key (1, 0).  A frame
// is a delivered segment here, so the entry has no frame plan (record_plan): the kernel's list is made where it is needed -- a
// repeated call, which only copies, pays for none.
template <class P>
int record_stft_run(rt_handle *h, rt_handle *l, const char *entry, int k, int w, const StftHopWork &, int64_t) {
    using C = typename stft_types<P>::C;
    RecordIq &q = *l->riq;
    IqSlot &qs = q.slot[q.delivered];
    IqProduct &p = qs.prod[kProdStft];
    if (p.holds(k, w)) return RT_OK;
    const size_t n = qs.first_seg.size();
    StftWork work;
    const int64_t cells = stft_build_work(qs.offsets.data(), qs.fi.data(), n, iq_nperseg(l), &work);
    if (cells < 0 || !record_pool_ok(qs, cells, kStftWaves)) return record_mismatch(h, entry);
    if (cells == 0) {
        p.set(k, w);
        return RT_OK;
    }
    RT_HIP(h, hipSetDevice(l->cfg.device));
    int rc = record_tables<P>(h, l, entry);
    if (rc != RT_OK) return rc;
    // the work list in one piece: seg_first [n + 1], fi [n]
    const size_t b_first = (n + 1) * sizeof(int64_t), b_i32 = n * sizeof(int32_t);
    rc = product_begin(h, entry, p, (size_t)cells * sizeof(C), "the call's values", b_first + b_i32, "the work list");
    if (rc != RT_OK) return rc;
    std::vector<char> packed(b_first + b_i32);
    std::memcpy(packed.data(), work.seg_first.data(), b_first);
    std::memcpy(packed.data() + b_first, work.fi.data(), b_i32);
    StftArgs<P> a{};
    record_pool_args<P>(l, a);
    a.seg_first = reinterpret_cast<const int64_t *>(p.work);
    a.fi = reinterpret_cast<const int32_t *>(p.work + b_first);
    a.n_segs = cells;
    a.values = reinterpret_cast<C *>(p.out);
    return product_finish(h, q, entry, p, k, w, packed, "record_stft", [&] {
        with_record_format(qs.fmt, [&](auto fmt) { launch_record_stft<P, decltype(fmt)::value>(a, q.s_gather); });
    });
}

// ---- rt_fetch_record_stft_hop: the same values for frames every nperseg / k samples (rt_record_stft_hop.h) ----
template <class P, int FMT>
void launch_record_stft_hop(const StftHopArgs<P> &a, int group, hipStream_t st) {
    const int64_t per_block = (int64_t)kStftWaves * (64 / group);
    const dim3 grid((unsigned)((a.n_frames + per_block - 1) / per_block)), block(kStftBlock);
    if (group == 8) hipLaunchKernelGGL((record_stft_hop<P, FMT, 8>), grid, block, 0, st, a);
    else if (group == 16) hipLaunchKernelGGL((record_stft_hop<P, FMT, 16>), grid, block, 0, st, a);
    else if (group == 32) hipLaunchKernelGGL((record_stft_hop<P, FMT, 32>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((record_stft_hop<P, FMT, 64>), grid, block, 0, st, a);
}

// The hop and the band product run from the same work list, in one piece: frame_first [n + 1], pool_seg [n], lp [n], fi [n].
inline size_t hop_work_bytes(size_t n) { return (n + 1) * sizeof(int64_t) + n * sizeof(int64_t) + 2 * n * sizeof(int32_t); }
// `work` packed for the upload, and the kernel's arguments against product `p`, whose pools product_begin has made
template <class P>
StftHopArgs<P> hop_args(rt_handle *l, const IqProduct &p, int k, const StftHopWork &work, int64_t frames, std::vector<char> *packed) {
    const IqSlot &qs = l->riq->slot[l->riq->delivered];
    const size_t n = qs.first_seg.size(), b_first = (n + 1) * sizeof(int64_t), b_seg = n * sizeof(int64_t), b_i32 = n * sizeof(int32_t);
    packed->resize(hop_work_bytes(n));
    std::memcpy(packed->data(), work.frame_first.data(), b_first);
    std::memcpy(packed->data() + b_first, work.pool_seg.data(), b_seg);
    std::memcpy(packed->data() + b_first + b_seg, work.lp.data(), b_i32);
    std::memcpy(packed->data() + b_first + b_seg + b_i32, work.fi.data(), b_i32);
    StftHopArgs<P> a{};
    record_pool_args<P>(l, a);
    a.frame_first = reinterpret_cast<const int64_t *>(p.work);
    a.pool_seg = reinterpret_cast<const int64_t *>(p.work + b_first);
    a.lp = reinterpret_cast<const int32_t *>(p.work + b_first + b_seg);
    a.fi = reinterpret_cast<const int32_t *>(p.work + b_first + b_seg + b_i32);
    a.hop_div = k;
    a.n_frames = frames;
    a.pool_samples = qs.offsets.back();
    a.values = reinterpret_cast<typename stft_types<P>::C *>(p.out);
    return a;
}

// The frames of lane-less handle `l`'s delivered call at hop nperseg / k into its slot's kProdHop: once per delivered call and k.
template <class P>
int record_stft_hop_run(rt_handle *h, rt_handle *l, const char *entry, int k, int w, const StftHopWork &work, int64_t frames) {
    using C = typename stft_types<P>::C;
    RecordIq &q = *l->riq;
    IqSlot &qs = q.slot[q.delivered];
    IqProduct &p = qs.prod[kProdHop];
    if (p.holds(k, w)) return RT_OK;
    const int group = stft_hop_group(iq_nperseg(l), qs.bps);
    if (!record_pool_ok(qs, frames, (int64_t)kStftWaves * (64 / group))) return record_mismatch(h, entry);
    if (frames == 0) {
        p.set(k, w);
        return RT_OK;
    }
    RT_HIP(h, hipSetDevice(l->cfg.device));
    int rc = record_tables<P>(h, l, entry);
    if (rc != RT_OK) return rc;
    rc = product_begin(h, entry, p, (size_t)frames * sizeof(C), "the call's frames", hop_work_bytes(qs.first_seg.size()), "the work list");
    if (rc != RT_OK) return rc;
    std::vector<char> packed;
    const StftHopArgs<P> a = hop_args<P>(l, p, k, work, frames, &packed);
    return product_finish(h, q, entry, p, k, w, packed, "record_stft_hop", [&] {
        with_record_format(qs.fmt, [&](auto fmt) { launch_record_stft_hop<P, decltype(fmt)::value>(a, group, q.s_gather); });
    });
}

// ---- rt_fetch_record_band: the 2 w + 1 bins around each record's bin, frame by frame (rt_record_band.h) ----
template <class P, int FMT, int HW>
void launch_record_band_hw(const StftBandArgs<P> &a, int group, hipStream_t st) {
    const int64_t per_block = (int64_t)kStftWaves * (64 / group);
    const dim3 grid((unsigned)((a.hop.n_frames + per_block - 1) / per_block)), block(kStftBlock);
    const size_t lds = stft_band_lds_bytes(a.hop.nperseg, sizeof(typename stft_types<P>::C));
    if (group == 8) hipLaunchKernelGGL((record_band<P, FMT, 8, HW>), grid, block, lds, st, a);
    else if (group == 16) hipLaunchKernelGGL((record_band<P, FMT, 16, HW>), grid, block, lds, st, a);
    else if (group == 32) hipLaunchKernelGGL((record_band<P, FMT, 32, HW>), grid, block, lds, st, a);
    else hipLaunchKernelGGL((record_band<P, FMT, 64, HW>), grid, block, lds, st, a);
}
template <class P, int FMT>
void launch_record_band(const StftBandArgs<P> &a, int group, hipStream_t st) {
    const int hw = stft_band_bound(a.half_width);
    if (hw == 0) launch_record_band_hw<P, FMT, 0>(a, group, st);
    else if (hw == 2) launch_record_band_hw<P, FMT, 2>(a, group, st);
    else launch_record_band_hw<P, FMT, 8>(a, group, st);
}

// The band of lane-less handle `l`'s delivered call for (k, w) into its slot's kProdBand: once per delivered call and pair.  The
// frames and the work list are the hop entry's; the pools and the pair they hold are this product's own.
template <class P>
int record_band_run(rt_handle *h, rt_handle *l, const char *entry, int k, int w, const StftHopWork &work, int64_t frames) {
    using C = typename stft_types<P>::C;
    RecordIq &q = *l->riq;
    IqSlot &qs = q.slot[q.delivered];
    IqProduct &p = qs.prod[kProdBand];
    if (p.holds(k, w)) return RT_OK;
    const int group = stft_hop_group(iq_nperseg(l), qs.bps);
    const int64_t elems = stft_band_elems(frames, w);
    if (elems < 0 || !record_pool_ok(qs, frames, (int64_t)kStftWaves * (64 / group))) return record_mismatch(h, entry);
    if (frames == 0) {
        p.set(k, w);
        return RT_OK;
    }
    RT_HIP(h, hipSetDevice(l->cfg.device));
    int rc = record_tables<P>(h, l, entry);
    if (rc != RT_OK) return rc;
    rc = product_begin(h, entry, p, (size_t)((uint64_t)elems * sizeof(C)), "the call's band", hop_work_bytes(qs.first_seg.size()), "the work list");
    if (rc != RT_OK) return rc;
    std::vector<char> packed;
    StftBandArgs<P> b{};
    b.hop = hop_args<P>(l, p, k, work, frames, &packed);
    b.half_width = w;
    return product_finish(h, q, entry, p, k, w, packed, "record_band", [&] {
        with_record_format(qs.fmt, [&](auto fmt) { launch_record_band<P, decltype(fmt)::value>(b, group, q.s_gather); });
    });
}

// ---- rt_fetch_record_estimates: one row per record, reduced from the hop product's frames (rt_record_estimates.h) ----
// The rows of lane-less handle `l`'s delivered call for hop_div k into its slot's kProdEst: once per delivered call and k.  The hop
// product is made to hold k first (record_stft_hop_run: a no-op where it does); the frames stay on the device.  The rows are a
// product of their own: they stay valid when the hop product moves on to another k.
template <class P>
int record_estimates_run(rt_handle *h, rt_handle *l, const char *entry, int k, int w, const StftHopWork &hop, const EstimatesWork &work, int64_t frames) {
    using C = typename stft_types<P>::C;
    RecordIq &q = *l->riq;
    IqSlot &qs = q.slot[q.delivered];
    IqProduct &p = qs.prod[kProdEst];
    if (p.holds(k, w)) return RT_OK;
    const size_t n = qs.first_seg.size();
    if (n == 0) {
        p.set(k, w);
        return RT_OK;
    }
    if (n > (size_t)INT32_MAX) return record_mismatch(h, entry);  // (the kernel counts records in int32; the grid is a quarter of that)
    int rc = record_stft_hop_run<P>(h, l, entry, k, w, hop, frames);
    if (rc != RT_OK) return rc;
    RT_HIP(h, hipSetDevice(l->cfg.device));
    // the plan in one piece: the turn-back table, frame_first [n + 1], base [n][2], range [n][4], lp [n], fmod [n]
    const size_t b_first = (n + 1) * sizeof(int64_t), b_base = 2 * n * sizeof(int64_t), b_range = 4 * n * sizeof(int32_t), b_i32 = n * sizeof(int32_t);
    const size_t o_first = kEstTurnBytes, o_base = o_first + b_first, o_range = o_base + b_base, o_lp = o_range + b_range, o_fmod = o_lp + b_i32;
    const size_t work_bytes = o_fmod + b_i32;
    rc = product_begin(h, entry, p, n * sizeof(rt_record_estimate), "the call's estimates", work_bytes, "the estimates' plan");
    if (rc != RT_OK) return rc;
    std::vector<char> packed(work_bytes);
    static_assert(kEstTurnBytes >= 2 * kStftHopMaxDiv * (int)sizeof(double), "the turn-back table holds every hop_div");
    estimates_turn_table(k, reinterpret_cast<double *>(packed.data()));
    std::memcpy(packed.data() + o_first, work.frame_first.data(), b_first);
    std::memcpy(packed.data() + o_base, work.base.data(), b_base);
    std::memcpy(packed.data() + o_range, work.range.data(), b_range);
    std::memcpy(packed.data() + o_lp, work.lp.data(), b_i32);
    std::memcpy(packed.data() + o_fmod, work.fmod.data(), b_i32);
    EstimatesArgs<P> a{};
    a.values = reinterpret_cast<const C *>(qs.prod[kProdHop].out);
    a.turn = reinterpret_cast<const double *>(p.work);
    a.frame_first = reinterpret_cast<const int64_t *>(p.work + o_first);
    a.base = reinterpret_cast<const int64_t *>(p.work + o_base);
    a.range = reinterpret_cast<const int32_t *>(p.work + o_range);
    a.lp = reinterpret_cast<const int32_t *>(p.work + o_lp);
    a.fmod = reinterpret_cast<const int32_t *>(p.work + o_fmod);
    a.n_records = (int32_t)n;
    a.nperseg = iq_nperseg(l);
    a.hop_div = k;
    a.n_frames = frames;
    a.out = reinterpret_cast<rt_record_estimate *>(p.out);
    return product_finish(h, q, entry, p, k, w, packed, "record_estimates", [&] {
        hipLaunchKernelGGL((record_estimates<P>), dim3((unsigned)((n + kStftWaves - 1) / kStftWaves)), dim3(kStftBlock), 0, q.s_gather, a);
    });
}

// ---- rt_fetch_record_spectrum: one row per record and its column means and peaks, reduced from the band product (rt_record_spectrum.h) ----
template <class P>
void launch_record_spectrum(const SpectrumArgs<P> &a, hipStream_t st) {
    const dim3 grid((unsigned)(((size_t)a.n_records + kStftWaves - 1) / kStftWaves)), block(kStftBlock);
    const int hw = stft_band_bound(a.half_width);
    if (hw == 0) hipLaunchKernelGGL((record_spectrum<P, 0>), grid, block, 0, st, a);
    else if (hw == 2) hipLaunchKernelGGL((record_spectrum<P, 2>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((record_spectrum<P, 8>), grid, block, 0, st, a);
}

// The rows of lane-less handle `l`'s delivered call for (k, w) into its slot's kProdSpec: once per delivered call and pair.  The
// band product is made to hold (k, w) first (record_band_run: a no-op where it does); the frames stay on the device, and the rows
// stay valid when the band product moves on to another pair.
template <class P>
int record_spectrum_run(rt_handle *h, rt_handle *l, const char *entry, int k, int w, const StftHopWork &hop, const EstimatesWork &work, int64_t frames) {
    using C = typename stft_types<P>::C;
    RecordIq &q = *l->riq;
    IqSlot &qs = q.slot[q.delivered];
    IqProduct &p = qs.prod[kProdSpec];
    if (p.holds(k, w)) return RT_OK;
    const size_t n = qs.first_seg.size();
    if (n == 0) {
        p.set(k, w);
        return RT_OK;
    }
    if (n > (size_t)INT32_MAX) return record_mismatch(h, entry);  // (the kernel counts records in int32; the grid is a quarter of that)
    int rc = record_band_run<P>(h, l, entry, k, w, hop, frames);
    if (rc != RT_OK) return rc;
    RT_HIP(h, hipSetDevice(l->cfg.device));
    // the plan in one piece: frame_first [n + 1], range [n][4], lp [n]
    const size_t row_bytes = n * sizeof(rt_record_spectrum), col_bytes = n * (size_t)stft_band_columns(w) * sizeof(double);
    static_assert(sizeof(rt_record_spectrum) == 48, "the row pool's layout: rows of 48 bytes, then the means, then the peaks");
    const size_t b_first = (n + 1) * sizeof(int64_t), b_range = 4 * n * sizeof(int32_t), b_i32 = n * sizeof(int32_t);
    const size_t o_range = b_first, o_lp = o_range + b_range, work_bytes = o_lp + b_i32;
    rc = product_begin(h, entry, p, spectrum_pool_bytes(n, w), "the call's spectrum rows", work_bytes, "the spectrum's plan");
    if (rc != RT_OK) return rc;
    std::vector<char> packed(work_bytes);
    std::memcpy(packed.data(), work.frame_first.data(), b_first);
    std::memcpy(packed.data() + o_range, work.range.data(), b_range);
    std::memcpy(packed.data() + o_lp, work.lp.data(), b_i32);
    SpectrumArgs<P> a{};
    a.values = reinterpret_cast<const C *>(qs.prod[kProdBand].out);
    a.frame_first = reinterpret_cast<const int64_t *>(p.work);
    a.range = reinterpret_cast<const int32_t *>(p.work + o_range);
    a.lp = reinterpret_cast<const int32_t *>(p.work + o_lp);
    a.n_records = (int32_t)n;
    a.hop_div = k;
    a.half_width = w;
    a.n_frames = frames;
    a.rows = reinterpret_cast<rt_record_spectrum *>(p.out);
    a.mean = reinterpret_cast<double *>(p.out + row_bytes);
    a.peak = reinterpret_cast<double *>(p.out + row_bytes + col_bytes);
    return product_finish(h, q, entry, p, k, w, packed, "record_spectrum", [&] { launch_record_spectrum<P>(a, q.s_gather); });
}

// ---- the entries: refusals, the plan, the products, the delivery ----
// The plan of the delivered call for hop_div k: the lanes that hold it and each lane's frame list, before anything is launched or
// written.  kPlanRows: each lane's EstimatesWork too.  kPlanSegments: the k = 1 entry, whose frames are the delivered segments --
// they are counted and no list is made (record_stft_run).  `band_w` >= 0: the frames are a band's, 2 band_w + 1 values each.
enum { kPlanSegments, kPlanFrames, kPlanRows };
struct RecordPlan {
    std::vector<rt_handle *> lanes;
    std::vector<StftHopWork> hops;    // [lanes]
    std::vector<EstimatesWork> rows;  // [lanes] where wanted
    std::vector<int64_t> frames;      // [lanes]
    size_t records = 0, total = 0;    // records and frames over all lanes
    IqSlot &slot(size_t i) const { return lanes[i]->riq->slot[lanes[i]->riq->delivered]; }
};
int record_plan(rt_handle *h, const char *entry, int what, int k, int band_w, const int64_t *offsets, size_t n_offsets, const int32_t *first_seg,
                size_t n_first, RecordPlan *p) {
    const bool want_rows = what == kPlanRows;
    size_t samples = 0;
    int bps = 0;
    const int rc = iq_delivered_call(h, entry, &p->lanes, &p->records, &samples, &bps);
    if (rc != RT_OK) return rc;
    if ((offsets && n_offsets != p->records + 1) || (first_seg && n_first != p->records))
        return record_refuse(h, entry, "n_offsets must be the number of records the last rt_fetch delivered plus one, n_first that number");
    const int N = iq_nperseg(h);
    p->hops.resize(p->lanes.size());
    p->rows.resize(want_rows ? p->lanes.size() : 0);
    p->frames.resize(p->lanes.size());
    for (size_t i = 0; i < p->lanes.size(); ++i) {
        const IqSlot &qs = p->slot(i);
        const size_t n = qs.first_seg.size();
        const bool sized = qs.fi.size() == n && (!want_rows || (qs.start.size() == n && qs.end.size() == n));
        int64_t f = what == kPlanSegments ? qs.offsets.back() / N
                    : sized               ? stft_hop_build_work(qs.offsets.data(), qs.first_seg.data(), qs.fi.data(), n, N, k, &p->hops[i])
                                          : -1;
        // (both builders agree on the frame count)
        if (want_rows && f >= 0 &&
            estimates_build_work(qs.offsets.data(), qs.first_seg.data(), qs.fi.data(), qs.start.data(), qs.end.data(), n, N, k, &p->rows[i]) != f)
            f = -1;
        if (f < 0 || (band_w >= 0 && stft_band_elems(f, band_w) < 0)) return record_mismatch(h, entry);
        p->frames[i] = f;
        p->total += (size_t)f;
    }
    return RT_OK;
}
// the (k, w) rule of an entry: the band and spectrum entries', or the hop's alone
inline std::string record_rule(rt_handle *h, bool band, int k, int w) {
    return band ? spectrum_refusal(iq_nperseg(h), k, w) : stft_hop_refusal(iq_nperseg(h), k);
}

// rt_fetch_record_stft (k = 1), _stft_hop and _band (`band`; w = 0 otherwise) and their _f64 twins: `run` makes product `prod` of a
// lane hold (k, w), and a frame is 2 w + 1 values.
using RecordFramesRun = int (*)(rt_handle *, rt_handle *, const char *, int, int, const StftHopWork &, int64_t);
template <class P>
int fetch_record_frames(rt_handle *h, const char *entry, const char *twin, int prod, RecordFramesRun run, bool band, int k, int w, int64_t *offsets,
                        size_t n_offsets, int32_t *first_seg, size_t n_first, P *values, size_t cap_frames, size_t *n_frames) {
    if (!h || !n_frames) return RT_E_INVALID;
    *n_frames = 0;
    if ((h->f64 != nullptr) != (sizeof(P) == 8)) {
        h->err = std::string(entry) + (h->f64 ? " on a float64 handle (rt_create_f64): use " : " on a float32 handle (rt_create): use ") + twin;
        return RT_E_INVALID;
    }
    const std::string why = record_rule(h, band, k, w);
    if (!why.empty()) return record_refuse(h, entry, why);
    RecordPlan plan;
    const bool segments = prod == kProdStft;
    const int N = iq_nperseg(h);
    const int rc = record_plan(h, entry, segments ? kPlanSegments : kPlanFrames, k, band ? w : -1, offsets, n_offsets, first_seg, n_first, &plan);
    if (rc != RT_OK) return rc;
    *n_frames = plan.total;
    const bool query = !values || cap_frames == 0;
    if (!query && cap_frames < plan.total) return record_refuse(h, entry, "output buffer too small", RT_E_CAPACITY);
    if (!query)
        for (size_t i = 0; i < plan.lanes.size(); ++i) {
            const int rs = run(h, plan.lanes[i], entry, k, w, plan.hops[i], plan.frames[i]);
            if (rs != RT_OK) return rs;
        }
    const size_t frame_bytes = (size_t)stft_band_columns(w) * sizeof(typename stft_types<P>::C);
    size_t r0 = 0, c0 = 0;
    if (offsets) offsets[0] = 0;
    for (size_t i = 0; i < plan.lanes.size(); ++i) {
        rt_handle *l = plan.lanes[i];
        const IqSlot &qs = plan.slot(i);
        const size_t n = qs.first_seg.size(), mine = (size_t)plan.frames[i];
        if (offsets)
            for (size_t r = 0; r < n; ++r) offsets[r0 + r + 1] = (int64_t)c0 + (segments ? qs.offsets[r + 1] / N : plan.hops[i].frame_first[r + 1]);
        if (first_seg && n) std::memcpy(first_seg + r0, qs.first_seg.data(), n * sizeof(int32_t));
        if (!query && mine) {
            RT_HIP(h, hipSetDevice(l->cfg.device));
            RT_HIP(h, hipMemcpy(reinterpret_cast<char *>(values) + c0 * frame_bytes, qs.prod[prod].out, mine * frame_bytes, hipMemcpyDeviceToHost));
        }
        r0 += n;
        c0 += mine;
    }
    return RT_OK;
}

// rt_fetch_record_estimates and _spectrum (`band`; w = 0 otherwise): `run32` / `run64` makes product `prod` of a float32 / float64
// lane hold (k, w); copy(pool, r0, n) hands out a lane's n rows, the caller's rows r0 on, from the product's output pool.
using RecordRowsRun = int (*)(rt_handle *, rt_handle *, const char *, int, int, const StftHopWork &, const EstimatesWork &, int64_t);
template <class Copy>
int fetch_record_rows(rt_handle *h, const char *entry, int prod, RecordRowsRun run32, RecordRowsRun run64, bool band, int k, int w, bool query, size_t cap,
                      size_t *n_out, Copy copy) {
    if (!h || !n_out) return RT_E_INVALID;
    *n_out = 0;
    const std::string why = record_rule(h, band, k, w);
    if (!why.empty()) return record_refuse(h, entry, why);
    RecordPlan plan;
    const int rc = record_plan(h, entry, kPlanRows, k, band ? w : -1, nullptr, 0, nullptr, 0, &plan);
    if (rc != RT_OK) return rc;
    *n_out = plan.records;
    if (query) return RT_OK;
    if (cap < plan.records) return record_refuse(h, entry, "output buffer too small", RT_E_CAPACITY);
    for (size_t i = 0; i < plan.lanes.size(); ++i) {
        const int rs = (plan.lanes[i]->f64 ? run64 : run32)(h, plan.lanes[i], entry, k, w, plan.hops[i], plan.rows[i], plan.frames[i]);
        if (rs != RT_OK) return rs;
    }
    size_t r0 = 0;
    for (size_t i = 0; i < plan.lanes.size(); ++i) {
        const size_t n = plan.slot(i).first_seg.size();
        if (n) {
            RT_HIP(h, hipSetDevice(plan.lanes[i]->cfg.device));
            RT_HIP(h, copy(plan.slot(i).prod[prod].out, r0, n));
        }
        r0 += n;
    }
    return RT_OK;
}

// ---- rt_set_input_stats: the call's rows, at enqueue (rt_input_stats.h) ----
// On the scan's stream, in front of the scan, where the call's IQ is in place (the staged copy of the _host entries included) and
// the call's presence rows are on the device.  `d_absent`: row kMaskAbsent of the call's mask, or null.  The slot's rows are no
// call's from here on; the caller marks them the new call's once the whole call is enqueued.
template <int FMT>
void launch_input_stats(const InputStatsArgs &a, hipStream_t st) {
    hipLaunchKernelGGL((input_stats<FMT>), dim3((unsigned)a.n_streams * (unsigned)a.n_chunks), dim3(kInputStatsBlock), 0, st, a);
}
int enqueue_input_stats(rt_handle *h, int idx, const void *iq, int64_t n_samples, int64_t stream_stride, int fmt, const int32_t *d_absent) {
    InputStatsState &q = *h->ist;
    InputStatsSlot &qs = q.slot[idx];
    qs.seq = 0;
    const int kfmt = (h->f64 && fmt == kFmtC64) ? kStatsC128 : fmt;
    static_assert(kStatsC64 == kFmtC64 && kStatsU8 == kFmtU8 && kStatsI16 == kFmtI16 && kStatsI8 == kFmtI8, "one numbering of the input formats");
    InputStatsArgs a{};
    a.iq = static_cast<const char *>(iq);
    a.stream_stride = stream_stride;
    a.n_samples = n_samples;
    a.n_streams = h->cfg.n_streams;
    a.n_chunks = (int32_t)((n_samples + kInputStatsChunk - 1) / kInputStatsChunk);
    a.absent = d_absent;
    a.parts = qs.d_parts;
    a.rows = qs.h_rows;
    if (a.n_chunks > q.max_chunks || (int64_t)a.n_streams * a.n_chunks > 0x7FFFFFFFll) {
        h->err = "input_stats: internal: more chunks than rt_config.max_samples holds";
        return RT_E_HIP;
    }
    if (a.n_chunks > 0) {
        switch (kfmt) {
        case kStatsC64: launch_input_stats<kStatsC64>(a, h->s_scan); break;
        case kStatsU8: launch_input_stats<kStatsU8>(a, h->s_scan); break;
        case kStatsI16: launch_input_stats<kStatsI16>(a, h->s_scan); break;
        case kStatsI8: launch_input_stats<kStatsI8>(a, h->s_scan); break;
        default: launch_input_stats<kStatsC128>(a, h->s_scan); break;
        }
    }
    const dim3 grid((unsigned)((a.n_streams + kInputStatsBlock - 1) / kInputStatsBlock));
    if (stats_is_float(kfmt)) hipLaunchKernelGGL((input_stats_fold<double>), grid, dim3(kInputStatsBlock), 0, h->s_scan, a, kfmt);
    else hipLaunchKernelGGL((input_stats_fold<int64_t>), grid, dim3(kInputStatsBlock), 0, h->s_scan, a, kfmt);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        h->err = std::string("input_stats: ") + hipGetErrorString(e);
        return RT_E_HIP;
    }
    return RT_OK;
}
void input_stats_free(rt_handle *h) {
    if (!h->ist) return;
    for (InputStatsSlot &qs : h->ist->slot) {
        (void)hipFree(qs.d_parts);
        (void)hipHostFree(qs.h_rows);
    }
    delete h->ist;
    h->ist = nullptr;
}

int claim_slot(rt_handle *h, Slot **out, CallCtx *saved) {
    Slot &sl = h->slot[h->n_calls % kSlots];
    // the slot's previous call may still be in its detection (a stream of its own): what is enqueued from here on waits for it
    if (sl.call.seq != 0 && h->s_detect != h->s_scan) (void)hipStreamWaitEvent(h->s_scan, sl.ev_done, 0);
    if (sl.pool_cap < h->pool_want && !sl.call.pending) {
        // the other slot's pool had to grow: this one follows before its next call needs it (best effort)
        if (sl.call.seq == 0 || hipEventSynchronize(sl.ev_done) == hipSuccess) (void)grow_pool(h, sl, h->pool_want);
    }
    if (sl.d_cells && sl.cell_cap < h->cells_want && !sl.call.pending) {  // (the cell pool likewise)
        if (sl.call.seq == 0 || hipEventSynchronize(sl.ev_done) == hipSuccess) (void)grow_cells(h, sl.d_cells, sl.cell_cap, h->cells_want);
    }
    *saved = sl.call;  // put back if the new call fails before it has launched anything
    std::swap(sl.lc, h->lc_saved);  // (... with the ledger's snapshot of it: process_impl swaps it back)
    sl.lc.clear();
    sl.call = CallCtx{};
    sl.call.seq = h->n_calls + 1;
    *out = &sl;
    return RT_OK;
}

// What the call in `sl` took from the handle's host bookkeeping when it was enqueued goes back (its enqueue failed: process_impl; a
// later lane's did: rollback_newest): AUTO's probe counter, the slot of the chunk minima, and all the ledger gave it -- the
// rotation, the segment counts, the stream resets it consumed, the presence, chain and record-IQ books.
void undo_call_books(rt_handle *h, Slot &sl) {
    const CallCtx &c = sl.call;
    h->ap.restore(c.prev_auto);
    h->minsum_slot = c.prev_minsum_slot;  // (the chunk minima of the dropped buffer must not set the next call's thresholds)
    h->ledger.rollback(sl.lc);
}

// Undo the newest enqueued call of a (lane-less) handle: wait for its kernels, forget it, and put the
// look-back bookkeeping back to what it was before the call.
void rollback_newest(rt_handle *h) {
    Slot *best = nullptr;
    for (auto &sl : h->slot)
        if (sl.call.pending && (!best || sl.call.seq > best->call.seq)) best = &sl;
    if (!best || best->call.seq != h->n_calls) return;
    (void)hipSetDevice(h->cfg.device);
    (void)hipEventSynchronize(best->ev_done);
    const CallCtx &c = best->call;
    if (!c.is_extract) {
        undo_call_books(h, *best);
        if (best->min_seq == c.seq) best->min_items = 0;  // (the dropped buffer's chunk minima must not stand in for the slot's older ones, which they have overwritten)
    }
    best->call = CallCtx{};
    h->n_calls--;
}

Slot *oldest_pending(rt_handle *h) {
    Slot *best = nullptr;
    for (auto &sl : h->slot)
        if (sl.call.pending && (!best || sl.call.seq < best->call.seq)) best = &sl;
    return best;
}

// rt_fetch_row_means: the row means of the call just delivered are the ones to hand out (an rt_extract has none) ...
void keep_row_means(rt_handle *h, const Slot &sl) { h->rm_slot = sl.call.is_extract ? kRowMeansExtract : (int)(&sl - h->slot); }

// ... until the next rt_process*, rt_extract or rt_reset (in every lane: a lane that fails to enqueue leaves none behind either)
void forget_row_means(rt_handle *h) {
    h->rm_slot = kRowMeansNone;
    if (h->f64) h->f64->rm_slot = kRowMeansNone;
    if (h->riq) h->riq->delivered = kIqNone;  // (rt_fetch_record_iq: the same validity)
    for (rt_handle *k : h->kids) forget_row_means(k);
}

// forward one call to every lane; `call(kid, first stream of the kid)`; the first failure is reported.
// `enqueues`: the call enqueues work (rt_process*, rt_extract) -- when lane k fails, the lanes before it
// are rolled back, so that no lane holds a pending call the others lack (FIFO fetches pair calls by position).
template <class F>
int for_each_lane(rt_handle *h, F call, bool enqueues = false) {
    if (enqueues) {
        // The slot every lane is about to claim may still hold a call that was never fetched (a third rt_process without
        // an rt_fetch): it is dropped HERE, in all lanes, before any of them starts -- if a later lane then fails, the
        // lanes before it roll their new call back and all of them are left with the same pending calls (a lane that
        // failed before its first launch used to put the old call back while the others had lost it).
        for (rt_handle *k : h->kids) {
            Slot &sl = k->slot[k->n_calls % kSlots];
            if (sl.call.pending) {
                (void)hipSetDevice(k->cfg.device);
                (void)hipEventSynchronize(sl.ev_done);
                sl.call.pending = false;
            }
        }
    }
    // test hook of the DIAGNOSTIC build (librt_analyze_diag.so; tests/test_gpu_parity.py, fault injection): a handle created under
    // RT_TEST_FAIL_LANE=<k>:<n> has its lane k refuse the handle's n-th enqueue, as a device allocation failure inside that lane
    // would.  The product build never reads the environment (rt_diag.h): test_fail_lane stays -1 there.
    int fail_lane = -1;
#ifdef RT_DIAG
    if (enqueues && h->test_fail_lane >= 0 && ++h->test_enqueues == (uint64_t)h->test_fail_nth) fail_lane = h->test_fail_lane;
#endif
    for (size_t k = 0; k < h->kids.size(); ++k) {
        int rc;
        if ((int)k == fail_lane) {
            h->kids[k]->err = "injected failure";
            rc = RT_E_NOMEM;
        } else {
            rc = call(h->kids[k], (int64_t)h->kid_base[k]);
        }
        if (rc != RT_OK) {
            h->err = h->kids[k]->err;
            if (enqueues)
                for (size_t j = 0; j < k; ++j) rollback_newest(h->kids[j]);
            return rc;
        }
    }
    return RT_OK;
}

}  // namespace

// rt_set_stream_settings[_f64]: the arrays against the rules of the header, before anything is copied or launched.
template <class P>
static int check_stream_settings(rt_handle *h, const char *what, const P *snr, const double *min_d, const double *max_d) {
    for (int s = 0; s < h->cfg.n_streams; ++s) {
        const std::string who = std::string(what) + ": stream " + std::to_string(s) + ": ";
        if (snr && !(snr[s] > (P)0 && std::isfinite(snr[s]))) {
            h->err = who + "snr_threshold must be positive and finite";
            return RT_E_INVALID;
        }
        if (min_d && !std::isfinite(min_d[s])) {
            h->err = who + "min_duration_s is not finite";
            return RT_E_INVALID;
        }
        if (max_d && !std::isfinite(max_d[s])) {
            h->err = who + "max_duration_s is not finite";
            return RT_E_INVALID;
        }
        if (min_d && min_d[s] < h->cfg.min_duration_s) {
            h->err = who + "min_duration_s " + std::to_string(min_d[s]) + " is under the handle's (rt_config.min_duration_s " + std::to_string(h->cfg.min_duration_s) + ")";
            return RT_E_INVALID;
        }
        if (max_d && max_d[s] > h->cfg.max_duration_s) {
            h->err = who + "max_duration_s " + std::to_string(max_d[s]) + " is over the handle's (rt_config.max_duration_s " + std::to_string(h->cfg.max_duration_s) + ")";
            return RT_E_INVALID;
        }
    }
    return RT_OK;
}

// rt_set_chain: the streams of a run are buffers of ONE analyzer, so per-stream values must not differ inside a run (the sparse
// scans write a look-back cell iff the later cells pass the WRITING stream's threshold: a reader with a lower one could walk onto
// a cell that was never stored).  Each array [S] or null (= the handle's one value for every stream).
static int chain_runs_uniform(rt_handle *h, const ChainBook &book, const char *what, const float *thr, const float *cal, const float *snr,
                              const double *min_d, const double *max_d) {
    if (!book.on()) return RT_OK;
    const char *name = nullptr;
    int r = -1;
    auto look = [&](int run, const char *n) {
        if (r < 0 && run >= 0) {
            r = run;
            name = n;
        }
    };
    if (thr) look(book.first_mixed_run(thr), "threshold");
    if (cal) look(book.first_mixed_run(cal), "calibration_db");
    if (snr) look(book.first_mixed_run(snr), "snr_threshold");
    if (min_d) look(book.first_mixed_run(min_d), "min_duration_s");
    if (max_d) look(book.first_mixed_run(max_d), "max_duration_s");
    if (r < 0) return RT_OK;
    h->err = std::string(what) + ": run " + std::to_string(r) + " (streams " + std::to_string(r * book.links) + " ... " +
             std::to_string((r + 1) * book.links - 1) + "): " + name + " differs inside the run; the streams of a chained run are buffers of one recording";
    return RT_E_INVALID;
}

// ... and the table itself: `cur` becomes the new settings (empty: all three arrays null), `changed[s]` says whether stream s's differ from before
template <class P>
static void build_stream_settings(const rt_config &cfg, int N, P cfg_snr, const P *snr, const double *min_d, const double *max_d,
                                  std::vector<StreamSettingsT<P>> &cur, std::vector<uint8_t> &changed) {
    const int S = cfg.n_streams;
    StreamSettingsT<P> dflt{};
    dflt.snr = cfg_snr;
    dflt.min_d = cfg.min_duration_s;
    dflt.max_d = cfg.max_duration_s;
    std::vector<StreamSettingsT<P>> next;
    if (snr || min_d || max_d) next.resize((size_t)S);
    changed.assign((size_t)S, 0);
    for (int s = 0; s < S; ++s) {
        const StreamSettingsT<P> was = cur.empty() ? dflt : cur[(size_t)s];
        StreamSettingsT<P> is = dflt;
        if (snr) is.snr = snr[s];
        if (min_d) is.min_d = min_d[s];
        if (max_d) is.max_d = max_d[s];
        is.stride = probe_stride(N, cfg.sample_rate, is.min_d);
        if (!(was.snr == is.snr && was.min_d == is.min_d && was.max_d == is.max_d)) changed[(size_t)s] = 1;
        if (!next.empty()) next[(size_t)s] = is;
    }
    cur.swap(next);
}

// rt_set_stream_params[_f64] of one lane-less handle, on the power type P: `cfg_thr` = the handle's one threshold, `h_thr_s` / `d_thr_s` /
// `d_cal_s` its per-stream arrays, `h_cal_s` (or null) the host copy of the calibration a chained handle checks.
template <class P>
static int set_stream_params_one(rt_handle *h, P cfg_thr, std::vector<P> &h_thr_s, std::vector<P> *h_cal_s, P *&d_thr_s, P *&d_cal_s, const P *threshold,
                                 const P *calibration_db) {
    RT_HIP(h, hipSetDevice(h->cfg.device));
    // kernels in flight read the arrays: let them finish first (a configuration call, not on the hot path)
    RT_HIP(h, hipStreamSynchronize(h->s_scan));
    RT_HIP(h, hipStreamSynchronize(h->s_detect));
    const int S = h->cfg.n_streams;
    const size_t bytes = (size_t)S * sizeof(P);
    auto put = [&](P *&dst, const P *src) -> int {
        if (!src) {
            if (dst) (void)hipFree(dst);
            dst = nullptr;
            return RT_OK;
        }
        if (!dst) RT_HIP(h, hipMalloc(&dst, bytes));
        RT_HIP(h, hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
        return RT_OK;
    };
    // A stream whose threshold changes starts without look-back: the reference fixes the threshold when a SignalAnalyzer is
    // built (analyze.py:115), a new one needs a new analyzer (_spectrogram_last = None) -- and the sparse scans keep only
    // those tail cells a walk with the threshold of their own call can reach (rt_kernels.h: sparse tail).
    std::vector<uint8_t> changed((size_t)S, (uint8_t)0);
    for (int s = 0; s < S; ++s) {
        const P was = h_thr_s.empty() ? cfg_thr : h_thr_s[(size_t)s];
        const P is = threshold ? threshold[s] : cfg_thr;
        changed[(size_t)s] = !(was == is);
    }
    h->ledger.mark_changed(changed);
    if (threshold) h_thr_s.assign(threshold, threshold + S); else h_thr_s.clear();
    if (h_cal_s) {
        if (calibration_db) h_cal_s->assign(calibration_db, calibration_db + S); else h_cal_s->clear();
    }
    const int rc = put(d_thr_s, threshold);
    if (rc != RT_OK) return rc;
    return put(d_cal_s, calibration_db);
}

// rt_set_stream_settings[_f64] of one lane-less handle, on the power type P: `h_set_s` / `d_set_s` its table, `cfg_snr` the handle's one value
template <class P>
static int set_stream_settings_one(rt_handle *h, P cfg_snr, std::vector<StreamSettingsT<P>> &h_set_s, StreamSettingsT<P> *&d_set_s, const P *snr,
                                   const double *min_d, const double *max_d) {
    RT_HIP(h, hipSetDevice(h->cfg.device));
    // kernels in flight read the table: let them finish first (a configuration call, not on the hot path)
    RT_HIP(h, hipStreamSynchronize(h->s_scan));
    RT_HIP(h, hipStreamSynchronize(h->s_detect));
    const size_t bytes = (size_t)h->cfg.n_streams * sizeof(StreamSettingsT<P>);
    if ((snr || min_d || max_d) && !d_set_s) RT_HIP(h, hipMalloc(&d_set_s, bytes));
    // A stream whose settings change starts without look-back, as after rt_reset_stream: in the reference they are fixed when the
    // SignalAnalyzer is built (analyze.py:113-116), new ones mean a new analyzer (_spectrogram_last = None, analyze.py:128).
    std::vector<uint8_t> changed;
    build_stream_settings<P>(h->cfg, iq_nperseg(h), cfg_snr, snr, min_d, max_d, h_set_s, changed);
    h->ledger.mark_changed(changed);
    if (h_set_s.empty()) {
        if (d_set_s) (void)hipFree(d_set_s);
        d_set_s = nullptr;
        return RT_OK;
    }
    RT_HIP(h, hipMemcpy(d_set_s, h_set_s.data(), bytes, hipMemcpyHostToDevice));
    return RT_OK;
}

extern "C" {

int rt_abi_version(void) { return RT_ABI_VERSION; }

int rt_device_count(int *count) {
    if (!count) return RT_E_INVALID;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        g_create_error = std::string("hipGetDeviceCount: ") + hipGetErrorString(e);
        return RT_E_NO_DEVICE;
    }
    *count = n;
    return RT_OK;
}

const char *rt_last_error(rt_handle *h) { return h ? h->err.c_str() : g_create_error.c_str(); }

static void destroy_f64(rt_handle *h);

void rt_destroy(rt_handle *h) {
    if (!h) return;
    if (h->f64) {
        destroy_f64(h);
        return;
    }
    if (!h->kids.empty()) {
        for (rt_handle *k : h->kids) rt_destroy(k);
        delete h;
        return;
    }
    (void)hipSetDevice(h->cfg.device);
    (void)hipDeviceSynchronize();
    iq_free(h);
    input_stats_free(h);
    (void)hipFree(h->d_work);
    (void)hipFree(h->d_twg);
    (void)hipFree(h->d_cwin);
    (void)hipFree(h->d_bfilt);
    (void)hipFree(h->d_window);
    (void)hipFree(h->d_window_t);
    (void)hipFree(h->d_sub_first);
    (void)hipHostFree(h->h_sub_list);
    (void)hipFree(h->d_tw1);
    (void)hipFree(h->d_tw2);
    for (auto &t : h->d_tail) (void)hipFree(t);
    (void)hipFree(h->d_spec);
    (void)hipFree(h->d_spec_part);
    for (auto &st : h->d_iq_stage) (void)hipFree(st);
    (void)hipFree(h->d_thr_s);
    (void)hipFree(h->d_cal_s);
    (void)hipFree(h->d_set_s);
    for (auto &sl : h->slot) {
        (void)hipFree(sl.d_hot);
        (void)hipFree(sl.d_hot_count);
        (void)hipFree(sl.d_hot_seen);
        (void)hipFree(sl.d_items);
        (void)hipHostFree(sl.h_hot_total);
        (void)hipFree(sl.d_psum);
        (void)hipFree(sl.d_full);
        (void)hipFree(sl.d_cell_hot);
        (void)hipFree(sl.d_cell_need);
        (void)hipFree(sl.d_chunk_min);
        (void)hipFree(sl.d_thr_bin);
        (void)hipFree(sl.d_thr_nat);
        (void)hipFree(sl.d_abs_hot);
        (void)hipHostFree(sl.h_abs_hot);
        (void)hipFree(sl.d_seg_list);
        (void)hipHostFree(sl.h_seg_total);
        (void)hipFree(sl.d_raw);
        (void)hipFree(sl.d_raw_count);
        (void)hipFree(sl.d_counters);
        (void)hipHostFree(sl.h_counters);
        (void)hipHostFree(sl.h_rec_offset);
        (void)hipHostFree(sl.h_rec_count);
        (void)hipHostFree(sl.h_records);
        (void)hipHostFree(sl.h_no_last);
        (void)hipHostFree(sl.h_mask);
        (void)hipFree(sl.d_mask);
        (void)hipHostFree(sl.h_chain_rows);
        (void)hipFree(sl.d_chain_rows);
        (void)hipFree(sl.d_chain);
        (void)hipHostFree(sl.h_overflow);
        (void)hipHostFree(sl.h_incons);
        (void)hipHostFree(sl.h_dc_flag);
        (void)hipHostFree(sl.h_list);
        (void)hipHostFree(sl.h_total);
        (void)hipFree(sl.d_row_means);
        (void)hipFree(sl.d_cells);
        (void)hipFree(sl.d_hot_kept);
        (void)hipFree(sl.d_stream_cells);
        (void)hipFree(sl.d_stream_base);
        (void)hipHostFree(sl.h_cells_info);
        if (sl.ev_begin) (void)hipEventDestroy(sl.ev_begin);
        if (sl.ev_first) (void)hipEventDestroy(sl.ev_first);
        if (sl.ev_scan) (void)hipEventDestroy(sl.ev_scan);
        if (sl.ev_done) (void)hipEventDestroy(sl.ev_done);
    }
    if (h->own_scan_stream && h->s_detect && h->s_detect != h->s_scan) (void)hipStreamDestroy(h->s_detect);
    if (h->own_scan_stream && h->s_scan) (void)hipStreamDestroy(h->s_scan);
    delete h;
}

int rt_create(const rt_config *cfg, rt_handle **out) {
    if (!cfg || !out) return fail_create(RT_E_INVALID, "null argument");
    *out = nullptr;
#ifdef RT_DIAG
    warn_unknown_switches();
#endif
    if (cfg->n_streams < 1 || cfg->max_samples < 0 || !cfg->window || !(cfg->sample_rate > 0))
        return fail_create(RT_E_INVALID, "n_streams, max_samples, window and sample_rate must be set");
    if (!(cfg->max_duration_s >= 0) || !(cfg->min_duration_s >= 0))
        return fail_create(RT_E_INVALID, "durations must be non-negative");
    const ScanFamily fam = scan_family(cfg->nperseg);  // which kernels run this size (rt_core.h)
    if (!fam.supported)
        return fail_create(RT_E_UNSUPPORTED, "fft_nperseg " + std::to_string(cfg->nperseg) + " is not supported: 8 ... 8192, or a power of two up to 16384 (the powers of two from 32 "
                                             "on run the fused scan kernels, every other size a general transform on the dense path)");
    const int R3 = fam.R3, QS = fam.QS, big = fam.big;
    const bool general = fam.general, bluestein = fam.bluestein;
    if (cfg->mode < RT_MODE_AUTO || cfg->mode > RT_MODE_RUNFILTER) return fail_create(RT_E_INVALID, "bad mode");
    if (cfg->flags & RT_FLAG_F64_SPARSE) return fail_create(RT_E_INVALID, "RT_FLAG_F64_SPARSE is a flag of float64 handles (rt_create_f64)");
    if (cfg->flags & RT_FLAG_F64_RESCUE) return fail_create(RT_E_INVALID, "RT_FLAG_F64_RESCUE is a flag of float64 handles (rt_create_f64)");
    if (general && cfg->mode != RT_MODE_AUTO && cfg->mode != RT_MODE_DENSE)
        return fail_create(RT_E_UNSUPPORTED, "fft_nperseg " + std::to_string(cfg->nperseg) + " runs on the dense path only: mode must be RT_MODE_AUTO or RT_MODE_DENSE");
    if (big && (cfg->mode == RT_MODE_PREFILTER || cfg->mode == RT_MODE_RUNFILTER))
        return fail_create(RT_E_UNSUPPORTED, "fft_nperseg " + std::to_string(cfg->nperseg) + " has the sparse and the dense path only: mode must be RT_MODE_AUTO, RT_MODE_SPARSE or RT_MODE_DENSE");
    if (cfg->lanes > 1 && cfg->n_streams > 1) {
        // stream groups on their own handles and HIP streams: the detection kernels, launch gaps and last
        // workgroup round of one group overlap the scan of another
        if (cfg->hip_stream) return fail_create(RT_E_INVALID, "lanes > 1 run on their own HIP streams: hip_stream must be NULL");
        const int lanes = cfg->lanes < cfg->n_streams ? cfg->lanes : cfg->n_streams;
        rt_handle *p = new (std::nothrow) rt_handle();
        if (!p) return fail_create(RT_E_NOMEM, "out of host memory");
        p->cfg = *cfg;
        if (const char *spec = RT_DIAG_ENV("RT_TEST_FAIL_LANE")) {  // (diagnostic builds only: rt_diag.h)
            int lane = -1, nth = 0;
            if (std::sscanf(spec, "%d:%d", &lane, &nth) == 2 && lane >= 0 && nth > 0) {
                p->test_fail_lane = lane;
                p->test_fail_nth = nth;
            }
        }
        for (int k = 0; k <= lanes; ++k) p->kid_base.push_back((int)((int64_t)cfg->n_streams * k / lanes));
        for (int k = 0; k < lanes; ++k) {
            rt_config kc = *cfg;
            kc.lanes = 1;
            kc.segs_per_chunk = choose_chunk(*cfg, fam, cfg->n_streams, (int)(cfg->max_samples / cfg->nperseg));  // the whole batch's choice
            kc.n_streams = p->kid_base[(size_t)k + 1] - p->kid_base[(size_t)k];
            // (detection by groups of buckets is decided by the whole batch: the lanes' launches run side by side)
            if (cfg->n_streams >= 1024) kc.flags |= (int32_t)kFlagLaneOfLargeBatch;
            rt_handle *kid = nullptr;
            g_creating_lane = true;
            const int rc = rt_create(&kc, &kid);
            g_creating_lane = false;
            if (rc != RT_OK) {
                if (p->kids.empty()) delete p; else rt_destroy(p);
                return rc;  // g_create_error was set by the failing rt_create
            }
            p->kids.push_back(kid);
        }
        *out = p;
        return RT_OK;
    }

    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev < 1)
        return fail_create(RT_E_NO_DEVICE, std::string("no HIP device: ") + (e != hipSuccess ? hipGetErrorString(e) : "count 0"));
    if (cfg->device < 0 || cfg->device >= ndev) return fail_create(RT_E_INVALID, "device ordinal out of range");
    e = hipSetDevice(cfg->device);
    if (e != hipSuccess) return fail_create(RT_E_NO_DEVICE, std::string("hipSetDevice: ") + hipGetErrorString(e));

    rt_handle *h = new (std::nothrow) rt_handle();
    if (!h) return fail_create(RT_E_NOMEM, "out of host memory");
    h->cfg = *cfg;
    h->cfg.window = nullptr;
    h->h_window.assign(cfg->window, cfg->window + cfg->nperseg);
    h->R3 = R3;
    h->big = big;
    h->QS = QS;
    h->general = general;
    if (general) {
        h->cfg.mode = RT_MODE_DENSE;
        h->bluestein = bluestein;
        h->gen_m = 1;
        while (h->gen_m < (bluestein ? 2 * cfg->nperseg - 1 : cfg->nperseg)) h->gen_m <<= 1;
        h->log2n = 0;
        while ((1 << h->log2n) < h->gen_m) ++h->log2n;
    }
    h->N = cfg->nperseg;
    h->LG = QS ? QS : 16 * R3;
    h->GPW = big ? 1 : scan_block(R3) / h->LG;  // (stft_wg: a chunk per workgroup)
    h->timing = (cfg->flags & RT_FLAG_TIMING) != 0;
    h->rec_cap = cfg->record_capacity > 0 ? cfg->record_capacity : 1024;
    h->stride = probe_stride(h->N, cfg->sample_rate, cfg->min_duration_s);
    h->K = tail_cols(h->N, cfg->sample_rate, cfg->max_duration_s);
    h->max_seg = (int)(cfg->max_samples / h->N);
    h->L = choose_chunk(*cfg, fam, cfg->n_streams, h->max_seg);  // fixed per handle so the scratch bound holds for every call
    h->max_chunks = std::max(1, (h->max_seg + h->L - 1) / h->L);
    int max_blocks_per_stream = (h->max_chunks + h->GPW - 1) / h->GPW;
    h->max_blocks = max_blocks_per_stream;
    {
        // Run-length pre-filter: a run shorter than r_min cells (and not through t = 0) fails the duration gate whatever
        // else holds -- (len + 1) * hop < signal_min_duration (analyze.py:427-430; rt_core.h: gate_run), with a margin of
        // 1e-9 for the rounding of the float64 expressions.  A run of >= 2 L - 1 cells covers an aligned chunk of L.
        const long long r_min = min_run_cells(h);
        h->ap.lv.prefilter_ok = !general && !big && h->L >= 4 && 2ll * h->L - 1 <= r_min && h->max_seg >= 2 * h->L &&
                                h->max_chunks <= (1 << 18);  // (plan_pass_b keeps a bit per chunk in LDS)
        if (cfg->mode == RT_MODE_PREFILTER && !h->ap.lv.prefilter_ok) {
            delete h;
            return fail_create(RT_E_UNSUPPORTED, "RT_MODE_PREFILTER needs signal_min_duration >= 2 * segs_per_chunk STFT hops");
        }
        // nperseg 4096 without chunk bits (they need chunks of one length): a stream's earliest chunks are half as long, so that
        // the last items a launch hands out are short (rt_kernels.h: chunk_geometry).  A few chunks more than max_seg / L.
        h->two_level = scan_wave64(R3) && !h->ap.lv.prefilter_ok && !RT_DIAG_ENV("RT_EXP_ONE_LEVEL");  // (the variable: A/B runs of diagnostic builds, rt_diag.h)
        if (h->two_level) {
            h->max_chunks += h->max_chunks / 4 + 2;
            max_blocks_per_stream = (h->max_chunks + h->GPW - 1) / h->GPW;
            h->max_blocks = max_blocks_per_stream;
        }
        // Exact run-length pre-filter: any chunk length, any plateau length the planner's counters hold (rt_kernels.h: plan_runs).
        // Built where it is asked for, and in AUTO mode.
        h->run_cells = (int)std::max<long long>(1, std::min<long long>(r_min, 1 << 20));
        // (lane groups of two lanes -- nperseg 32 -- hold half a planner word per row: no exact pre-filter there)
        const bool fits = !general && !big && h->LG >= 4 && std::min<long long>(h->run_cells, (long long)h->max_seg + 1) <= kPlanMaxRun && h->max_seg >= 2;
        if (cfg->mode == RT_MODE_RUNFILTER && !fits) {
            delete h;
            return fail_create(RT_E_UNSUPPORTED, "RT_MODE_RUNFILTER: the minimum plateau length (in STFT hops) is beyond the planner's counters");
        }
        h->ap.lv.runfilter_ok = fits && (cfg->mode == RT_MODE_RUNFILTER || cfg->mode == RT_MODE_AUTO);
        if (h->ap.lv.runfilter_ok && cfg->mode == RT_MODE_AUTO) {
            // In AUTO mode the level is optional -- the only one between the sparse and the dense path at the reference's
            // default geometry, the one above the chunk bits elsewhere (noise far over the absolute threshold: every chunk
            // bit set, while SNR-aware cell bits stay selective): its scratch (two slots of threshold bits + kept cells +
            // segment lists + chunk minima) is taken where it is a small part of what is free -- at most half where it is
            // the only middle level, an eighth where the chunk bits exist -- and AUTO does without it otherwise.
            const size_t per_slot = (size_t)cfg->n_streams * std::max(h->max_seg, 1) * (size_t)(h->LG * 4 + 4) + (size_t)cfg->n_streams * h->N * 4 * (size_t)(h->max_blocks + 2);
            size_t free_b = 0, total_b = 0;
            if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || (size_t)kSlots * per_slot > free_b / (h->ap.lv.prefilter_ok ? 8 : 2)) h->ap.lv.runfilter_ok = false;
        }
    }
    if (!general && ((long long)h->N << key_tbits(std::max(h->max_seg, 2))) > 0x100000000ll) {
        delete h;
        return fail_create(RT_E_UNSUPPORTED, "max_samples too large for 32-bit cell keys");
    }
    // candidate cells per (stream, bucket): by default a full row of one bin fits, times nperseg / 1024 -- a bucket
    // holds nperseg / 16 bins, and with 256 of them (nperseg 4096) a dozen tags per stream put several active
    // bins into one bucket (config 5: up to ~1000 cells per bucket at 781 segments)
    h->hot_cap = general ? 64  // (no candidate lists on the dense path: the smallest scratch)
                 : cfg->hot_capacity > 0
                     ? cfg->hot_capacity
                     : std::min(8192, std::max(kSmallBucket, next_pow2(std::max(h->max_seg, 1)) * std::max(1, h->N / 1024)));
    h->lds_dense = rec_lds_bytes(h->rec_cap);
    {
        // plateaus a wave stages per bucket: a bucket holds N/16 bins; 32 keeps four waves' LDS
        // under 40 KiB (all 16 bucket waves of a CU resident at once) for nperseg 256/512
        h->cand_cap = (h->N / kBuckets <= 32) ? 32 : kCandCapMax;
        const size_t tail = (((size_t)(h->N / kBuckets) * 4 + 15) & ~(size_t)15) + sizeof(rt_record) * h->cand_cap;
        h->lds_large = (size_t)next_pow2(std::max(h->hot_cap, 64)) * 8 + tail;
        h->lds_small = 4 * ((size_t)kSmallBucket * 8 + tail);
    }
    if (h->lds_large + 8 * 1024 > 160 * 1024) {
        delete h;
        return fail_create(RT_E_INVALID, "hot_capacity does not fit the 160 KiB LDS of a CU");
    }
    {
        // Sparse detection by groups of buckets (detect_group) where a launch of one wave per (stream, bucket) would be many rounds of
        // nearly empty waves: from 1 024 streams per handle on (below that the per-bucket waves fit the chip in a round or two and finish
        // sooner than one wave per stream would).  Needs the group's row means beside its cells (nperseg <= 256) and (bin, t) + a
        // 10-bit position in one word.  RT_FLAG_GROUP_DETECT / RT_FLAG_NO_GROUP_DETECT force it either way (tests, A/B runs).
        int fbits = 0;
        while ((1 << fbits) < h->N) ++fbits;
        const bool can = !general && h->N <= kGroupBins && fbits + key_tbits(std::max(h->max_seg, 1)) + 10 <= 32;
        const bool want = (cfg->flags & RT_FLAG_GROUP_DETECT) ? true : (cfg->flags & RT_FLAG_NO_GROUP_DETECT) ? false
                          : cfg->n_streams >= 1024 || (g_creating_lane && (cfg->flags & kFlagLaneOfLargeBatch));
        h->group_detect = can && want;
        h->group_forced = (cfg->flags & RT_FLAG_GROUP_DETECT) != 0;
    }

    auto fail = [&](int code, const std::string &msg) {
        std::string m = msg;
        rt_destroy(h);
        return fail_create(code, m);
    };
#define RT_CREATE_HIP(expr)                                                                  \
    do {                                                                                     \
        hipError_t e2_ = (expr);                                                             \
        if (e2_ != hipSuccess) return fail(RT_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e2_)); \
    } while (0)

    if (cfg->hip_stream) {
        h->s_scan = static_cast<hipStream_t>(cfg->hip_stream);
        h->s_detect = h->s_scan;  // (a caller's stream: everything in order on it)
    } else {
        RT_CREATE_HIP(hipStreamCreateWithFlags(&h->s_scan, hipStreamNonBlocking));
        h->own_scan_stream = true;
        // A second stream for everything behind a call's first scan (enqueue_analysis: `sd`) -- where it pays.  Measured on one box
        // each, whole path, against everything in order on one stream: config 2 one lane 0.79 -> 0.73 ms per step (profiles/r04_e_*);
        // the exact pre-filter at the reference's default geometry 2.45 -> 2.1 ms (round 5: its planning kernels and second scan run
        // beside the next call's first scan, profiles/r05_b_*).  Not at nperseg >= 1024: behind a persistent grid (a chip-filling
        // launch whose workgroups live until the items run out) the next scan takes the chip first, the tail runs at its very end,
        // and rt_fetch -- and with it the host's next rt_process -- returns a scan later than it could (config 3 14.87 -> 15.7 ms per
        // step; nperseg 4096: 5.09 ms per launch in order against 5.34 with the detection's stream beside it, round 4's csv).
        // The lanes of a laned handle overlap one another's tails already (config 2 two lanes 0.688 -> 0.735 with a second stream
        // per lane).  Stream priorities changed none of this.
        bool second = R3 <= 2 && !big && !g_creating_lane;  // (stft_wg's launches fill the chip many times over: in order, like nperseg >= 1024)
        if (const char *v = RT_DIAG_ENV("RT_EXP_TAIL")) h->tail_mode = (v[0] == 'C') ? 1 : 0;
        if (const char *v = RT_DIAG_ENV("RT_EXP_STREAMS")) second = (v[0] == '2');  // (diagnostic builds: "1" / "2" force the choice, lanes included)
        if (!second) {
            h->s_detect = h->s_scan;
        } else {
            int least = 0, greatest = 0;
            (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
            int prio = greatest;
            if (const char *v = RT_DIAG_ENV("RT_EXP_TAIL_PRIO")) prio = v[0] == 'l' ? least : v[0] == 'n' ? 0 : greatest;
            RT_CREATE_HIP(hipStreamCreateWithPriority(&h->s_detect, hipStreamNonBlocking, prio));
        }
    }

    const int S = cfg->n_streams, N = h->N, LG = h->LG;
    h->ledger.configure(S);
    if (general) {
        const int M = h->gen_m;
        const std::vector<cf> twg = transform_twiddles<cf, double>(M);
        RT_DEVICE_COPY(RT_CREATE_HIP, h->d_twg, twg.data(), sizeof(cf) * twg.size());
        {
            std::vector<const void *> big_lds;
#define RT_BIG_LDS(F_)                                                                                                             \
    big_lds.insert(big_lds.end(), {reinterpret_cast<const void *>(stft_general<F_>), reinterpret_cast<const void *>(stft_bluestein<F_, 1, 256>), \
                                   reinterpret_cast<const void *>(stft_bluestein<F_, 2, 256>), reinterpret_cast<const void *>(stft_bluestein<F_, 2, 512>), \
                                   reinterpret_cast<const void *>(stft_bluestein<F_, 4, 512>), reinterpret_cast<const void *>(stft_bluestein<F_, 4, 1024>)})
            RT_BIG_LDS(kFmtC64);
            RT_BIG_LDS(kFmtU8);
            RT_BIG_LDS(kFmtI16);
            RT_BIG_LDS(kFmtI8);
#undef RT_BIG_LDS
            for (const void *f : big_lds) RT_CREATE_HIP(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, padded_len(kGeneralMaxN, 14) * (int)sizeof(cf)));
        }
        if (h->bluestein) {
            const BluesteinTables<cf> bt = bluestein_tables<cf, double>(cfg->window, N, M, h->log2n, std::sqrt((double)cfg->scale));
            RT_DEVICE_COPY(RT_CREATE_HIP, h->d_cwin, bt.cwin.data(), sizeof(cf) * bt.cwin.size());
            RT_DEVICE_COPY(RT_CREATE_HIP, h->d_bfilt, bt.bfilt.data(), sizeof(cf) * bt.bfilt.size());
        }
    }
    // window and twiddle tables, built in rt_tables.h (where each layout is described beside the kernel that reads it)
    static_assert(kScan64TwiddleRows == kW64TwRows, "rt_tables.h builds stft_scan64's twiddle rows");
    const ScanTwiddles tw = scan_twiddles(N, R3, QS, big, scan_wave64(R3));
    const std::vector<float> ws = scaled_window(cfg->window, N, cfg->scale);
    {
        int cus = 0;
        RT_CREATE_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, cfg->device));
        if (cus > 0) h->n_cu = cus;
    }
    h->h_sub_first.assign((size_t)cfg->n_streams, 0);
    RT_DEVICE_ZEROS(RT_CREATE_HIP, h->d_sub_first, (size_t)cfg->n_streams * sizeof(int32_t));
    RT_CREATE_HIP(hipHostMalloc(&h->h_sub_list, (size_t)cfg->n_streams * sizeof(int32_t)));
    RT_DEVICE_ZEROS(RT_CREATE_HIP, h->d_work, 2 * sizeof(uint32_t));
    RT_DEVICE_COPY(RT_CREATE_HIP, h->d_window, ws.data(), sizeof(float) * N);
    RT_DEVICE_COPY(RT_CREATE_HIP, h->d_tw1, tw.tw1.data(), sizeof(cf) * tw.tw1.size());
    RT_DEVICE_COPY(RT_CREATE_HIP, h->d_tw2, tw.tw2.data(), sizeof(cf) * tw.tw2.size());
    if (big || R3 == 16) {
        const std::vector<float> wt = big ? window_thread_order(ws, N, big) : window_lane_order(ws, N, LG, scan_wave64(R3));
        RT_DEVICE_COPY(RT_CREATE_HIP, h->d_window_t, wt.data(), sizeof(float) * N);
    }
    {
        // If the window is a cosine sum of order <= 1 the constant detrend is applied to the transform (LIN kernels); any other
        // window keeps the subtract-first kernels.
        const CosineFit fit = fit_cosine_window(ws, N);
        h->lin = fit.cosine_sum && !(cfg->flags & RT_FLAG_NO_LIN_DETREND) && !big;
        if (h->lin) {
            for (int j = 0; j < 3; ++j) h->lin_c[j] = (float)(fit.wr[j] / N);
        }
        if (big) {
            // stft_wg subtracts the mean first, in SciPy's order (no linearity form, no guard); what it takes from the fit is the WINDOW:
            // w[n] = c0 + c1 cos 2 pi n / N, c0 = W[0] / N, c1 = (W[1] + W[N-1]) / N (rt_scan_wg.h: WCOS)
            h->wcos = fit.cosine_sum;
            h->lin_c[0] = (float)(fit.wr[0] / N);
            h->lin_c[1] = (float)((fit.wr[1] + fit.wr[2]) / N);
            h->lin_c[2] = 0.f;
        }
    }

    const size_t psum_bytes = (size_t)S * max_blocks_per_stream * N * sizeof(float);
    const size_t tail_bytes = (size_t)S * h->K * N * sizeof(float);
    for (auto &t : h->d_tail) RT_CREATE_HIP(hipMalloc(&t, tail_bytes));
    // (the records of streams re-run dense on their own go behind the ones already in the pool: their first lists stay orphaned)
    h->pool_max = ((int64_t)S + std::min(S, kMaxPartial)) * h->rec_cap;
    h->pool_want = std::min<int64_t>(h->pool_max, cfg->record_pool > 0 ? (int64_t)cfg->record_pool : std::min<int64_t>((int64_t)S * h->rec_cap, kInitialPoolRecords));
    for (auto &sl : h->slot) {
        sl.pool_cap = h->pool_want;
        RT_CREATE_HIP(hipMalloc(&sl.d_psum, std::max<size_t>(psum_bytes, 4)));
        if (h->ap.lv.prefilter_ok && cfg->mode != RT_MODE_DENSE)
            RT_CREATE_HIP(hipMalloc(&sl.d_full, (size_t)S * (h->max_chunks + h->L) * LG * sizeof(uint16_t)));  // + the bits of chunk 0 by segment
        if (sl.d_full) RT_CREATE_HIP(hipMalloc(&sl.d_items, ((size_t)S * h->max_blocks * h->GPW + S) * sizeof(int32_t)));
        if (h->ap.lv.runfilter_ok) {
            const size_t cells = (size_t)S * std::max(h->max_seg, 1) * LG;
            RT_CREATE_HIP(hipMalloc(&sl.d_cell_hot, cells * sizeof(uint16_t)));
            RT_DEVICE_ZEROS(RT_CREATE_HIP, sl.d_cell_need, cells * sizeof(uint16_t));  // (all zeros between calls: plan_runs writes only the words that keep anything)
            RT_CREATE_HIP(hipMalloc(&sl.d_chunk_min, std::max<size_t>(psum_bytes, 4)));  // (a row per work item, like psum)
            h->chunk_min_bytes = std::max<size_t>(psum_bytes, 4);
            RT_CREATE_HIP(hipMalloc(&sl.d_thr_bin, (size_t)S * N * sizeof(float)));
            RT_CREATE_HIP(hipMalloc(&sl.d_thr_nat, (size_t)S * N * sizeof(float)));
            RT_CREATE_HIP(hipMalloc(&sl.d_seg_list, ((size_t)S * std::max(h->max_seg, 1) + S + 1) * sizeof(int32_t)));
            RT_CREATE_HIP(hipHostMalloc(&sl.h_seg_total, sizeof(int32_t)));
            *sl.h_seg_total = 0;
        }
        if (sl.d_full || sl.d_cell_hot) {
            RT_DEVICE_ZEROS(RT_CREATE_HIP, sl.d_abs_hot, (size_t)S * sizeof(uint32_t));
            RT_CREATE_HIP(hipHostMalloc(&sl.h_abs_hot, sizeof(uint32_t)));
            *sl.h_abs_hot = 0u;
        }
        RT_CREATE_HIP(hipMalloc(&sl.d_hot, (size_t)S * kBuckets * h->hot_cap * sizeof(uint2)));
        RT_DEVICE_ZEROS(RT_CREATE_HIP, sl.d_hot_count, (size_t)S * kBuckets * sizeof(uint32_t));
        RT_DEVICE_ZEROS(RT_CREATE_HIP, sl.d_hot_seen, (size_t)S * kBuckets * sizeof(uint32_t));
        RT_CREATE_HIP(hipHostMalloc(&sl.h_hot_total, (size_t)S * sizeof(int32_t)));
        std::memset(sl.h_hot_total, 0, (size_t)S * sizeof(int32_t));
        RT_CREATE_HIP(hipMalloc(&sl.d_raw, (size_t)S * h->rec_cap * sizeof(rt_record)));
        RT_DEVICE_ZEROS(RT_CREATE_HIP, sl.d_raw_count, (size_t)S * sizeof(int32_t));
        RT_DEVICE_ZEROS(RT_CREATE_HIP, sl.d_counters, kCounterWords * sizeof(unsigned long long));
        RT_CREATE_HIP(hipHostMalloc(&sl.h_counters, kCounterWords * sizeof(unsigned long long)));
        RT_CREATE_HIP(hipHostMalloc(&sl.h_rec_offset, (size_t)S * sizeof(int32_t)));
        RT_CREATE_HIP(hipHostMalloc(&sl.h_rec_count, (size_t)S * sizeof(int32_t)));
        RT_CREATE_HIP(hipHostMalloc(&sl.h_records, (size_t)sl.pool_cap * sizeof(rt_record)));
        RT_CREATE_HIP(hipHostMalloc(&sl.h_no_last, (size_t)S * sizeof(int32_t)));
        std::memset(sl.h_no_last, 0, (size_t)S * sizeof(int32_t));
        RT_CREATE_HIP(hipHostMalloc(&sl.h_overflow, (size_t)S * sizeof(int32_t)));
        std::memset(sl.h_overflow, 0, (size_t)S * sizeof(int32_t));
        RT_CREATE_HIP(hipHostMalloc(&sl.h_incons, (size_t)S * sizeof(int32_t)));
        std::memset(sl.h_incons, 0, (size_t)S * sizeof(int32_t));
        RT_CREATE_HIP(hipHostMalloc(&sl.h_dc_flag, (size_t)S * sizeof(int32_t)));
        std::memset(sl.h_dc_flag, 0, (size_t)S * sizeof(int32_t));
        RT_CREATE_HIP(hipHostMalloc(&sl.h_list, (size_t)kMaxPartial * sizeof(int32_t)));
        RT_CREATE_HIP(hipHostMalloc(&sl.h_total, sizeof(unsigned long long)));
        if (cfg->flags & RT_FLAG_ROW_MEANS) RT_CREATE_HIP(hipMalloc(&sl.d_row_means, (size_t)S * N * sizeof(float)));
        if (cfg->flags & RT_FLAG_RECORD_CELLS) {
            sl.cell_cap = std::max<int64_t>(64, std::min<int64_t>(kInitialPoolCells, 16 * sl.pool_cap));
            RT_CREATE_HIP(hipMalloc(&sl.d_cells, (size_t)sl.cell_cap * sizeof(float)));
            RT_DEVICE_ZEROS(RT_CREATE_HIP, sl.d_hot_kept, (size_t)S * kBuckets * sizeof(uint32_t));
            RT_CREATE_HIP(hipMalloc(&sl.d_stream_cells, (size_t)S * sizeof(long long)));
            RT_CREATE_HIP(hipMalloc(&sl.d_stream_base, (size_t)S * sizeof(long long)));
            RT_CREATE_HIP(hipHostMalloc(&sl.h_cells_info, 2 * sizeof(unsigned long long)));
            sl.h_cells_info[0] = sl.h_cells_info[1] = 0ull;
        }
        RT_CREATE_HIP(hipEventCreate(&sl.ev_begin));
        RT_CREATE_HIP(hipEventCreateWithFlags(&sl.ev_first, hipEventDisableTiming));
        RT_CREATE_HIP(hipEventCreate(&sl.ev_scan));
        RT_CREATE_HIP(hipEventCreate(&sl.ev_done));
    }

    if (big) {
#define RT_WG_SET(B_, M_, U_, W_) RT_CREATE_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(stft_wg<B_, M_, U_, W_>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)wg_lds_bytes(B_)))
#define RT_WG_SET4(B_, M_) RT_WG_SET(B_, M_, false, false); RT_WG_SET(B_, M_, false, true); RT_WG_SET(B_, M_, true, false); RT_WG_SET(B_, M_, true, true); \
    RT_WG_SET(B_, M_ | kModeI16, false, false); RT_WG_SET(B_, M_ | kModeI16, false, true); \
    RT_WG_SET(B_, M_ | kModeI8, false, false); RT_WG_SET(B_, M_ | kModeI8, false, true)
        RT_WG_SET4(256, 0); RT_WG_SET4(256, 1); RT_WG_SET4(256, 2);
        RT_WG_SET4(512, 0); RT_WG_SET4(512, 1); RT_WG_SET4(512, 2);
#undef RT_WG_SET4
#undef RT_WG_SET
    }
    RT_CREATE_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(detect_bucket<true>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds_large));
    RT_CREATE_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(detect_bucket<false>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds_small));
    RT_CREATE_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(detect_group), hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds_small));
    RT_CREATE_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(detect_bucket_listed), hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds_small));
    RT_CREATE_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(detect_dense<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)rec_lds_bytes(kDenseLdsRecords)));
#undef RT_CREATE_HIP
    *out = h;
    return RT_OK;
}

int rt_reset(rt_handle *h) {
    if (!h) return RT_E_INVALID;
    forget_row_means(h);
    for (rt_handle *k : h->kids) rt_reset(k);
    h->ledger.forget_all();  // (no look-back, no lead: the held sample tails go with it)
    return RT_OK;
}

int rt_reset_stream(rt_handle *h, int32_t stream) {
    if (!h) return RT_E_INVALID;
    if (stream < 0 || stream >= h->cfg.n_streams) {
        h->err = "stream index out of range";
        return RT_E_INVALID;
    }
    if (!h->kids.empty()) {
        for (size_t k = 0; k < h->kids.size(); ++k)
            if (stream < h->kid_base[k + 1]) return rt_reset_stream(h->kids[k], stream - h->kid_base[k]);
        return RT_E_INVALID;
    }
    h->ledger.reset_stream(stream);
    return RT_OK;
}

static int refuse_on_f64(rt_handle *h, const char *what, const char *twin) {
    h->err = std::string(what) + " on a float64 handle (rt_create_f64): " + (twin ? std::string("use ") + twin : std::string("not available"));
    return RT_E_INVALID;
}

int rt_set_stream_params(rt_handle *h, const float *threshold, const float *calibration_db) {
    if (!h) return RT_E_INVALID;
    if (h->f64) return refuse_on_f64(h, "rt_set_stream_params", "rt_set_stream_params_f64");
    if (!h->kids.empty())
        return for_each_lane(h, [&](rt_handle *k, int64_t s0) {
            return rt_set_stream_params(k, threshold ? threshold + s0 : nullptr, calibration_db ? calibration_db + s0 : nullptr);
        });
    if (oldest_pending(h)) {
        // a pending call may still be re-run when it is fetched (AUTO mode): it must see the thresholds it was enqueued with
        h->err = "rt_set_stream_params with unfetched calls pending: fetch them first";
        return RT_E_INVALID;
    }
    { const int rcu = chain_runs_uniform(h, h->ledger.chain, "rt_set_stream_params", threshold, calibration_db, nullptr, nullptr, nullptr); if (rcu != RT_OK) return rcu; }
    return set_stream_params_one<float>(h, h->cfg.threshold, h->h_thr_s, &h->h_cal_s, h->d_thr_s, h->d_cal_s, threshold, calibration_db);
}

int rt_set_stream_settings(rt_handle *h, const float *snr_threshold, const double *min_duration_s, const double *max_duration_s) {
    if (!h) return RT_E_INVALID;
    if (h->f64) return refuse_on_f64(h, "rt_set_stream_settings", "rt_set_stream_settings_f64");
    // every refusal before the first copy, in every lane: the values (checked on the whole batch, so that a message names the
    // stream as the caller counts it -- the lanes share rt_config's envelope), then the pending calls
    const int rc = check_stream_settings<float>(h, "rt_set_stream_settings", snr_threshold, min_duration_s, max_duration_s);
    if (rc != RT_OK) return rc;
    { const int rcu = chain_runs_uniform(h, h->ledger.chain, "rt_set_stream_settings", nullptr, nullptr, snr_threshold, min_duration_s, max_duration_s); if (rcu != RT_OK) return rcu; }
    bool pending = h->kids.empty() && oldest_pending(h);
    for (rt_handle *k : h->kids) pending = pending || oldest_pending(k);
    if (pending) {
        // a pending call may still be re-run when it is fetched (AUTO mode): it must see the settings it was enqueued with
        h->err = "rt_set_stream_settings with unfetched calls pending: fetch them first";
        return RT_E_INVALID;
    }
    if (!h->kids.empty())
        return for_each_lane(h, [&](rt_handle *k, int64_t s0) {
            return set_stream_settings_one<float>(k, k->cfg.snr_threshold, k->h_set_s, k->d_set_s, snr_threshold ? snr_threshold + s0 : nullptr,
                                                  min_duration_s ? min_duration_s + s0 : nullptr, max_duration_s ? max_duration_s + s0 : nullptr);
        });
    return set_stream_settings_one<float>(h, h->cfg.snr_threshold, h->h_set_s, h->d_set_s, snr_threshold, min_duration_s, max_duration_s);
}

// rt_set_present (include/rt_analyze.h).  The first call on a handle allocates the two call slots' mask rows and moves the handle
// to per-stream segment counts (rt_core.h: PresenceBook), every stream starting from the handle's one count; calls already
// enqueued keep that count.  Later calls only change the mask in force: host memory, no copy, no launch, no synchronisation.
int rt_set_present(rt_handle *h, const uint8_t *present) {
    if (!h) return RT_E_INVALID;
    if (!h->kids.empty())
        return for_each_lane(h, [&](rt_handle *k, int64_t s0) { return rt_set_present(k, present ? present + s0 : nullptr); });
    const int S = h->cfg.n_streams;
    if (!h->ledger.pres.active) {
        RT_HIP(h, hipSetDevice(h->cfg.device));
        const size_t bytes = (size_t)kMaskRows * (size_t)S * sizeof(int32_t);
        int32_t *hm[kSlots] = {nullptr, nullptr}, *dm[kSlots] = {nullptr, nullptr};
        bool ok = true;
        for (int i = 0; i < kSlots && ok; ++i) ok = hipHostMalloc(&hm[i], bytes) == hipSuccess && hipMalloc(&dm[i], bytes) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            for (int i = 0; i < kSlots; ++i) {
                (void)hipHostFree(hm[i]);
                (void)hipFree(dm[i]);
            }
            h->err = "rt_set_present: no memory for the mask rows";
            return RT_E_NOMEM;
        }
        for (int i = 0; i < kSlots; ++i) {
            std::memset(hm[i], 0, bytes);
            if (h->f64) {
                h->f64->slot[i].h_mask = hm[i];
                h->f64->slot[i].d_mask = dm[i];
            } else {
                h->slot[i].h_mask = hm[i];
                h->slot[i].d_mask = dm[i];
            }
        }
        // RT_MODE_RUNFILTER's quiet levels are not carried across a gap: a stream's thresholds behind one come from
        // whatever rows of chunk minima the slots still hold.  From here on those are minima some scan wrote or "none" (0x7f7f7f7f:
        // no estimate, the absolute threshold alone), never what the allocation happened to hold.  Behind everything enqueued.
        if (!h->f64)
            for (int i = 0; i < kSlots; ++i)
                if (h->slot[i].d_chunk_min && h->chunk_min_bytes) RT_HIP(h, hipMemsetAsync(h->slot[i].d_chunk_min, 0x7f, h->chunk_min_bytes, h->s_scan));
        h->ledger.activate_presence();
    }
    h->ledger.set_mask(present);
    return RT_OK;
}

// rt_set_chain (include/rt_analyze.h).  Every refusal comes before any device work.  The first call with links >= 2 moves the
// handle to the per-stream rows of rt_set_present (a chained call always fills them) and allocates, per call slot, the source
// rows and the [S][K][N] buffer its detection reads as look-back (rt_chain.h); later calls only regroup the book.
int rt_set_chain(rt_handle *h, int32_t links) {
    if (!h) return RT_E_INVALID;
    if (links < 0) {
        h->err = "rt_set_chain: links must be >= 0";
        return RT_E_INVALID;
    }
    if (h->f64) {
        h->err = "rt_set_chain on a float64 handle (rt_create_f64): not available in this version";
        return RT_E_UNSUPPORTED;
    }
    if (!h->kids.empty() || h->cfg.lanes > 1) {
        h->err = "rt_set_chain on a handle created with lanes > 1: lanes cut the streams into groups that a run may straddle (not available in this version)";
        return RT_E_UNSUPPORTED;
    }
    const int S = h->cfg.n_streams;
    const int want = links >= 2 ? links : 0;
    if (want && S % want != 0) {
        h->err = "rt_set_chain: links " + std::to_string(links) + " does not divide n_streams " + std::to_string(S);
        return RT_E_INVALID;
    }
    if (oldest_pending(h)) {
        h->err = "rt_set_chain with unfetched calls pending: fetch them first";
        return RT_E_INVALID;
    }
    if (want == h->ledger.chain.links) return RT_OK;
    if (want) {
        ChainBook next;
        next.configure(S, want);
        std::vector<float> snr;
        std::vector<double> min_d, max_d;
        for (const StreamSettings &q : h->h_set_s) {
            snr.push_back(q.snr);
            min_d.push_back(q.min_d);
            max_d.push_back(q.max_d);
        }
        const int rcu = chain_runs_uniform(h, next, "rt_set_chain", h->h_thr_s.empty() ? nullptr : h->h_thr_s.data(), h->h_cal_s.empty() ? nullptr : h->h_cal_s.data(),
                                           snr.empty() ? nullptr : snr.data(), min_d.empty() ? nullptr : min_d.data(), max_d.empty() ? nullptr : max_d.data());
        if (rcu != RT_OK) return rcu;
        if (!h->slot[0].d_chain) {
            RT_HIP(h, hipSetDevice(h->cfg.device));
            const size_t row_bytes = 2 * (size_t)S * sizeof(int32_t), col_bytes = (size_t)S * (size_t)h->K * (size_t)h->N * sizeof(float);
            int32_t *hr[kSlots] = {nullptr, nullptr}, *dr[kSlots] = {nullptr, nullptr};
            float *dc[kSlots] = {nullptr, nullptr};
            bool ok = true;
            for (int i = 0; i < kSlots && ok; ++i)
                ok = hipHostMalloc(&hr[i], row_bytes) == hipSuccess && hipMalloc(&dr[i], row_bytes) == hipSuccess && hipMalloc(&dc[i], col_bytes ? col_bytes : 4) == hipSuccess;
            if (!ok) {
                (void)hipGetLastError();
                for (int i = 0; i < kSlots; ++i) {
                    (void)hipHostFree(hr[i]);
                    (void)hipFree(dr[i]);
                    (void)hipFree(dc[i]);
                }
                h->err = "rt_set_chain: no memory for the chained look-back columns (" + std::to_string(col_bytes) + " bytes per call slot)";
                return RT_E_NOMEM;
            }
            for (int i = 0; i < kSlots; ++i) {
                std::memset(hr[i], 0, row_bytes);
                h->slot[i].h_chain_rows = hr[i];
                h->slot[i].d_chain_rows = dr[i];
                h->slot[i].d_chain = dc[i];
            }
        }
        if (!h->ledger.pres.active) {
            const int rcp = rt_set_present(h, nullptr);  // (every stream present: the mask rows exist from here on)
            if (rcp != RT_OK) return rcp;
        }
    }
    forget_row_means(h);
    h->ledger.set_chain(want);  // (a change of the grouping forgets all look-back, as rt_reset does)
    return RT_OK;
}

static int process_impl(rt_handle *h, const void *iq_dev, int64_t n_samples, int64_t stream_stride, int fmt);

int rt_process(rt_handle *h, const void *iq_dev, int64_t n_samples, int64_t stream_stride) {
    return process_impl(h, iq_dev, n_samples, stream_stride, kFmtC64);
}

int rt_process_u8(rt_handle *h, const void *iq_u8_dev, int64_t n_samples, int64_t stream_stride) {
    return process_impl(h, iq_u8_dev, n_samples, stream_stride, kFmtU8);
}

int rt_process_i16(rt_handle *h, const void *iq_i16_dev, int64_t n_samples, int64_t stream_stride) {
    return process_impl(h, iq_i16_dev, n_samples, stream_stride, kFmtI16);
}

int rt_process_i8(rt_handle *h, const void *iq_i8_dev, int64_t n_samples, int64_t stream_stride) {
    return process_impl(h, iq_i8_dev, n_samples, stream_stride, kFmtI8);
}

static int process_f64(rt_handle *h, const void *iq, int64_t n_samples, int64_t stream_stride, int fmt, bool host);

static int process_impl(rt_handle *h, const void *iq_dev, int64_t n_samples, int64_t stream_stride, int fmt) {
    if (!h) return RT_E_INVALID;
    forget_row_means(h);
    if (h->f64) return process_f64(h, iq_dev, n_samples, stream_stride, fmt, false);
    if (!h->kids.empty()) {
        const int64_t bytes = (int64_t)fmt_sample_bytes(fmt);
        return for_each_lane(h, [&](rt_handle *k, int64_t s0) {
            const char *base = iq_dev ? static_cast<const char *>(iq_dev) + s0 * stream_stride * bytes : nullptr;
            return process_impl(k, base, n_samples, stream_stride, fmt);
        }, true);
    }
    int T = 0;
    int rc = check_process_args(h, iq_dev, n_samples, stream_stride, fmt, true, &T);
    if (rc != RT_OK) return rc;
    RT_HIP(h, hipSetDevice(h->cfg.device));
    Slot *slp = nullptr;
    CallCtx saved;
    rc = claim_slot(h, &slp, &saved);
    if (rc != RT_OK) return rc;
    Slot &sl = *slp;
    CallCtx &c = sl.call;
    LedgerCall &lc = sl.lc;
    c.prev_auto = h->ap.restore_point();
    c.prev_minsum_slot = h->minsum_slot;
    c.iq = iq_dev;
    c.fmt = fmt;
    c.n_samples = n_samples;
    c.stream_stride = stream_stride;
    c.n_seg = T;
    // Everything that can fail from here on runs inside `enqueue`; one block below undoes a failed call: nothing stays
    // enqueued, the ledger (look-back state, pending stream resets, books) is the one before the call, and the call the slot
    // held (possibly still unfetched) is put back unless a launch has already rewritten its scratch (include/rt_analyze.h).
    bool launched = false;
    auto enqueue = [&]() -> int {
        const int S = h->cfg.n_streams, idx = (int)(&sl - h->slot);
        const Slot &o = h->slot[1 - idx];
        // the ledger's decisions for this call, and with rt_set_record_iq on the tails of its samples in front of its scan
        const int rcl = begin_ledger_call(h, idx, lc, o.call.pending ? &o.lc : nullptr, saved.seq ? sl.ev_done : nullptr, T, fmt, iq_dev, stream_stride);
        if (rcl != RT_OK) return rcl;
        c.tail_read = lc.tail_read;
        c.tail_write = lc.tail_write;
        c.n_seg_last = lc.n_seg_last;
        // (the slot's pinned rows are rewritten from here on: its previous call -- two calls back -- may still be reading them if it
        // was never fetched)
        if ((lc.masked || !lc.took.empty()) && sl.ev_done && h->n_calls >= (uint64_t)kSlots) RT_HIP(h, hipEventSynchronize(sl.ev_done));
        if (lc.masked || lc.iq_on) launched = true;
        if (lc.masked) {
            // rt_set_present: the mask in force, every stream's own previous segment count and the resets it takes go to the device, and
            // the absent streams' look-back columns are carried along the rotation; rt_set_chain: who follows whom
            int rcm = lc.chained ? upload_chain_rows(h, sl) : RT_OK;
            if (rcm == RT_OK) rcm = upload_mask(h, sl);
            if (rcm == RT_OK)
                rcm = enqueue_carry<float>(h, sl.d_mask + (size_t)kMaskAbsentList * S, sl.n_absent, h->d_tail[c.tail_read], h->d_tail[c.tail_write], h->K, h->N);
            if (rcm != RT_OK) return rcm;
        } else if (!lc.took.empty()) {
            std::memcpy(sl.h_no_last, lc.took.data(), (size_t)S * sizeof(int32_t));  // (lock-step: the streams that take a reset)
        }
        if (h->ist && h->ist->on) {
            // rt_set_input_stats: the rows of the raw input, once per call (no re-analysis inside rt_fetch comes through here)
            launched = true;  // (the slot's rows are rewritten from here on)
            const int rci = enqueue_input_stats(h, idx, iq_dev, n_samples, stream_stride, fmt, lc.masked ? sl.d_mask + (size_t)kMaskAbsent * S : nullptr);
            if (rci != RT_OK) return rci;
        }
        c.mode_used = h->ap.begin_call(h->cfg.mode, (uint64_t)kBuckets * (uint64_t)h->hot_cap, (uint64_t)T * (uint64_t)h->N);
        if (T == 0) {
            // empty spectrogram: no signals; `_spectrogram_last` becomes an empty map
            const size_t sb = (size_t)S * sizeof(int32_t);
            launched = true;  // (the slot's result arrays are rewritten from here on)
            RT_HIP(h, hipMemsetAsync(sl.d_counters, 0, kCounterWords * sizeof(unsigned long long), h->s_scan));
            RT_HIP(h, hipMemsetAsync(sl.h_rec_count, 0, sb, h->s_scan));
            RT_HIP(h, hipMemsetAsync(sl.h_rec_offset, 0, sb, h->s_scan));
            RT_HIP(h, hipEventRecord(sl.ev_begin, h->s_scan));
            RT_HIP(h, hipEventRecord(sl.ev_scan, h->s_scan));
            const int rc2 = enqueue_readback(h, sl, h->s_scan);
            if (rc2 != RT_OK) return rc2;
            RT_HIP(h, hipEventRecord(sl.ev_done, h->s_scan));
            return RT_OK;
        }
        return enqueue_analysis(h, sl, c.mode_used, &launched);
    };
    rc = enqueue();
    if (rc != RT_OK) {
        undo_call_books(h, sl);
        if (launched) {
            (void)hipStreamSynchronize(h->s_scan);
            (void)hipStreamSynchronize(h->s_detect);
            sl.call = CallCtx{};
        } else {
            sl.call = saved;
            std::swap(sl.lc, h->lc_saved);
        }
        return rc;
    }
    c.pending = true;
    h->n_calls++;
    if (h->ist && h->ist->on) h->ist->slot[&sl - h->slot].seq = c.seq;  // (the slot's rows are this call's)
    return RT_OK;
}

static int process_host_impl(rt_handle *h, const void *iq_host, int64_t n_samples, int64_t stream_stride, int fmt) {
    if (!h) return RT_E_INVALID;
    forget_row_means(h);
    if (h->f64) return process_f64(h, iq_host, n_samples, stream_stride, fmt, true);
    const size_t sample_bytes = fmt_sample_bytes(fmt);
    if (!h->kids.empty())
        return for_each_lane(h, [&](rt_handle *k, int64_t s0) {
            const char *base = iq_host ? static_cast<const char *>(iq_host) + s0 * stream_stride * (int64_t)sample_bytes : nullptr;
            return process_host_impl(k, base, n_samples, stream_stride, fmt);
        }, true);
    if (n_samples < 0 || n_samples > h->cfg.max_samples || stream_stride < n_samples || (!iq_host && n_samples > 0)) {
        h->err = "n_samples/stream_stride out of range for this handle, or null IQ pointer";
        return RT_E_INVALID;
    }
    RT_HIP(h, hipSetDevice(h->cfg.device));
    const size_t bytes = (size_t)h->cfg.n_streams * (size_t)stream_stride * sample_bytes;
    // One staging buffer per call slot.  The call that used this slot two calls ago is over or dropped by now
    // (at most two are in flight); the one still in flight keeps its own buffer -- it may be re-run from it
    // when it is fetched (AUTO mode, candidate overflow), so it must not be overwritten by this call.
    const int which = (int)(h->n_calls % kSlots);
    Slot &prev = h->slot[which];
    if (prev.call.seq) RT_HIP(h, hipEventSynchronize(prev.ev_done));
    if (bytes > h->iq_stage_bytes[which]) {
        if (h->d_iq_stage[which]) (void)hipFree(h->d_iq_stage[which]);
        h->d_iq_stage[which] = nullptr;
        h->iq_stage_bytes[which] = 0;
        hipError_t e = hipMalloc(&h->d_iq_stage[which], bytes);
        if (e != hipSuccess) {
            h->err = std::string("IQ staging buffer: ") + hipGetErrorString(e);
            return RT_E_NOMEM;
        }
        h->iq_stage_bytes[which] = bytes;
    }
    // blocking copy: the caller may reuse or free its (pageable) buffer as soon as this returns
    if (bytes) RT_HIP(h, hipMemcpy(h->d_iq_stage[which], iq_host, bytes, hipMemcpyHostToDevice));
    return process_impl(h, h->d_iq_stage[which], n_samples, stream_stride, fmt);
}

int rt_process_host(rt_handle *h, const void *iq_host, int64_t n_samples, int64_t stream_stride) {
    return process_host_impl(h, iq_host, n_samples, stream_stride, kFmtC64);
}

int rt_process_u8_host(rt_handle *h, const void *iq_u8_host, int64_t n_samples, int64_t stream_stride) {
    return process_host_impl(h, iq_u8_host, n_samples, stream_stride, kFmtU8);
}

int rt_process_i16_host(rt_handle *h, const void *iq_i16_host, int64_t n_samples, int64_t stream_stride) {
    return process_host_impl(h, iq_i16_host, n_samples, stream_stride, kFmtI16);
}

int rt_process_i8_host(rt_handle *h, const void *iq_i8_host, int64_t n_samples, int64_t stream_stride) {
    return process_host_impl(h, iq_i8_host, n_samples, stream_stride, kFmtI8);
}

int rt_extract(rt_handle *h, const float *spec_dev, int32_t n_seg, int32_t n_bins, const float *last_dev,
               int32_t n_seg_last) {
    if (!h) return RT_E_INVALID;
    forget_row_means(h);
    if (h->f64) return refuse_on_f64(h, "rt_extract", "rt_extract_f64");
    if (!h->kids.empty())
        return for_each_lane(h, [&](rt_handle *k, int64_t s0) {
            const float *sp = spec_dev ? spec_dev + s0 * n_seg * n_bins : nullptr;
            const float *la = last_dev ? last_dev + s0 * n_seg_last * n_bins : nullptr;
            return rt_extract(k, sp, n_seg, n_bins, la, n_seg_last);
        }, true);
    if (n_seg < 0 || n_bins < 1 || (n_seg > 0 && !spec_dev) || (last_dev && n_seg_last < 0)) {
        h->err = "bad spectrogram arguments";
        return RT_E_INVALID;
    }
    if (n_seg == 1) {
        h->err = "exactly one segment: the reference raises IndexError (times[1])";
        return RT_E_ONE_SEGMENT;
    }
    if (reinterpret_cast<uintptr_t>(spec_dev) % 4u != 0 || reinterpret_cast<uintptr_t>(last_dev) % 4u != 0) {
        h->err = "spectrogram pointers must be 4-byte aligned (float32)";
        return RT_E_INVALID;
    }
    if ((int64_t)n_seg * n_bins > 0x7FFFFFFFll) {
        h->err = "spectrogram too large";
        return RT_E_UNSUPPORTED;
    }
    RT_HIP(h, hipSetDevice(h->cfg.device));
    Slot *slp = nullptr;
    CallCtx saved;
    int rc = claim_slot(h, &slp, &saved);
    if (rc != RT_OK) return rc;
    Slot &sl = *slp;
    CallCtx &c = sl.call;
    c.n_seg = n_seg;
    c.is_extract = true;
    c.mode_used = RT_MODE_DENSE;
    const size_t sb = (size_t)h->cfg.n_streams * sizeof(int32_t);
    RT_HIP(h, hipMemsetAsync(sl.d_counters, 0, kCounterWords * sizeof(unsigned long long), h->s_scan));
    RT_HIP(h, hipEventRecord(sl.ev_begin, h->s_scan));
    RT_HIP(h, hipEventRecord(sl.ev_scan, h->s_scan));
    if (n_seg == 0) {
        RT_HIP(h, hipMemsetAsync(sl.h_rec_count, 0, sb, h->s_scan));
        RT_HIP(h, hipMemsetAsync(sl.h_rec_offset, 0, sb, h->s_scan));
    } else {
        DetectArgs a = make_detect_args(h, sl, n_seg, n_bins, last_dev ? n_seg_last : -1);
        a.dp.tail_cols = last_dev ? n_seg_last : 0;
        a.prev = last_dev;
        a.prev_cols = last_dev ? n_seg_last : 0;
        a.spec = spec_dev;
        a.psum = nullptr;  // caller-supplied map: the kernel sums the rows itself
        launch_detect_dense(h, h->cfg.n_streams, h->s_scan, a);
        RT_HIP(h, hipGetLastError());
    }
    if (n_seg == 0) {
        rc = enqueue_readback(h, sl, h->s_scan);
        if (rc != RT_OK) return rc;
    }
    RT_HIP(h, hipEventRecord(sl.ev_done, h->s_scan));
    c.pending = true;
    h->n_calls++;
    return RT_OK;
}

// peek-mode results of fetch_one: the call produced no usable result (the caller decides what happens to it)
constexpr int kCallFailed = -100;          // -> RT_E_HOT_OVERFLOW (candidate lists overflowed in sparse mode)
constexpr int kCallFailedInternal = -101;  // -> RT_E_HIP

// drop the oldest pending call of a handle (its GPU work is waited for first)
static void discard_oldest(rt_handle *h) {
    Slot *sl = oldest_pending(h);
    if (!sl) return;
    (void)hipSetDevice(h->cfg.device);
    (void)hipEventSynchronize(sl->ev_done);
    sl->call.pending = false;
}

// A call is about to be analysed again from rt_fetch (level-up, stale thresholds, pool growth, the detrend guard) while a later
// call may be in flight: its re-run scan rewrites the look-back columns that later call's detection reads on the handle's second
// stream (the same values, or a superset of the cells -- still an unordered read / write pair), so the re-run waits for it.
static int before_rerun(rt_handle *h, Slot &sl) {
    if (h->s_detect != h->s_scan)
        for (auto &o : h->slot)
            if (&o != &sl && o.call.pending) RT_HIP(h, hipStreamWaitEvent(h->s_scan, o.ev_done, 0));
    return RT_OK;
}

// ... and the re-run itself: the same buffer with the same look-back state on `mode`, waited for; `flags` become its flag word.
enum : unsigned {
    kRerunClearMarks = 1,     // the per-stream overflow / inconsistency marks of the run before are dropped unread (and with them its partial dense streams)
    kRerunMask = 2,           // a masked call's mask rows are built and uploaded again (the rows the scans take have changed)
    kRerunSecondPassOnly = 4, // enqueue_analysis: second_pass_only
    kRerunOwnMeans = 8,       // enqueue_analysis: own_means
    kRerunNoWait = 16,        // the caller enqueues more behind it and calls await_call itself
};
static int await_call(rt_handle *h, Slot &sl, unsigned long long &flags) {
    RT_HIP(h, hipEventSynchronize(sl.ev_done));
    flags = sl.h_counters[2];
    return RT_OK;
}
static int rerun(rt_handle *h, Slot &sl, int mode, unsigned long long &flags, unsigned how = 0) {
    if (how & kRerunClearMarks) {
        for (int s = 0; s < h->cfg.n_streams; ++s) sl.h_overflow[s] = sl.h_incons[s] = 0;
        sl.call.n_dense_streams = 0;
    }
    int rc = before_rerun(h, sl);
    if (rc == RT_OK && (how & kRerunMask) && sl.lc.masked) rc = upload_mask(h, sl);
    if (rc == RT_OK) rc = enqueue_analysis(h, sl, mode, nullptr, (how & kRerunSecondPassOnly) != 0, (how & kRerunOwnMeans) != 0);
    if (rc != RT_OK || (how & kRerunNoWait)) return rc;
    return await_call(h, sl, flags);
}

// fetch_one, step 2: a stream the scans have newly marked for SciPy's order of the detrend has this call (and the one in flight
// behind it) analysed again; `flags` become the re-run's.
static int guard_detrend(rt_handle *h, Slot &sl, unsigned long long &flags) {
    CallCtx &c = sl.call;
    // Guard of the detrend by linearity (rt_kernels.h: StftParams::dc_flag).  The form carries a stream's constant offset through
    // the transform: harmless while the offset is <= 60 dB over the per-sample noise (any <= 16-bit front end; <= 0.02 dB against
    // the oracle), 0.06 - 0.17 dB at 80 dB.  A scan that meets such a stream marks it; from then on that stream -- and only that
    // stream -- is detrended in SciPy's order (_spectral_py.py:2191-2194), and every call whose kernels were enqueued before the
    // mark (this one, and any in flight) is analysed again.
    if (c.ran_lin && !c.is_extract && c.n_seg > 0) {
        bool newly = false;
        for (int s = 0; s < h->cfg.n_streams; ++s) {
            if (sl.h_dc_flag[s] != 0 && !h->h_sub_first[(size_t)s]) {
                h->h_sub_first[(size_t)s] = 1;
                newly = true;
            }
            sl.h_dc_flag[s] = 0;
        }
        if (newly) {
            // (both of the handle's streams drained first, so that no kernel in flight reads the list while it changes)
            RT_HIP(h, hipStreamSynchronize(h->s_scan));
            RT_HIP(h, hipStreamSynchronize(h->s_detect));
            h->n_sub = 0;
            for (int s = 0; s < h->cfg.n_streams; ++s)
                if (h->h_sub_first[(size_t)s]) h->h_sub_list[h->n_sub++] = s;
            RT_HIP(h, hipMemcpy(h->d_sub_first, h->h_sub_first.data(), h->h_sub_first.size() * sizeof(int32_t), hipMemcpyHostToDevice));
            ++h->sub_epoch;
        }
        if (c.sub_epoch != h->sub_epoch) {
            // (the marked streams are part of the mask rows the scans take; the re-run takes the current epoch)
            int rc = rerun(h, sl, c.mode_used, flags, kRerunClearMarks | kRerunMask | kRerunNoWait);
            if (rc != RT_OK) return rc;
            // The call enqueued behind this one (at most one is in flight) was analysed under the old set as well, and the next
            // rt_process will read the look-back columns it wrote: it is analysed again HERE, in sequence order, before anything
            // newer can be enqueued -- not at its own fetch, by which time a newer call's detection would have read the old
            // columns or raced the rewrite (advisor, round 4).  Once per marking.
            for (auto &o : h->slot) {
                if (&o == &sl || !o.call.pending || o.call.seq < c.seq || !o.call.ran_lin || o.call.is_extract || o.call.n_seg <= 0 ||
                    o.call.sub_epoch == h->sub_epoch)
                    continue;
                RT_HIP(h, hipEventSynchronize(o.ev_done));
                for (int s = 0; s < h->cfg.n_streams; ++s) o.h_overflow[s] = o.h_incons[s] = o.h_dc_flag[s] = 0;
                // (its absent streams' look-back columns again as well: the re-run in front of it has rewritten the marked streams' columns
                // in the buffer they were carried from)
                if (o.lc.masked) rc = upload_mask(h, o);
                if (rc == RT_OK && o.lc.masked)
                    rc = enqueue_carry<float>(h, o.d_mask + (size_t)kMaskAbsentList * h->cfg.n_streams, o.n_absent, h->d_tail[o.call.tail_read],
                                              h->d_tail[o.call.tail_write], h->K, h->N);
                if (rc != RT_OK) return rc;
                rc = enqueue_analysis(h, o, o.call.mode_used);  // (behind this call's re-run on s_scan; its scratch is its slot's)
                if (rc != RT_OK) return rc;
            }
            rc = await_call(h, sl, flags);
            if (rc != RT_OK) return rc;
            for (int s = 0; s < h->cfg.n_streams; ++s) sl.h_dc_flag[s] = 0;  // (marked streams mark themselves again: nothing new)
        }
    }
    return RT_OK;
}

// fetch_one, step 3: while the call's analysis does not stand -- candidate lists overflowed (what then: rt_core.h, overflow_step), or
// a capacity or pool was too small -- it is analysed again.  `peek`: see fetch_one.
static int rerun_until_it_stands(rt_handle *h, Slot &sl, unsigned long long &flags, bool peek) {
    CallCtx &c = sl.call;
    const bool can_rerun = !c.is_extract && c.n_seg > 0;  // (rt_extract: the caller's spectrogram is not kept)
    for (;;) {  // (a second round only after something had to grow)
        RT_TRACE_FETCH(h, sl, "round");
        while ((flags & kFlagHotOverflow) && !c.is_extract && c.mode_used != RT_MODE_DENSE) {
            RT_TRACE_FETCH(h, sl, "hot overflow");
            // which streams overflowed?  (the flags are consumed here, whatever happens next)  The scan stops emitting for a
            // stream once one of its lists has overflowed, so a "run without its preceding cell" in such a stream is not an
            // internal error; in any other stream it is.
            int n_bad = 0;
            bool incons_elsewhere = false;
            for (int s = 0; s < h->cfg.n_streams; ++s) {
                if (sl.h_incons[s] && !sl.h_overflow[s]) incons_elsewhere = true;
                sl.h_incons[s] = 0;
                if (sl.h_overflow[s]) {
                    if (n_bad < kMaxPartial) sl.h_list[n_bad] = s;
                    ++n_bad;
                    sl.h_overflow[s] = 0;
                }
            }
            const AutoOverflow step = overflow_step(c.mode_used, c.thr_rerun, (flags & kFlagThrStale) != 0, n_bad, h->cfg.n_streams, h->cfg.mode, h->ap.lv);
            flags &= ~kFlagThrStale;
            if (step == kOverflowOwnMeans) {
                c.thr_rerun = true;
                const int rc = rerun(h, sl, RT_MODE_RUNFILTER, flags, kRerunOwnMeans);
                if (rc != RT_OK) return rc;
                continue;
            }
            if (step == kOverflowFail) {
                h->err = "candidate-cell capacity exceeded (hot_capacity)";
                if (peek) return kCallFailed;  // the laned rt_fetch drops this call in every lane together
                c.pending = false;
                return RT_E_HOT_OVERFLOW;
            }
            if (step == kOverflowPartialDense) {
                const unsigned long long other = flags & ~(kFlagHotOverflow | (incons_elsewhere ? 0ull : kFlagInconsistent));
                const unsigned long long wanted_so_far = sl.h_counters[4];  // (a stream OUTSIDE the few may have outgrown its record capacity)
                int rc = before_rerun(h, sl);
                if (rc == RT_OK) rc = enqueue_partial_dense(h, sl, n_bad, sl.h_counters[0]);
                if (rc == RT_OK) {
                    rc = await_call(h, sl, flags);
                    if (rc != RT_OK) return rc;
                    flags |= other;
                    sl.h_counters[2] = flags;  // (the laned rt_fetch looks at this call twice: sizing, then delivery)
                    // ... and what that stream wanted survives the partial run's own counter words: the record-overflow flag kept in `other`
                    // without it was a truncated delivery (round 6's soak, seed 64 case 56)
                    sl.h_counters[4] = std::max(sl.h_counters[4], wanted_so_far);
                    c.fell_back = true;
                    c.n_dense_streams = n_bad;
                    break;
                }
                // the partial re-run could not be enqueued (its scratch spectrogram did not fit): the whole batch goes one
                // level up instead, which needs no scratch of its own or reports its own failure
                if (rc != RT_E_NOMEM) return rc;
            }
            // Re-run of the same buffer with the same look-back state, one level up.  Its scan queues up behind whatever is in
            // flight on the handle's scan stream and behind the later call's detection (before_rerun: that call read the tail
            // columns this call's first scan already wrote -- the re-run writes the same values); other lanes' streams are left alone.
            const int from = c.mode_used;
            c.mode_used = h->ap.climb(from, !c.fell_back);
            c.fell_back = true;
            const int rc = rerun(h, sl, c.mode_used, flags, from == RT_MODE_SPARSE && c.mode_used == RT_MODE_PREFILTER ? kRerunSecondPassOnly : 0u);
            if (rc != RT_OK) return rc;
        }
        // Something was too small for what the call found; it grows and the call is analysed again on the level it ended on -- same
        // buffer, same look-back state, like a fall-back re-run -- so the caller loses nothing.  Up to three times each per call (a
        // re-run on a higher level, or a partial dense one, may find more).  Where it cannot grow (rt_extract; no memory left) the
        // truncated lists are delivered with RT_E_CAPACITY.
        const char *grown = nullptr;
        int *times = nullptr;
        if ((flags & kFlagRecOverflow) && can_rerun && sl.h_counters[4] > (unsigned long long)c.rec_cap_used && c.cap_grown < 3 &&
            grow_record_capacity(h, sl.h_counters[4]) == RT_OK) {
            // A stream wanted more records than the handle's per-stream capacity holds (word 4) -- the reference has no limit
            // (analyze.py:449-450).  (Measured against the capacity the call's kernels RAN with: with two calls in flight the first one's
            // growth may already cover what the second one wanted -- its lists were still cut at the old capacity.)
            grown = "capacity grown";
            times = &c.cap_grown;
        } else if ((flags & kFlagRecOverflow) && can_rerun && sl.h_counters[0] > (unsigned long long)sl.pool_cap && sl.pool_cap < h->pool_max &&
                   c.pool_grown < 3 && grow_pool(h, sl, (int64_t)std::min<unsigned long long>(sl.h_counters[0], (unsigned long long)h->pool_max)) == RT_OK) {
            // The call found more records than the slot's pinned pool holds (word 0 = records wanted): streams beyond its end got
            // truncated lists.  Later calls find the larger pool.
            grown = "pool grown";
            times = &c.pool_grown;
        } else if (sl.d_cells && can_rerun && sl.h_cells_info[0] > (unsigned long long)sl.cell_cap && c.cells_grown < 3 &&
                   grow_cells(h, sl.d_cells, sl.cell_cap, (int64_t)sl.h_cells_info[0]) == RT_OK) {
            // RT_FLAG_RECORD_CELLS: the call's records hold more cells than the slot's pool (word 0 of the gather's words) -- the
            // gather reads a map that is gone by now.
            grown = "cell pool grown";
            times = &c.cells_grown;
            h->cells_want = std::max(h->cells_want, sl.cell_cap);
        }
        if (!grown) return RT_OK;
        RT_TRACE_FETCH(h, sl, grown);
        ++*times;
        const int rc = rerun(h, sl, c.mode_used, flags, kRerunClearMarks);
        if (rc != RT_OK) return rc;
    }
}

// rt_fetch of one (lane-less) handle: wait for the call, guard its detrend, analyse it again until its result stands, tell the
// AUTO policy, deliver.  `peek`: all but the delivery, and the call stays pending even when it has no records (the laned rt_fetch
// sizes all lanes before it copies).
static int fetch_one(rt_handle *h, rt_record *out, size_t cap, size_t *n_out, bool peek) {
    *n_out = 0;
    Slot *slp = oldest_pending(h);
    if (!slp) {
        h->err = "rt_fetch without a preceding successful rt_process/rt_extract";
        return RT_E_INVALID;
    }
    Slot &sl = *slp;
    CallCtx &c = sl.call;
    RT_HIP(h, hipSetDevice(h->cfg.device));
    unsigned long long flags = 0;
    int rc = await_call(h, sl, flags);
    if (rc != RT_OK) return rc;
    h->info = rt_call_info{};
    h->info.n_seg = c.n_seg;
    h->info.segs_per_chunk = h->L;
    h->info.n_hot = 0;
    rc = guard_detrend(h, sl, flags);
    if (rc == RT_OK) rc = rerun_until_it_stands(h, sl, flags, peek);
    if (rc != RT_OK) return rc;
    RT_TRACE_FETCH(h, sl, "settled");
    if (c.mode_used != RT_MODE_DENSE && !c.is_extract && c.n_seg > 0)
        for (int s = 0; s < h->cfg.n_streams; ++s) h->info.n_hot += sl.h_hot_total[s];
    // one wave per stream in the next calls' sparse detection while a stream holds half of what such a wave takes on average (heavier
    // batches -- BASELINE config 4: 1 500 cells per stream -- are faster with the per-list waves: most of their streams would be left to them anyway)
    // (a call with a presence mask: the streams that took part -- an absent one adds nothing to either side of these ratios)
    const int64_t n_took_part = sl.lc.masked ? sl.lc.pc.n_present : h->cfg.n_streams;
    if (c.mode_used != RT_MODE_DENSE && !c.is_extract && c.n_seg > 0) h->group_light = h->info.n_hot * 2 <= (int64_t)kGroupCells * n_took_part;
    h->ap.settle(c.level_settled, h->cfg.mode, c.mode_used, c.fell_back, !c.is_extract && c.n_seg > 0, h->info.n_hot, sl.h_seg_total ? (int64_t)*sl.h_seg_total : -1,
                 n_took_part, c.n_seg, h->N);
    c.level_settled = true;
    if (flags & kFlagInconsistent) {
        std::memset(sl.h_incons, 0, (size_t)h->cfg.n_streams * sizeof(int32_t));
        h->err = "internal: candidate list lacks the cell preceding a run";
        if (peek) return kCallFailedInternal;
        c.pending = false;
        return RT_E_HIP;
    }
    if (h->timing && c.n_seg > 0) {
        (void)hipEventElapsedTime(&h->info.ms_stft, sl.ev_begin, sl.ev_scan);
        (void)hipEventElapsedTime(&h->info.ms_detect, sl.ev_scan, sl.ev_done);
        (void)hipEventElapsedTime(&h->info.ms_total, sl.ev_begin, sl.ev_done);
    }
    h->ap.keep_abs_hot(c.abs_counted && sl.h_abs_hot, sl.h_abs_hot ? *sl.h_abs_hot : 0u, c.mode_used, c.n_dense_streams);
    h->info.mode_used = c.mode_used;
    h->info.fell_back = c.fell_back ? 1 : 0;
    h->info.n_dense_streams = c.n_dense_streams;

    const int S = h->cfg.n_streams;
    size_t total = 0;
    for (int s = 0; s < S; ++s) total += (size_t)sl.h_rec_count[s];
    h->info.n_records = (int64_t)total;
    *n_out = total;
    if (peek) {
        // nothing is delivered
    } else if (total && out && cap) {
        size_t w = 0;
        for (int s = 0; s < S && w < cap; ++s) {
            const int n = sl.h_rec_count[s];
            const int off = sl.h_rec_offset[s];
            for (int i = 0; i < n && w < cap; ++i) out[w++] = sl.h_records[(size_t)off + i];
        }
        c.pending = false;  // delivered
    } else if (total == 0) {
        c.pending = false;  // nothing to deliver
    }
    if (!peek && !c.pending) {
        keep_row_means(h, sl);
        h->cells_full = cap >= total && !(flags & kFlagRecOverflow);  // (rt_fetch_record_cells: only of a call delivered in full)
        if (h->riq) {
            // rt_fetch_record_iq: the record list stands (every re-run is behind us) and the call's IQ is still the caller's to keep
            RecordIq &q = *h->riq;
            if (c.is_extract) {
                q.delivered = kIqExtract;
            } else if (!sl.lc.iq_on) {
                q.delivered = kIqOff;
            } else if (!h->cells_full) {
                q.delivered = kIqTruncated;
            } else {
                std::vector<int32_t> keys;  // stream, fi, start, end of every record, in delivery order
                keys.reserve(total * 4);
                for (int s = 0; s < S; ++s) {
                    const rt_record *r = sl.h_records + sl.h_rec_offset[s];
                    for (int i = 0; i < sl.h_rec_count[s]; ++i) keys.insert(keys.end(), {(int32_t)s, r[i].fi, r[i].start, r[i].end});
                }
                iq_gather(h, (int)(&sl - h->slot), sl.lc.iq, keys.data(), 4 * sizeof(int32_t), total, c.iq, c.stream_stride);
            }
        }
    }
    // (out == NULL / cap == 0 with records available is a size query: the call stays pending)
    if (flags & kFlagRecOverflow) {
        h->err = "record capacity exceeded (record_capacity per stream, or the record pool could not grow); results truncated";
        return RT_E_CAPACITY;
    }
    return RT_OK;
}

int rt_fetch(rt_handle *h, rt_record *out, size_t cap, size_t *n_out) {
    if (!h || !n_out) return RT_E_INVALID;
    if (h->f64) return refuse_on_f64(h, "rt_fetch", "rt_fetch_f64");
    if (h->kids.empty()) return fetch_one(h, out, cap, n_out, false);
    // lanes: size every lane first (a size query must leave all of them pending), then deliver in
    // stream order with the lane's first stream added to the records' stream index
    *n_out = 0;
    int truncated = RT_OK;
    size_t total = 0;
    int failed = RT_OK;
    std::vector<size_t> lane_records;  // what every lane holds for this call
    for (rt_handle *k : h->kids) {
        size_t n = 0;
        const int rc = fetch_one(k, nullptr, 0, &n, true);
        if (rc != RT_OK && rc != RT_E_CAPACITY && failed == RT_OK) {
            h->err = k->err;
            failed = (rc == kCallFailed) ? RT_E_HOT_OVERFLOW : (rc == kCallFailedInternal) ? RT_E_HIP : rc;
        }
        total += n;
        lane_records.push_back(n);
    }
    if (failed != RT_OK) {
        // one lane has no result for this call: the call is dropped in every lane, so that the lanes stay in step
        // (the next rt_fetch belongs to the next rt_process in all of them)
        for (rt_handle *k : h->kids) discard_oldest(k);
        *n_out = 0;
        return failed;
    }
    *n_out = total;
    h->info = rt_call_info{};
    const bool deliver = !(total && (!out || !cap));
    size_t w = 0;
    for (size_t i = 0; i < h->kids.size(); ++i) {
        rt_handle *k = h->kids[i];
        if (deliver && total && cap <= w && lane_records[i]) {
            // the caller's buffer is full: this lane's records are lost, but the call is consumed here as in the
            // lanes before it -- otherwise the lanes would be out of step from the next rt_fetch on.  (A lane WITHOUT records
            // behind a buffer of exactly the call's size loses nothing: it is delivered in full below, and its cells stand.)
            if (const Slot *o = oldest_pending(k)) keep_row_means(k, *o);  // (delivered, if not in full: its row means stand)
            k->cells_full = false;
            if (k->riq) k->riq->delivered = kIqTruncated;
            discard_oldest(k);
        } else if (deliver) {
            size_t n = 0;
            const int rc = fetch_one(k, out ? out + w : nullptr, cap > w ? cap - w : 0, &n, false);
            if (rc == RT_E_CAPACITY) {
                truncated = rc;
                h->err = k->err;
            } else if (rc != RT_OK) {
                h->err = k->err;
                return rc;
            }
            const size_t got = (cap > w) ? (n < cap - w ? n : cap - w) : 0;
            if (out)
                for (size_t j = 0; j < got; ++j) out[w + j].stream += h->kid_base[i];
            w += got;
        }
        const rt_call_info &ki = k->info;
        h->info.n_seg = ki.n_seg;
        h->info.segs_per_chunk = ki.segs_per_chunk;
        h->info.mode_used = i == 0 ? ki.mode_used : (ki.mode_used < h->info.mode_used ? ki.mode_used : h->info.mode_used);
        h->info.fell_back |= ki.fell_back;
        h->info.n_dense_streams += ki.n_dense_streams;
        h->info.n_hot += ki.n_hot;
        h->info.n_records += ki.n_records;
        h->info.ms_stft += ki.ms_stft;      // sums over the lanes' launches (they overlap in time)
        h->info.ms_detect += ki.ms_detect;
        h->info.ms_total += ki.ms_total;
    }
    return truncated;
}

int rt_spectrogram(rt_handle *h, const void *iq_dev, int64_t n_samples, int64_t stream_stride, float *spec_dev) {
    if (!h || !iq_dev || !spec_dev) return RT_E_INVALID;
    if (h->f64) return refuse_on_f64(h, "rt_spectrogram", "rt_spectrogram_f64");
    if (!h->kids.empty())
        return for_each_lane(h, [&](rt_handle *k, int64_t s0) {
            const int64_t T = n_samples / k->N;
            return rt_spectrogram(k, static_cast<const char *>(iq_dev) + s0 * stream_stride * (int64_t)sizeof(cf), n_samples,
                                  stream_stride, spec_dev + s0 * T * k->N);
        });
    if (n_samples < 0 || n_samples > h->cfg.max_samples || stream_stride < n_samples ||
        reinterpret_cast<uintptr_t>(iq_dev) % 8u != 0 || reinterpret_cast<uintptr_t>(spec_dev) % 4u != 0) {
        h->err = "n_samples/stream_stride out of range for this handle, or misaligned pointer";
        return RT_E_INVALID;
    }
    RT_HIP(h, hipSetDevice(h->cfg.device));
    const int T = (int)(n_samples / h->N);
    if (T == 0) return RT_OK;
    RT_HIP(h, hipDeviceSynchronize());
    if (h->general) {
        launch_general(h, iq_dev, stream_stride, T, spec_dev, nullptr, false);
        RT_HIP(h, hipGetLastError());
        RT_HIP(h, hipStreamSynchronize(h->s_scan));
        return RT_OK;
    }
    StftParams sp = make_stft_params(h, h->slot[0], iq_dev, stream_stride, T, 0);
    sp.spec = spec_dev;
    launch_stft<2>(h, sp, h->cfg.n_streams * sp.blocks_per_stream, h->s_scan);
    if (h->lin)  // (the map scan has no guard of the detrend by linearity: rt_kernels.h)
        hipLaunchKernelGGL(nan_columns_of_nonfinite_segments, dim3((unsigned)((int64_t)h->cfg.n_streams * T)), dim3(256), 0, h->s_scan,
                           static_cast<const float2 *>(iq_dev), stream_stride, T, h->N, spec_dev);
    RT_HIP(h, hipGetLastError());
    RT_HIP(h, hipStreamSynchronize(h->s_scan));
    return RT_OK;
}

int rt_calibrate_read(rt_handle *h, const void *iq_dev, int64_t n_samples, int64_t stream_stride) {
    if (!h || !iq_dev) return RT_E_INVALID;
    if (h->f64) return refuse_on_f64(h, "rt_calibrate_read", nullptr);
    if (!h->kids.empty())
        return for_each_lane(h, [&](rt_handle *k, int64_t s0) {
            return rt_calibrate_read(k, static_cast<const char *>(iq_dev) + s0 * stream_stride * (int64_t)sizeof(cf), n_samples,
                                     stream_stride);
        });
    if (n_samples < 0 || n_samples > h->cfg.max_samples || stream_stride < n_samples || reinterpret_cast<uintptr_t>(iq_dev) % 8u != 0) {
        h->err = "n_samples/stream_stride out of range for this handle, or misaligned pointer";
        return RT_E_INVALID;
    }
    RT_HIP(h, hipSetDevice(h->cfg.device));
    const int T = (int)(n_samples / h->N);
    if (h->general || h->big) {
        h->err = "rt_calibrate_read: the load stream of the fused scans of nperseg 32 ... 4096 only";
        return RT_E_UNSUPPORTED;
    }
    if (T < 2) return RT_OK;
    RT_HIP(h, hipDeviceSynchronize());
    StftParams sp = make_stft_params(h, h->slot[0], iq_dev, stream_stride, T, 0);
    launch_stft<3>(h, sp, h->cfg.n_streams * sp.blocks_per_stream, h->s_scan);
    RT_HIP(h, hipGetLastError());
    RT_HIP(h, hipStreamSynchronize(h->s_scan));
    return RT_OK;
}

// rt_fetch_row_means / _f64 (include/rt_analyze.h): the checks both make; `rm_slot` is the lane-less handle's (or the float64 state's)
static int row_means_refused(rt_handle *h, const void *out, size_t n, int rm_slot) {
    const char *why = nullptr;
    if (!out) why = "null output";
    else if (!(h->cfg.flags & RT_FLAG_ROW_MEANS)) why = "the handle was created without RT_FLAG_ROW_MEANS";
    else if (n != (size_t)h->cfg.n_streams * (size_t)h->cfg.nperseg) why = "n must be n_streams * nperseg";
    else if (rm_slot == kRowMeansExtract) why = "the call fetched last was an rt_extract: the caller holds its spectrogram";
    else if (rm_slot < 0) why = "no row means: no call delivered by rt_fetch since the last rt_process*, rt_extract or rt_reset";
    if (!why) return RT_OK;
    h->err = std::string("rt_fetch_row_means: ") + why;
    return RT_E_INVALID;
}

int rt_fetch_row_means(rt_handle *h, float *out, size_t n) {
    if (!h) return RT_E_INVALID;
    if (h->f64) return refuse_on_f64(h, "rt_fetch_row_means", "rt_fetch_row_means_f64");
    if (!h->kids.empty()) {
        // every lane holds the row means of its streams: all of them are checked before anything is written
        int rc = row_means_refused(h, out, n, 0);
        for (size_t k = 0; k < h->kids.size() && rc == RT_OK; ++k) {
            rt_handle *kid = h->kids[k];
            rc = row_means_refused(kid, out, (size_t)kid->cfg.n_streams * (size_t)kid->cfg.nperseg, kid->rm_slot);
            if (rc != RT_OK) h->err = kid->err;
        }
        if (rc != RT_OK) return rc;
        for (size_t k = 0; k < h->kids.size(); ++k) {
            rt_handle *kid = h->kids[k];
            rc = rt_fetch_row_means(kid, out + (size_t)h->kid_base[k] * (size_t)h->cfg.nperseg, (size_t)kid->cfg.n_streams * (size_t)kid->cfg.nperseg);
            if (rc != RT_OK) {
                h->err = kid->err;
                return rc;
            }
        }
        return RT_OK;
    }
    const int rc = row_means_refused(h, out, n, h->rm_slot);
    if (rc != RT_OK) return rc;
    const Slot &sl = h->slot[h->rm_slot];
    if (sl.call.n_seg == 0) {
        std::fill(out, out + n, std::numeric_limits<float>::quiet_NaN());  // np.mean of an empty row
        return RT_OK;
    }
    // The kernel wrote the slot's buffer before the call's ev_done, which the delivering rt_fetch waited for.  A copy on the null
    // stream, which does not wait for the handle's (non-blocking) streams: the next call's kernels run on.  (Written into pinned
    // host memory by the kernel instead, like the records, the row means cost 2.6 % at the reference's defaults and 8 % at
    // config 5's share: 4 / 16 MB a call over the host link, behind the call's detection -- DESIGN.md section 4.10.)
    RT_HIP(h, hipSetDevice(h->cfg.device));
    RT_HIP(h, hipMemcpy(out, sl.d_row_means, n * sizeof(float), hipMemcpyDeviceToHost));
    return RT_OK;
}

// ---- rt_fetch_record_cells / _f64 (include/rt_analyze.h) ----
// the checks both entries make on a lane-less handle (or a lane); `rm_slot` / `full`: the handle's, or the float64 state's
static int record_cells_refused(rt_handle *h, int rm_slot, bool full) {
    const char *why = nullptr;
    if (!(h->cfg.flags & RT_FLAG_RECORD_CELLS)) why = "the handle was created without RT_FLAG_RECORD_CELLS";
    else if (rm_slot == kRowMeansExtract) why = "the call fetched last was an rt_extract: the caller holds its spectrogram";
    else if (rm_slot < 0) why = "no cells: no call delivered by rt_fetch since the last rt_process*, rt_extract or rt_reset";
    else if (!full) why = "the call fetched last was delivered truncated";
    if (!why) return RT_OK;
    h->err = std::string("rt_fetch_record_cells: ") + why;
    return RT_E_INVALID;
}

// what the gather left for a delivered call of `total` cells: the pool could not grow, or a record's cells were not on its list
static int record_cells_state(rt_handle *h, const unsigned long long *info, int64_t cell_cap, size_t total) {
    if (total == 0) return RT_OK;
    if (info[0] > (unsigned long long)cell_cap) {
        h->err = "rt_fetch_record_cells: the cell pool could not grow to " + std::to_string(info[0]) + " cells";
        return RT_E_NOMEM;
    }
    if (info[1] != 0ull || info[0] != (unsigned long long)total) {
        h->err = "internal: a record's cells are not all on its candidate list";
        return RT_E_HIP;
    }
    return RT_OK;
}

// records / cells of the call a lane-less float32 handle delivered last (its slot's result arrays stand until the slot's next call)
static void record_cells_count(const Slot &sl, int S, size_t *n_rec, size_t *n_cells) {
    size_t nr = 0, nc = 0;
    for (int s = 0; s < S; ++s) {
        const rt_record *r = sl.h_records + sl.h_rec_offset[s];
        for (int i = 0; i < sl.h_rec_count[s]; ++i) nc += (size_t)(r[i].end - r[i].start);
        nr += (size_t)sl.h_rec_count[s];
    }
    *n_rec = nr;
    *n_cells = nc;
}

// ... its offsets behind `base` cells (offsets[0] is the caller's), and its cells
static int record_cells_deliver(rt_handle *h, int64_t *offsets, int64_t base, float *cells, size_t n_cells) {
    const Slot &sl = h->slot[h->rm_slot];
    if (offsets) {
        size_t w = 0;
        for (int s = 0; s < h->cfg.n_streams; ++s) {
            const rt_record *r = sl.h_records + sl.h_rec_offset[s];
            for (int i = 0; i < sl.h_rec_count[s]; ++i) {
                base += r[i].end - r[i].start;
                offsets[++w] = base;
            }
        }
    }
    if (cells && n_cells) {
        // (the gather ran before the call's ev_done, which the delivering rt_fetch waited for; a copy on the null stream, as
        // rt_fetch_row_means copies: the next call's kernels run on)
        RT_HIP(h, hipSetDevice(h->cfg.device));
        RT_HIP(h, hipMemcpy(cells, sl.d_cells, n_cells * sizeof(float), hipMemcpyDeviceToHost));
    }
    return RT_OK;
}

int rt_fetch_record_cells(rt_handle *h, int64_t *offsets, size_t n_offsets, float *cells, size_t cap, size_t *n_cells) {
    if (!h || !n_cells) return RT_E_INVALID;
    *n_cells = 0;
    if (h->f64) return refuse_on_f64(h, "rt_fetch_record_cells", "rt_fetch_record_cells_f64");
    std::vector<rt_handle *> one{h};
    const std::vector<rt_handle *> &lanes = h->kids.empty() ? one : h->kids;
    if (!(h->cfg.flags & RT_FLAG_RECORD_CELLS)) return record_cells_refused(h, 0, true);
    // every lane holds the cells of its streams: all of them are checked and counted before anything is written
    std::vector<size_t> n_rec(lanes.size()), n_cell(lanes.size());
    size_t records = 0, total = 0;
    for (size_t k = 0; k < lanes.size(); ++k) {
        rt_handle *l = lanes[k];
        int rc = record_cells_refused(l, l->rm_slot, l->cells_full);
        if (rc == RT_OK) {
            const Slot &sl = l->slot[l->rm_slot];
            record_cells_count(sl, l->cfg.n_streams, &n_rec[k], &n_cell[k]);
            rc = record_cells_state(l, sl.h_cells_info, sl.cell_cap, n_cell[k]);
        }
        if (rc != RT_OK) {
            h->err = l->err;
            return rc;
        }
        records += n_rec[k];
        total += n_cell[k];
    }
    if (offsets && n_offsets != records + 1) {
        h->err = "rt_fetch_record_cells: n_offsets must be the number of records the last rt_fetch delivered, plus one";
        return RT_E_INVALID;
    }
    *n_cells = total;
    const bool query = !cells || cap == 0;
    if (!query && cap < total) {
        h->err = "rt_fetch_record_cells: output buffer too small";
        return RT_E_CAPACITY;
    }
    if (offsets) offsets[0] = 0;
    size_t r0 = 0, c0 = 0;
    for (size_t k = 0; k < lanes.size(); ++k) {
        const int rc = record_cells_deliver(lanes[k], offsets ? offsets + r0 : nullptr, (int64_t)c0, query ? nullptr : cells + c0, n_cell[k]);
        if (rc != RT_OK) {
            h->err = lanes[k]->err;
            return rc;
        }
        r0 += n_rec[k];
        c0 += n_cell[k];
    }
    return RT_OK;
}

// rt_set_record_iq of one lane-less handle (float32 or float64): the first call with a margin makes the gather's stream and the
// slots' pinned rows; the tail area follows with the first rt_process* (its size depends on the format).
static int set_record_iq_one(rt_handle *h, int32_t m) {
    const int S = h->cfg.n_streams, K = h->f64 ? h->f64->K : h->K;
    h->iq_margin = m < 0 ? -1 : m;
    if (m < 0) {
        h->ledger.set_iq_margin(K, -1);
        if (h->riq) h->riq->delivered = kIqNone;
        return RT_OK;
    }
    RT_HIP(h, hipSetDevice(h->cfg.device));
    if (!h->riq) {
        h->riq = new (std::nothrow) RecordIq();
        bool ok = h->riq && hipStreamCreateWithFlags(&h->riq->s_gather, hipStreamNonBlocking) == hipSuccess;
        for (int i = 0; i < kSlots && ok; ++i)
            ok = hipHostMalloc(&h->riq->slot[i].h_rows, (size_t)S * sizeof(int32_t)) == hipSuccess &&
                 hipMalloc(&h->riq->slot[i].d_rows, (size_t)S * sizeof(int32_t)) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            iq_free(h);
            h->iq_margin = -1;
            h->err = "rt_set_record_iq: no memory for the rows of the sample tails";
            return RT_E_NOMEM;
        }
        h->ledger.set_iq_margin(K, m);
    } else if (h->ledger.iq.margin != m) {
        // another margin is another row length: the area is made again by the next rt_process*, the held tails are forgotten
        RT_HIP(h, hipStreamSynchronize(h->s_scan));
        (void)hipFree(h->riq->d_tails);
        h->riq->d_tails = nullptr;
        h->riq->row_bytes = 0;
        h->riq->area_bps = 0;
        h->ledger.set_iq_margin(K, m);
    }
    h->riq->delivered = kIqNone;
    return RT_OK;
}

int rt_set_record_iq(rt_handle *h, int32_t margin_segments) {
    if (!h) return RT_E_INVALID;
    if (margin_segments > kIqMaxMargin) {
        h->err = "rt_set_record_iq: margin_segments must be <= " + std::to_string(kIqMaxMargin);
        return RT_E_INVALID;
    }
    bool pending = false;
    if (h->f64) {
        for (const F64Slot &sl : h->f64->slot) pending = pending || sl.pending;
    } else {
        pending = h->kids.empty() && oldest_pending(h);
        for (rt_handle *k : h->kids) pending = pending || oldest_pending(k);
    }
    if (pending) {
        h->err = "rt_set_record_iq with unfetched calls pending: fetch them first";
        return RT_E_INVALID;
    }
    if (!h->kids.empty()) {
        const int rc = for_each_lane(h, [&](rt_handle *k, int64_t) { return set_record_iq_one(k, margin_segments); });
        h->iq_margin = (rc == RT_OK && margin_segments >= 0) ? margin_segments : -1;
        if (rc != RT_OK)
            for (rt_handle *k : h->kids) (void)set_record_iq_one(k, -1);  // (no lane keeps what another could not get)
        return rc;
    }
    return set_record_iq_one(h, margin_segments);
}

int rt_fetch_record_iq(rt_handle *h, int64_t *offsets, size_t n_offsets, int32_t *first_seg, size_t n_first, void *iq, size_t cap_bytes,
                       size_t *n_bytes, int32_t *bytes_per_sample) {
    if (!h || !n_bytes || !bytes_per_sample) return RT_E_INVALID;
    *n_bytes = 0;
    *bytes_per_sample = 0;
    std::vector<rt_handle *> lanes;
    size_t records = 0, samples = 0;
    int bps = 0;
    const int rc = iq_delivered_call(h, "rt_fetch_record_iq", &lanes, &records, &samples, &bps);
    if (rc != RT_OK) return rc;
    if ((offsets && n_offsets != records + 1) || (first_seg && n_first != records)) {
        h->err = "rt_fetch_record_iq: n_offsets must be the number of records the last rt_fetch delivered plus one, n_first that number";
        return RT_E_INVALID;
    }
    *n_bytes = samples * (size_t)bps;
    *bytes_per_sample = bps;
    const bool query = !iq || cap_bytes == 0;
    if (!query && cap_bytes < *n_bytes) {
        h->err = "rt_fetch_record_iq: output buffer too small";
        return RT_E_CAPACITY;
    }
    size_t r0 = 0, s0 = 0;
    if (offsets) offsets[0] = 0;
    for (rt_handle *l : lanes) {
        const IqSlot &qs = l->riq->slot[l->riq->delivered];
        const size_t n = qs.first_seg.size(), mine = (size_t)qs.offsets.back();
        if (offsets)
            for (size_t i = 0; i < n; ++i) offsets[r0 + i + 1] = (int64_t)s0 + qs.offsets[i + 1];
        if (first_seg && n) std::memcpy(first_seg + r0, qs.first_seg.data(), n * sizeof(int32_t));
        if (!query && mine) {
            // (the gather was waited for inside the delivering rt_fetch; a copy on the null stream, as rt_fetch_record_cells copies)
            RT_HIP(h, hipSetDevice(l->cfg.device));
            RT_HIP(h, hipMemcpy(static_cast<char *>(iq) + s0 * (size_t)bps, qs.d_pool, mine * (size_t)bps, hipMemcpyDeviceToHost));
        }
        r0 += n;
        s0 += mine;
    }
    return RT_OK;
}

int rt_fetch_record_stft(rt_handle *h, int64_t *offsets, size_t n_offsets, int32_t *first_seg, size_t n_first, float *values, size_t cap_cells,
                         size_t *n_cells) {
    return fetch_record_frames<float>(h, "rt_fetch_record_stft", "rt_fetch_record_stft_f64", kProdStft, record_stft_run<float>, false, 1, 0, offsets,
                                      n_offsets, first_seg, n_first, values, cap_cells, n_cells);
}

int rt_fetch_record_stft_f64(rt_handle *h, int64_t *offsets, size_t n_offsets, int32_t *first_seg, size_t n_first, double *values,
                             size_t cap_cells, size_t *n_cells) {
    return fetch_record_frames<double>(h, "rt_fetch_record_stft_f64", "rt_fetch_record_stft", kProdStft, record_stft_run<double>, false, 1, 0, offsets,
                                       n_offsets, first_seg, n_first, values, cap_cells, n_cells);
}

int rt_fetch_record_stft_hop(rt_handle *h, int32_t hop_div, int64_t *offsets, size_t n_offsets, int32_t *first_seg, size_t n_first, float *values,
                             size_t cap_frames, size_t *n_frames) {
    return fetch_record_frames<float>(h, "rt_fetch_record_stft_hop", "rt_fetch_record_stft_hop_f64", kProdHop, record_stft_hop_run<float>, false, hop_div, 0,
                                      offsets, n_offsets, first_seg, n_first, values, cap_frames, n_frames);
}

int rt_fetch_record_stft_hop_f64(rt_handle *h, int32_t hop_div, int64_t *offsets, size_t n_offsets, int32_t *first_seg, size_t n_first, double *values,
                                 size_t cap_frames, size_t *n_frames) {
    return fetch_record_frames<double>(h, "rt_fetch_record_stft_hop_f64", "rt_fetch_record_stft_hop", kProdHop, record_stft_hop_run<double>, false, hop_div, 0,
                                       offsets, n_offsets, first_seg, n_first, values, cap_frames, n_frames);
}

int rt_fetch_record_band(rt_handle *h, int32_t hop_div, int32_t half_width, int64_t *offsets, size_t n_offsets, int32_t *first_seg, size_t n_first,
                         float *values, size_t cap_frames, size_t *n_frames) {
    return fetch_record_frames<float>(h, "rt_fetch_record_band", "rt_fetch_record_band_f64", kProdBand, record_band_run<float>, true, hop_div, half_width,
                                      offsets, n_offsets, first_seg, n_first, values, cap_frames, n_frames);
}

int rt_fetch_record_band_f64(rt_handle *h, int32_t hop_div, int32_t half_width, int64_t *offsets, size_t n_offsets, int32_t *first_seg, size_t n_first,
                             double *values, size_t cap_frames, size_t *n_frames) {
    return fetch_record_frames<double>(h, "rt_fetch_record_band_f64", "rt_fetch_record_band", kProdBand, record_band_run<double>, true, hop_div, half_width,
                                       offsets, n_offsets, first_seg, n_first, values, cap_frames, n_frames);
}

int rt_fetch_record_estimates(rt_handle *h, int32_t hop_div, rt_record_estimate *out, size_t cap, size_t *n_out) {
    return fetch_record_rows(h, "rt_fetch_record_estimates", kProdEst, record_estimates_run<float>, record_estimates_run<double>, false, hop_div, 0,
                             !out || cap == 0, cap, n_out, [&](const char *pool, size_t r0, size_t n) {
                                 return hipMemcpy(out + r0, pool, n * sizeof(rt_record_estimate), hipMemcpyDeviceToHost);
                             });
}

int rt_fetch_record_spectrum(rt_handle *h, int32_t hop_div, int32_t half_width, rt_record_spectrum *rows, double *mean, double *peak, size_t cap,
                             size_t *n_out) {
    // (a lane's pool: its rows, then its means, then its peaks -- spectrum_pool_bytes)
    return fetch_record_rows(h, "rt_fetch_record_spectrum", kProdSpec, record_spectrum_run<float>, record_spectrum_run<double>, true, hop_div, half_width,
                             !rows || cap == 0, cap, n_out, [&](const char *pool, size_t r0, size_t n) {
                                 const size_t B = (size_t)stft_band_columns(half_width);
                                 const size_t row_bytes = n * sizeof(rt_record_spectrum), col_bytes = n * B * sizeof(double);
                                 hipError_t e = hipMemcpy(rows + r0, pool, row_bytes, hipMemcpyDeviceToHost);
                                 if (e == hipSuccess && mean) e = hipMemcpy(mean + r0 * B, pool + row_bytes, col_bytes, hipMemcpyDeviceToHost);
                                 if (e == hipSuccess && peak) e = hipMemcpy(peak + r0 * B, pool + row_bytes + col_bytes, col_bytes, hipMemcpyDeviceToHost);
                                 return e;
                             });
}

// ---- rt_set_input_stats / rt_fetch_input_stats (include/rt_analyze.h) ----
static int set_input_stats_one(rt_handle *h, bool on) {
    if (h->ist)
        for (InputStatsSlot &qs : h->ist->slot) qs.seq = 0;  // (whatever rows the slots hold are no delivered call's any more)
    if (!on) {
        if (h->ist) h->ist->on = false;
        return RT_OK;
    }
    if (!h->ist) {
        RT_HIP(h, hipSetDevice(h->cfg.device));
        InputStatsState *q = new (std::nothrow) InputStatsState();
        const size_t S = (size_t)h->cfg.n_streams;
        bool ok = q != nullptr;
        if (ok) q->max_chunks = (int)std::max<int64_t>(1, (h->cfg.max_samples + kInputStatsChunk - 1) / kInputStatsChunk);
        for (int i = 0; i < kSlots && ok; ++i)
            ok = hipMalloc(&q->slot[i].d_parts, S * (size_t)q->max_chunks * sizeof(InputStatsPart<double>)) == hipSuccess &&
                 hipHostMalloc(reinterpret_cast<void **>(&q->slot[i].h_rows), S * sizeof(rt_input_stats)) == hipSuccess;
        h->ist = q;
        if (!ok) {
            (void)hipGetLastError();
            input_stats_free(h);
            h->err = "rt_set_input_stats: no memory for the partial rows and the pinned rows";
            return RT_E_NOMEM;
        }
    }
    h->ist->on = true;
    return RT_OK;
}

int rt_set_input_stats(rt_handle *h, int32_t on) {
    if (!h) return RT_E_INVALID;
    bool pending = false;
    if (h->f64) {
        for (const F64Slot &sl : h->f64->slot) pending = pending || sl.pending;
    } else {
        pending = h->kids.empty() && oldest_pending(h);
        for (rt_handle *k : h->kids) pending = pending || oldest_pending(k);
    }
    if (pending) {
        h->err = "rt_set_input_stats with unfetched calls pending: fetch them first";
        return RT_E_INVALID;
    }
    if (!h->kids.empty()) {
        const int rc = for_each_lane(h, [&](rt_handle *k, int64_t) { return set_input_stats_one(k, on != 0); });
        if (rc != RT_OK)
            for (rt_handle *k : h->kids) (void)set_input_stats_one(k, false);  // (no lane keeps what another could not get)
        return rc;
    }
    return set_input_stats_one(h, on != 0);
}

// why a lane-less handle (or a lane) has no rows to hand out, or null: *slot holds them
static const char *input_stats_refused(const rt_handle *h, int *slot) {
    const InputStatsState *q = h->ist;
    if (!q || !q->on) return "the feature is off (rt_set_input_stats)";
    const int rm = h->f64 ? h->f64->rm_slot : h->rm_slot;
    if (rm == kRowMeansExtract) return "the call fetched last was an rt_extract: it has no input";
    if (rm < 0) return "no call delivered by rt_fetch since the last rt_process*, rt_extract, rt_reset or rt_set_input_stats";
    const uint64_t seq = h->f64 ? h->f64->slot[rm].seq : h->slot[rm].call.seq;
    if (q->slot[rm].seq == 0 || q->slot[rm].seq != seq) return "the call fetched last was enqueued before the feature was on";
    *slot = rm;
    return nullptr;
}

int rt_fetch_input_stats(rt_handle *h, rt_input_stats *out, size_t n) {
    if (!h) return RT_E_INVALID;
    const char *why = nullptr;
    if (!out) why = "null output";
    else if (n != (size_t)h->cfg.n_streams) why = "n must be n_streams";
    // every lane is checked before anything is written
    std::vector<rt_handle *> lanes = h->kids;
    if (lanes.empty()) lanes.push_back(h);
    std::vector<int> slots(lanes.size(), 0);
    for (size_t i = 0; i < lanes.size() && !why; ++i) why = input_stats_refused(lanes[i], &slots[i]);
    if (why) {
        h->err = std::string("rt_fetch_input_stats: ") + why;
        return RT_E_INVALID;
    }
    // (the fold wrote the pinned rows in front of the call's scan, and the delivering rt_fetch waited for the call's end)
    size_t s0 = 0;
    for (size_t i = 0; i < lanes.size(); ++i) {
        const size_t S = (size_t)lanes[i]->cfg.n_streams;
        std::memcpy(out + s0, lanes[i]->ist->slot[slots[i]].h_rows, S * sizeof(rt_input_stats));
        s0 += S;
    }
    return RT_OK;
}

int rt_get_call_info(rt_handle *h, rt_call_info *info) {
    if (!h || !info) return RT_E_INVALID;
    *info = h->info;
    return RT_OK;
}

int rt_dev_alloc(int32_t device, size_t bytes, void **out) {
    if (!out) return RT_E_INVALID;
    *out = nullptr;
    if (hipSetDevice(device) != hipSuccess) return fail_create(RT_E_NO_DEVICE, "hipSetDevice failed");
    hipError_t e = hipMalloc(out, bytes ? bytes : 4);
    if (e != hipSuccess) return fail_create(RT_E_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
    return RT_OK;
}

int rt_dev_free(int32_t device, void *ptr) {
    if (hipSetDevice(device) != hipSuccess) return fail_create(RT_E_NO_DEVICE, "hipSetDevice failed");
    hipError_t e = hipFree(ptr);
    return e == hipSuccess ? RT_OK : fail_create(RT_E_HIP, std::string("hipFree: ") + hipGetErrorString(e));
}

int rt_dev_upload(int32_t device, void *dst_dev, const void *src_host, size_t bytes) {
    if (hipSetDevice(device) != hipSuccess) return fail_create(RT_E_NO_DEVICE, "hipSetDevice failed");
    hipError_t e = hipMemcpy(dst_dev, src_host, bytes, hipMemcpyHostToDevice);
    return e == hipSuccess ? RT_OK : fail_create(RT_E_HIP, std::string("hipMemcpy H2D: ") + hipGetErrorString(e));
}

int rt_dev_download(int32_t device, void *dst_host, const void *src_dev, size_t bytes) {
    if (hipSetDevice(device) != hipSuccess) return fail_create(RT_E_NO_DEVICE, "hipSetDevice failed");
    hipError_t e = hipMemcpy(dst_host, src_dev, bytes, hipMemcpyDeviceToHost);
    return e == hipSuccess ? RT_OK : fail_create(RT_E_HIP, std::string("hipMemcpy D2H: ") + hipGetErrorString(e));
}

}  // extern "C"

// ---- float64 handles (include/rt_analyze.h: rt_create_f64; kernels: rt_f64.h) ----
namespace {

int f64_err(rt_handle *h, int code, const std::string &msg) {
    h->err = msg;
    return code;
}

F64Slot *f64_oldest(F64State *f) {
    F64Slot *best = nullptr;
    for (F64Slot &sl : f->slot)
        if (sl.pending && (!best || sl.seq < best->seq)) best = &sl;
    return best;
}

// a slot for the next call: a free one, else the older pending call is dropped (a third call without a fetch)
F64Slot &f64_claim(F64State *f) {
    for (F64Slot &sl : f->slot)
        if (!sl.pending) return sl;
    F64Slot *o = f64_oldest(f);
    o->pending = false;
    return *o;
}

// a slot's record areas for `cap` records per stream (a slot holds no call while this runs)
int f64_slot_areas(rt_handle *h, F64Slot &sl, int cap) {
    const size_t S = (size_t)h->cfg.n_streams;
    if (h->s_scan) (void)hipStreamSynchronize(h->s_scan);  // (a dropped call of the slot may still be writing them)
    (void)hipFree(sl.d_raw);
    (void)hipHostFree(sl.h_out);
    sl.d_raw = nullptr;
    sl.h_out = nullptr;
    sl.rec_cap = 0;
    if (hipMalloc(&sl.d_raw, S * (size_t)cap * sizeof(rt_record_f64)) != hipSuccess ||
        hipHostMalloc(&sl.h_out, S * (size_t)cap * sizeof(rt_record_f64)) != hipSuccess) {
        (void)hipGetLastError();
        return f64_err(h, RT_E_NOMEM, "float64 handle: no memory for " + std::to_string(cap) + " records per stream");
    }
    sl.rec_cap = cap;
    return RT_OK;
}

F64DetectArgs f64_detect_args(rt_handle *h, F64Slot &sl) {
    F64State *f = h->f64;
    F64DetectArgs a{};
    a.dp.n_seg = sl.n_seg;
    a.dp.stride = f->stride;
    a.dp.nperseg = f->N;
    a.dp.thr = f->c.threshold;
    a.dp.snr = f->c.snr_threshold;
    a.dp.cal_db = f->c.calibration_db;
    a.dp.fs = h->cfg.sample_rate;
    a.dp.min_d = h->cfg.min_duration_s;
    a.dp.max_d = h->cfg.max_duration_s;
    a.n_streams = h->cfg.n_streams;
    if (sl.is_extract) {
        a.spec = sl.ex_spec;
        a.n_bins = sl.ex_bins;
        a.prev = sl.ex_last;
        a.prev_cols = sl.ex_last_cols;
        a.dp.n_seg_last = sl.ex_last ? sl.ex_last_cols : -1;
        a.dp.tail_cols = sl.ex_last ? sl.ex_last_cols : 0;  // the whole previous spectrogram (the reference's unlimited look-back)
    } else {
        a.spec = f->d_map;
        a.n_bins = f->N;
        a.prev = f->d_tail[sl.tail_read];
        a.prev_cols = f->K;
        a.dp.n_seg_last = sl.n_seg_last;
        a.dp.tail_cols = sl.n_seg_last < 0 ? 0 : std::min(f->K, sl.n_seg_last);
        a.no_last = sl.lc.took.empty() ? nullptr : sl.d_no_last;
        if (sl.lc.masked) {  // rt_set_present: each stream's own previous segment count, and who sits the call out
            a.absent = sl.d_mask + (size_t)kMaskAbsent * h->cfg.n_streams;
            a.n_seg_last_s = sl.d_mask + (size_t)kMaskNSegLast * h->cfg.n_streams;
            a.tail_k = f->K;
        }
    }
    a.thr_s = f->d_thr_s;
    a.cal_s = f->d_cal_s;
    a.set_s = f->d_set_s;
    a.raw = sl.d_raw;
    a.raw_count = sl.d_raw_count;
    a.rec_cap = sl.rec_cap;
    a.out = sl.h_out;
    a.out_off = sl.h_meta;
    a.out_count = sl.h_meta + h->cfg.n_streams + 1;
    return a;
}

// the call's kernels on the handle's stream: the transform (not for rt_extract_f64), detection, records, then the call's event
template <int FMT>
void launch_scan_f64(const F64ScanParams &p, int nb, unsigned grid, size_t lds, hipStream_t st) {
    if (nb == 4) scan_f64<FMT, 4><<<grid, kF64ScanBlock, lds, st>>>(p);
    else if (nb == 8) scan_f64<FMT, 8><<<grid, kF64ScanBlock, lds, st>>>(p);
    else scan_f64<FMT, 16><<<grid, kF64ScanBlock, lds, st>>>(p);
}
size_t f64_scan_lds(const F64State *f) { return (size_t)16 * f->N * (f->group + 1); }
size_t f64_sort_lds(const F64State *f) { return (size_t)f->sort_cap * (sizeof(double) + sizeof(uint32_t)); }

// RT_FLAG_F64_SPARSE: the call's kernels -- the fused scan, detection from the lists, records, the counters back to zero
int f64_enqueue_sparse(rt_handle *h, F64Slot &sl) {
    F64State *f = h->f64;
    const int S = h->cfg.n_streams;
    hipStream_t st = h->s_scan;
    const int n_chunks = f64_sparse_chunks(sl.n_seg, f->chunk);
    sl.n_rescued = -1;
    if (sl.n_seg > 0) {
        F64ScanParams p{};
        p.iq = sl.iq;
        p.stream_stride = sl.stream_stride;
        p.n_streams = S;
        p.n_seg = sl.n_seg;
        p.nperseg = f->N;
        p.group = f->group;
        p.chunk = f->chunk;
        p.n_chunks = n_chunks;
        p.chunk_cap = f->chunk_cap;
        p.tail_cols = f->K;
        p.hot_cap = f->hot_cap;
        p.scale = f->c.scale;
        p.thr = f->c.threshold;
        p.thr_s = f->d_thr_s;
        p.window = f->d_window;
        p.tw = f->d_tw;
        p.tail = f->d_tail[sl.tail_write];
        p.absent = sl.lc.masked ? sl.d_mask + (size_t)kMaskAbsent * S : nullptr;
        p.partial = f->d_partial;
        p.keys = sl.d_keys;
        p.vals = sl.d_vals;
        p.count = sl.d_cell_count;
        const unsigned grid = (unsigned)((int64_t)S * n_chunks);
        const int nb = f->N * f->group / kF64ScanBlock;
        const size_t lds = f64_scan_lds(f);
        if (sl.fmt == kFmtU8) launch_scan_f64<kFmtU8>(p, nb, grid, lds, st);
        else if (sl.fmt == kFmtI16) launch_scan_f64<kFmtI16>(p, nb, grid, lds, st);
        else if (sl.fmt == kFmtI8) launch_scan_f64<kFmtI8>(p, nb, grid, lds, st);
        else launch_scan_f64<kFmtC64>(p, nb, grid, lds, st);
        RT_HIP(h, hipGetLastError());
    }
    F64SparseArgs sa{};
    sa.a = f64_detect_args(h, sl);
    sa.a.spec = nullptr;
    sa.partial = f->d_partial;
    sa.n_chunks = n_chunks;
    sa.chunk_cap = f->chunk_cap;
    sa.row_sums = f->d_row_sums;
    sa.keys = sl.d_keys;
    sa.vals = sl.d_vals;
    sa.count = sl.d_cell_count;
    sa.hot_cap = f->hot_cap;
    sa.sort_cap = f->sort_cap;
    sa.hot_out = sl.h_hot;
    if (sl.d_row_means) {
        sa.a.row_means = sl.d_row_means;
        detect_sparse_f64<true><<<(unsigned)S, 256, f64_sort_lds(f), st>>>(sa);
    } else {
        detect_sparse_f64<false><<<(unsigned)S, 256, f64_sort_lds(f), st>>>(sa);
    }
    finalize_sparse_f64<<<(unsigned)S, 256, 0, st>>>(sa.a);
    clear_counts_sparse_f64<<<(unsigned)((S + 255) / 256), 256, 0, st>>>(sl.d_raw_count, sl.d_cell_count, S);
    RT_HIP(h, hipGetLastError());
    RT_HIP(h, hipEventRecord(sl.ev_done, st));
    return RT_OK;
}

template <int FMT>
void launch_scan_map_f64(const F64MapScanParams &p, int nb, unsigned grid, size_t lds, hipStream_t st) {
    if (nb == 4) scan_map_f64<FMT, 4><<<grid, kF64ScanBlock, lds, st>>>(p);
    else if (nb == 8) scan_map_f64<FMT, 8><<<grid, kF64ScanBlock, lds, st>>>(p);
    else scan_map_f64<FMT, 16><<<grid, kF64ScanBlock, lds, st>>>(p);
}

// a rescue scratch area of at least `bytes` (kept; a smaller one is replaced once nothing on the stream uses it any more)
int f64_rescue_area(rt_handle *h, double *&area, size_t &have, size_t bytes) {
    if (have >= bytes) return RT_OK;
    RT_HIP(h, hipStreamSynchronize(h->s_scan));
    (void)hipFree(area);
    area = nullptr;
    have = 0;
    if (hipMalloc(&area, bytes) != hipSuccess) {
        (void)hipGetLastError();
        area = nullptr;
        return f64_err(h, RT_E_NOMEM, "RT_FLAG_F64_RESCUE: no device memory for the rescue scratch (" + std::to_string(bytes) + " bytes)");
    }
    have = bytes;
    return RT_OK;
}

// RT_FLAG_F64_RESCUE: the present streams of the slot's call (its first pass is over) whose lists overflowed, analysed again from
// the rescue map in rounds; then the whole call ranked and packed again.  Once per enqueue of the call: sl.n_rescued.
int f64_rescue(rt_handle *h, F64Slot &sl) {
    F64State *f = h->f64;
    if (sl.n_rescued >= 0) return RT_OK;
    const int S = h->cfg.n_streams, N = f->N, T = sl.n_seg;
    std::vector<int32_t> bad;
    for (int s = 0; s < S; ++s)
        if (sl.h_hot[s] > f->hot_cap) bad.push_back(s);  // (an absent stream reports 0 cells)
    if (bad.empty() || T <= 0) {
        sl.n_rescued = 0;
        return RT_OK;
    }
    hipStream_t st = h->s_scan;
    const int n_chunks = f64_sparse_chunks(T, f->chunk);
    const F64RescueRounds rr = f64_rescue_rounds((int)bad.size(), T, N, kF64RescueBudget);
    int rc = f64_rescue_area(h, f->d_rs_map, f->rs_map_bytes, (size_t)rr.per_round * (size_t)T * (size_t)N * sizeof(double));
    if (rc == RT_OK) rc = f64_rescue_area(h, f->d_rs_partial, f->rs_partial_bytes, (size_t)rr.per_round * (size_t)n_chunks * (size_t)N * sizeof(double));
    if (rc != RT_OK) return rc;
    if (!f->d_rs_list && hipMalloc(&f->d_rs_list, (size_t)S * sizeof(int32_t)) != hipSuccess) {
        (void)hipGetLastError();
        f->d_rs_list = nullptr;
        return f64_err(h, RT_E_NOMEM, "RT_FLAG_F64_RESCUE: no device memory for the stream list");
    }
    const size_t lds = f64_scan_lds(f);
    if (!f->rs_attr && lds > 64 * 1024) {
        const void *scans[] = {(const void *)scan_map_f64<kFmtC64, 4>, (const void *)scan_map_f64<kFmtC64, 8>, (const void *)scan_map_f64<kFmtC64, 16>,
                               (const void *)scan_map_f64<kFmtU8, 4>,  (const void *)scan_map_f64<kFmtU8, 8>,  (const void *)scan_map_f64<kFmtU8, 16>,
                               (const void *)scan_map_f64<kFmtI16, 4>, (const void *)scan_map_f64<kFmtI16, 8>, (const void *)scan_map_f64<kFmtI16, 16>,
                               (const void *)scan_map_f64<kFmtI8, 4>,  (const void *)scan_map_f64<kFmtI8, 8>,  (const void *)scan_map_f64<kFmtI8, 16>};
        for (const void *fn : scans) RT_HIP(h, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    }
    f->rs_attr = true;
    // (blocking: the list lives on this function's stack; the kernels of a round before have read it by the time it is rewritten,
    // because every rescue ends with a wait for the call's event)
    RT_HIP(h, hipMemcpy(f->d_rs_list, bad.data(), bad.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    // clear_counts_sparse_f64 has zeroed the raw counters behind the first pass, the other streams' raw records are still in
    // place: their counts back from the slot's meta block (an overflowing stream's is 0 there)
    RT_HIP(h, hipMemcpyAsync(sl.d_raw_count, sl.h_meta + S + 1, (size_t)S * sizeof(int32_t), hipMemcpyHostToDevice, st));
    F64ListArgs la{};
    la.a = f64_detect_args(h, sl);
    la.a.spec = f->d_rs_map;
    la.partial = f->d_rs_partial;
    la.n_chunks = n_chunks;
    const int nb = N * f->group / kF64ScanBlock;
    for (int r = 0; r < rr.rounds; ++r) {
        const int first = r * rr.per_round;
        const int n_list = std::min(rr.per_round, (int)bad.size() - first);
        F64MapScanParams p{};
        p.iq = sl.iq;
        p.stream_stride = sl.stream_stride;
        p.n_seg = T;
        p.nperseg = N;
        p.group = f->group;
        p.chunk = f->chunk;
        p.n_chunks = n_chunks;
        p.n_list = n_list;
        p.list = f->d_rs_list + first;
        p.scale = f->c.scale;
        p.window = f->d_window;
        p.tw = f->d_tw;
        p.map = f->d_rs_map;
        p.partial = f->d_rs_partial;
        const unsigned grid = (unsigned)((int64_t)n_list * n_chunks);
        if (sl.fmt == kFmtU8) launch_scan_map_f64<kFmtU8>(p, nb, grid, lds, st);
        else if (sl.fmt == kFmtI16) launch_scan_map_f64<kFmtI16>(p, nb, grid, lds, st);
        else if (sl.fmt == kFmtI8) launch_scan_map_f64<kFmtI8>(p, nb, grid, lds, st);
        else launch_scan_map_f64<kFmtC64>(p, nb, grid, lds, st);
        la.list = p.list;
        la.n_list = n_list;
        const int64_t rows = (int64_t)n_list * N;
        detect_list_f64<<<(unsigned)((rows + 255) / 256), 256, 0, st>>>(la);
        stats_list_f64<<<(unsigned)n_list, 256, 0, st>>>(la);
        RT_HIP(h, hipGetLastError());
    }
    finalize_sparse_f64<<<(unsigned)S, 256, 0, st>>>(la.a);
    clear_counts_sparse_f64<<<(unsigned)((S + 255) / 256), 256, 0, st>>>(sl.d_raw_count, sl.d_cell_count, S);
    RT_HIP(h, hipGetLastError());
    RT_HIP(h, hipEventRecord(sl.ev_done, st));
    RT_HIP(h, hipEventSynchronize(sl.ev_done));
    sl.n_rescued = (int)bad.size();
    return RT_OK;
}

int f64_enqueue(rt_handle *h, F64Slot &sl) {
    F64State *f = h->f64;
    if (f->sparse && !sl.is_extract) return f64_enqueue_sparse(h, sl);
    const int S = h->cfg.n_streams;
    hipStream_t st = h->s_scan;
    if (!sl.is_extract && sl.n_seg > 0) {
        F64StftParams p{};
        p.iq = sl.iq;
        p.stream_stride = sl.stream_stride;
        p.n_streams = S;
        p.n_seg = sl.n_seg;
        p.nperseg = f->N;
        p.m = f->M;
        p.log2m = f->log2m;
        p.segs_per_block = f->SPB;
        p.tail_cols = f->K;
        p.scale = f->c.scale;
        p.window = f->d_window;
        p.cwin = f->d_cwin;
        p.bfilt = f->d_bfilt;
        p.tw = f->d_tw;
        p.spec = f->d_map;
        p.tail = f->d_tail[sl.tail_write];
        p.absent = sl.lc.masked ? sl.d_mask + (size_t)kMaskAbsent * S : nullptr;
        const int64_t grid = (int64_t)S * ((sl.n_seg + f->SPB - 1) / f->SPB);
        const size_t lds = (size_t)f->SPB * f->M * sizeof(cd);
        if (sl.fmt == kFmtU8) {
            if (f->blu) stft_f64<kFmtU8, true><<<(unsigned)grid, kF64Block, lds, st>>>(p);
            else stft_f64<kFmtU8, false><<<(unsigned)grid, kF64Block, lds, st>>>(p);
        } else if (sl.fmt == kFmtI16) {
            if (f->blu) stft_f64<kFmtI16, true><<<(unsigned)grid, kF64Block, lds, st>>>(p);
            else stft_f64<kFmtI16, false><<<(unsigned)grid, kF64Block, lds, st>>>(p);
        } else if (sl.fmt == kFmtI8) {
            if (f->blu) stft_f64<kFmtI8, true><<<(unsigned)grid, kF64Block, lds, st>>>(p);
            else stft_f64<kFmtI8, false><<<(unsigned)grid, kF64Block, lds, st>>>(p);
        } else {
            if (f->blu) stft_f64<kFmtC64, true><<<(unsigned)grid, kF64Block, lds, st>>>(p);
            else stft_f64<kFmtC64, false><<<(unsigned)grid, kF64Block, lds, st>>>(p);
        }
        RT_HIP(h, hipGetLastError());
    }
    F64DetectArgs a = f64_detect_args(h, sl);
    const int64_t rows = (int64_t)S * a.n_bins;
    if (sl.d_row_means && !sl.is_extract) {  // RT_FLAG_ROW_MEANS: every row's mean as well
        a.row_means = sl.d_row_means;
        detect_f64<true><<<(unsigned)((rows + 255) / 256), 256, 0, st>>>(a);
    } else {
        detect_f64<false><<<(unsigned)((rows + 255) / 256), 256, 0, st>>>(a);
    }
    finalize_f64<<<(unsigned)S, 256, 0, st>>>(a);
    clear_counts_f64<<<(unsigned)((S + 255) / 256), 256, 0, st>>>(sl.d_raw_count, S);
    if (sl.d_cells && !sl.is_extract && sl.n_seg > 0) {
        // RT_FLAG_RECORD_CELLS: the cells finalize_f64 has just read, behind it on the call's stream (the map is the next call's after that)
        CellsArgs<double, rt_record_f64> ca{};
        ca.records = sl.h_out;
        ca.rec_off = sl.h_meta;  // [S + 1], packed
        ca.stage = sl.d_raw;
        ca.rec_cap = sl.rec_cap;
        ca.n_streams = S;
        ca.n_bins = a.n_bins;
        ca.n_seg = sl.n_seg;
        ca.spec = a.spec;
        ca.prev = a.prev;
        ca.prev_cols = a.prev_cols;
        ca.stream_cells = sl.d_stream_cells;
        ca.stream_base = sl.d_stream_base;
        ca.cells = sl.d_cells;
        ca.cell_cap = sl.cell_cap;
        ca.info = sl.h_cells_info;
        launch_record_cells(ca, st);
    }
    RT_HIP(h, hipGetLastError());
    RT_HIP(h, hipEventRecord(sl.ev_done, st));
    return RT_OK;
}

int f64_start(rt_handle *h, F64Slot &sl) {
    F64State *f = h->f64;
    if (sl.rec_cap < f->rec_cap) {  // (another call grew the capacity since this slot's areas were made)
        const int rc = f64_slot_areas(h, sl, f->rec_cap);
        if (rc != RT_OK) return rc;
    }
    if (sl.d_cells && sl.cell_cap < f->cells_want) {  // (... or the cell pool; best effort)
        if (h->s_scan) (void)hipStreamSynchronize(h->s_scan);
        (void)grow_cells(h, sl.d_cells, sl.cell_cap, f->cells_want);
    }
    const int rc = f64_enqueue(h, sl);
    if (rc != RT_OK) return rc;
    sl.seq = ++f->n_calls;
    sl.pending = true;
    return RT_OK;
}

}  // namespace

static void destroy_f64(rt_handle *h) {
    F64State *f = h->f64;
    (void)hipSetDevice(h->cfg.device);
    (void)hipDeviceSynchronize();
    iq_free(h);
    input_stats_free(h);
    for (F64Slot &sl : f->slot) {
        (void)hipFree(sl.d_raw);
        (void)hipFree(sl.d_raw_count);
        (void)hipFree(sl.d_no_last);
        (void)hipHostFree(sl.h_mask);
        (void)hipFree(sl.d_mask);
        (void)hipFree(sl.d_stage);
        (void)hipHostFree(sl.h_out);
        (void)hipHostFree(sl.h_meta);
        (void)hipFree(sl.d_row_means);
        (void)hipFree(sl.d_cells);
        (void)hipFree(sl.d_stream_cells);
        (void)hipFree(sl.d_stream_base);
        (void)hipHostFree(sl.h_cells_info);
        (void)hipFree(sl.d_keys);
        (void)hipFree(sl.d_vals);
        (void)hipFree(sl.d_cell_count);
        (void)hipHostFree(sl.h_hot);
        if (sl.ev_done) (void)hipEventDestroy(sl.ev_done);
    }
    (void)hipFree(f->d_partial);
    (void)hipFree(f->d_row_sums);
    (void)hipFree(f->d_rs_map);
    (void)hipFree(f->d_rs_partial);
    (void)hipFree(f->d_rs_list);
    (void)hipFree(f->d_window);
    (void)hipFree(f->d_cwin);
    (void)hipFree(f->d_bfilt);
    (void)hipFree(f->d_tw);
    (void)hipFree(f->d_map);
    for (double *t : f->d_tail) (void)hipFree(t);
    (void)hipFree(f->d_thr_s);
    (void)hipFree(f->d_cal_s);
    (void)hipFree(f->d_set_s);
    if (h->own_scan_stream && h->s_scan) (void)hipStreamDestroy(h->s_scan);
    delete f;
    h->f64 = nullptr;
    delete h;
}

static int process_f64(rt_handle *h, const void *iq, int64_t n_samples, int64_t stream_stride, int fmt, bool host) {
    F64State *f = h->f64;
    int T = 0;
    int rc = check_process_args(h, iq, n_samples, stream_stride, fmt, !host, &T);
    if (rc != RT_OK) return rc;
    RT_HIP(h, hipSetDevice(h->cfg.device));
    const int S = h->cfg.n_streams;
    F64Slot &sl = f64_claim(f);
    LedgerCall &lc = sl.lc;
    sl.pending = false;
    sl.is_extract = false;
    sl.fmt = fmt;
    sl.stream_stride = stream_stride;
    sl.n_seg = T;
    sl.iq = iq;
    lc.clear();
    if (host && n_samples > 0) {
        const size_t bytes = (size_t)S * (size_t)stream_stride * (size_t)iq_sample_bytes(h, fmt);
        if (sl.stage_bytes < bytes) {
            RT_HIP(h, hipStreamSynchronize(h->s_scan));  // (the slot's last call may still read its staging buffer)
            (void)hipFree(sl.d_stage);
            sl.d_stage = nullptr;
            sl.stage_bytes = 0;
            if (hipMalloc(&sl.d_stage, bytes) != hipSuccess) {
                (void)hipGetLastError();
                return f64_err(h, RT_E_NOMEM, "no device memory to stage the IQ");
            }
            sl.stage_bytes = bytes;
        }
        RT_HIP(h, hipMemcpyAsync(sl.d_stage, iq, bytes, hipMemcpyHostToDevice, h->s_scan));
        RT_HIP(h, hipStreamSynchronize(h->s_scan));  // (blocking: the caller may reuse its buffer when this returns)
        sl.iq = sl.d_stage;
    }
    const int idx = (int)(&sl - f->slot);
    const F64Slot &o = f->slot[1 - idx];
    rc = begin_ledger_call(h, idx, lc, o.pending ? &o.lc : nullptr, sl.seq ? sl.ev_done : nullptr, T, fmt, sl.iq, stream_stride);
    if (rc != RT_OK) return rc;
    sl.n_seg_last = lc.n_seg_last;
    sl.tail_read = lc.tail_read;
    sl.tail_write = lc.tail_write;
    // The call's rows to the device.  (Blocking: a float64 handle picks any free slot for a call, so no event of the slot's says when
    // a copy has left the host rows.  The float32 path waits for its slot's ev_done.)
    const auto upload = [&]() -> int {
        if (lc.masked) {
            // rt_set_present: the snapshot's rows, and the absent streams' look-back columns carried from the buffer the call reads
            // to the one it writes
            int n_sub = 0, n_lin = 0;
            fill_mask_rows(lc.pc, S, nullptr, sl.h_mask, &n_lin, &n_sub, &sl.n_absent);
            RT_HIP(h, hipMemcpyAsync(sl.d_mask, sl.h_mask, (size_t)kMaskRows * S * sizeof(int32_t), hipMemcpyHostToDevice, h->s_scan));
            RT_HIP(h, hipStreamSynchronize(h->s_scan));
            return enqueue_carry<double>(h, sl.d_mask + (size_t)kMaskAbsentList * S, sl.n_absent, f->d_tail[sl.tail_read], f->d_tail[sl.tail_write], f->K, f->N);
        }
        if (!lc.took.empty()) {  // lock-step: the streams that take a reset
            RT_HIP(h, hipMemcpyAsync(sl.d_no_last, lc.took.data(), (size_t)S * sizeof(int32_t), hipMemcpyHostToDevice, h->s_scan));
            RT_HIP(h, hipStreamSynchronize(h->s_scan));
        }
        return RT_OK;
    };
    rc = upload();
    const bool stats = h->ist && h->ist->on;
    if (rc == RT_OK && stats) rc = enqueue_input_stats(h, idx, sl.iq, n_samples, stream_stride, fmt, lc.masked ? sl.d_mask + (size_t)kMaskAbsent * S : nullptr);
    if (rc == RT_OK) rc = f64_start(h, sl);
    if (rc != RT_OK) h->ledger.rollback(lc);
    else if (stats) h->ist->slot[idx].seq = sl.seq;  // (the slot's rows are this call's)
    return rc;
}

extern "C" {

int rt_create_f64(const rt_config *cfg, const rt_config_f64 *f64, rt_handle **out) {
    if (!cfg || !f64 || !out) return fail_create(RT_E_INVALID, "null argument");
    *out = nullptr;
    if (cfg->n_streams < 1 || cfg->max_samples < 0 || !f64->window || !(cfg->sample_rate > 0))
        return fail_create(RT_E_INVALID, "float64 handle: n_streams, max_samples, rt_config_f64.window and sample_rate must be set");
    if (!(cfg->max_duration_s >= 0) || !(cfg->min_duration_s >= 0)) return fail_create(RT_E_INVALID, "durations must be non-negative");
    const int n = cfg->nperseg;
    const bool pow2 = n > 0 && (n & (n - 1)) == 0;
    if (n < 8 || (pow2 && n > kF64MaxM) || (!pow2 && n > kF64MaxN))
        return fail_create(RT_E_UNSUPPORTED, "fft_nperseg " + std::to_string(n) + " is not supported by a float64 handle: 8 ... 4096, or a power of two up to 8192");
    if (cfg->mode < RT_MODE_AUTO || cfg->mode > RT_MODE_RUNFILTER) return fail_create(RT_E_INVALID, "bad mode");
    const bool sparse = (cfg->flags & RT_FLAG_F64_SPARSE) != 0;
    if (sparse && cfg->mode != RT_MODE_AUTO)
        return fail_create(RT_E_INVALID, "RT_FLAG_F64_SPARSE on a float64 handle selects the path by itself: mode must be RT_MODE_AUTO");
    if (cfg->mode != RT_MODE_AUTO && cfg->mode != RT_MODE_DENSE)
        return fail_create(RT_E_UNSUPPORTED, "a float64 handle runs the dense path only: mode must be RT_MODE_AUTO or RT_MODE_DENSE");
    if ((cfg->flags & RT_FLAG_F64_RESCUE) && !sparse)
        return fail_create(RT_E_INVALID, "RT_FLAG_F64_RESCUE re-runs the overflowing streams of the map-free path: it needs RT_FLAG_F64_SPARSE");
    if (cfg->lanes > 1) return fail_create(RT_E_UNSUPPORTED, "a float64 handle has one launch sequence per call: lanes must be 0 or 1");
    if (sparse) {  // the map-free path (rt_f64_sparse.h): its own limits, the arithmetic in rt_core.h
        if (!f64_sparse_nperseg_ok(n))
            return fail_create(RT_E_UNSUPPORTED, "RT_FLAG_F64_SPARSE: fft_nperseg " + std::to_string(n) + " has no map-free float64 path (a power of two, 32 ... 4096)");
        if (cfg->flags & RT_FLAG_RECORD_CELLS)
            return fail_create(RT_E_UNSUPPORTED, "RT_FLAG_F64_SPARSE with RT_FLAG_RECORD_CELLS: a float64 handle without a map keeps no record cells");
        if (f64_sparse_hot_capacity(cfg->hot_capacity) < 0)
            return fail_create(RT_E_INVALID, "RT_FLAG_F64_SPARSE on a float64 handle: hot_capacity must be 0 or 1024 ... 8192 cells per stream");
        if (cfg->segs_per_chunk < 0) return fail_create(RT_E_INVALID, "RT_FLAG_F64_SPARSE on a float64 handle: segs_per_chunk must not be negative");
        if (cfg->max_samples / n > kF64KeyMaxSeg)
            return fail_create(RT_E_UNSUPPORTED, "RT_FLAG_F64_SPARSE on a float64 handle: max_samples / fft_nperseg exceeds 2^20 segments (the cell keys)");
    }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev < 1)
        return fail_create(RT_E_NO_DEVICE, std::string("no HIP device: ") + (e != hipSuccess ? hipGetErrorString(e) : "count 0"));
    if (cfg->device < 0 || cfg->device >= ndev) return fail_create(RT_E_INVALID, "device ordinal out of range");
    e = hipSetDevice(cfg->device);
    if (e != hipSuccess) return fail_create(RT_E_NO_DEVICE, std::string("hipSetDevice: ") + hipGetErrorString(e));

    rt_handle *h = new (std::nothrow) rt_handle();
    F64State *f = new (std::nothrow) F64State();
    if (!h || !f) {
        delete h;
        delete f;
        return fail_create(RT_E_NOMEM, "out of host memory");
    }
    h->f64 = f;
    h->cfg = *cfg;
    h->cfg.window = nullptr;
    h->cfg.mode = RT_MODE_DENSE;
    h->N = n;
    f->c = *f64;
    f->c.window = nullptr;
    f->N = n;
    f->blu = !pow2;
    f->M = 1;
    while (f->M < (pow2 ? n : 2 * n - 1)) f->M <<= 1;
    while ((1 << f->log2m) < f->M) ++f->log2m;
    f->SPB = std::max(1, std::min(64, 1024 / f->M));
    f->stride = probe_stride(n, cfg->sample_rate, cfg->min_duration_s);
    f->K = tail_cols(n, cfg->sample_rate, cfg->max_duration_s);
    f->max_seg = (int)(cfg->max_samples / n);
    f->rec_cap = cfg->record_capacity > 0 ? cfg->record_capacity : 1024;
    h->ledger.configure(cfg->n_streams);
    const size_t S = (size_t)cfg->n_streams;
    if (sparse) {
        f->sparse = true;
        h->cfg.mode = RT_MODE_SPARSE;
        f->group = f64_sparse_group(n);
        f->chunk = f64_sparse_chunk(n, cfg->segs_per_chunk, cfg->n_streams, f->max_seg);
        f->chunk_cap = std::max(1, f64_sparse_chunks(f->max_seg, f->chunk));
        f->hot_cap = f64_sparse_hot_capacity(cfg->hot_capacity);
        f->sort_cap = next_pow2(f->hot_cap);
        f->rescue = (cfg->flags & RT_FLAG_F64_RESCUE) != 0;
    }
#define RT_F64_CREATE(expr)                                                               \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess) {                                                           \
            const bool oom_ = e_ == hipErrorOutOfMemory;                                  \
            const std::string m_ = std::string(#expr) + ": " + hipGetErrorString(e_);     \
            (void)hipGetLastError();                                                      \
            destroy_f64(h);                                                               \
            return fail_create(oom_ ? RT_E_NOMEM : RT_E_NO_DEVICE, "float64 handle: " + m_); \
        }                                                                                 \
    } while (0)
    if (cfg->hip_stream) {
        h->s_scan = (hipStream_t)cfg->hip_stream;
    } else {
        RT_F64_CREATE(hipStreamCreateWithFlags(&h->s_scan, hipStreamNonBlocking));
        h->own_scan_stream = true;
    }
    h->s_detect = h->s_scan;
    // tables, made on the host so that every entry is rounded once to double (rt_tables.h)
    {
        const std::vector<cd> tw = transform_twiddles<cd, long double>(f->M);
        RT_DEVICE_COPY(RT_F64_CREATE, f->d_tw, tw.data(), tw.size() * sizeof(cd));
        RT_DEVICE_COPY(RT_F64_CREATE, f->d_window, f64->window, (size_t)n * sizeof(double));
        if (f->blu) {
            const BluesteinTables<cd> bt = bluestein_tables<cd, long double>(f64->window, n, f->M, f->log2m, 1.0L);
            RT_DEVICE_COPY(RT_F64_CREATE, f->d_cwin, bt.cwin.data(), (size_t)n * sizeof(cd));
            RT_DEVICE_COPY(RT_F64_CREATE, f->d_bfilt, bt.bfilt.data(), (size_t)f->M * sizeof(cd));
        }
    }
    const int lds = f->SPB * f->M * (int)sizeof(cd);
    if (lds > 64 * 1024) {
        const void *fns[] = {(const void *)stft_f64<kFmtC64, false>, (const void *)stft_f64<kFmtC64, true>, (const void *)stft_f64<kFmtU8, false>,
                             (const void *)stft_f64<kFmtU8, true>, (const void *)stft_f64<kFmtI16, false>, (const void *)stft_f64<kFmtI16, true>,
                             (const void *)stft_f64<kFmtI8, false>, (const void *)stft_f64<kFmtI8, true>};
        for (const void *fn : fns) RT_F64_CREATE(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    }
    // the float64 map (S T N 8 bytes) and the look-back tails; RT_FLAG_F64_SPARSE: no map (rt_extract_f64 and rt_spectrogram_f64
    // work on the caller's memory), the per-chunk row sums instead
    if (f->sparse) {
        const void *scans[] = {(const void *)scan_f64<kFmtC64, 4>, (const void *)scan_f64<kFmtC64, 8>, (const void *)scan_f64<kFmtC64, 16>,
                               (const void *)scan_f64<kFmtU8, 4>,  (const void *)scan_f64<kFmtU8, 8>,  (const void *)scan_f64<kFmtU8, 16>,
                               (const void *)scan_f64<kFmtI16, 4>, (const void *)scan_f64<kFmtI16, 8>, (const void *)scan_f64<kFmtI16, 16>,
                               (const void *)scan_f64<kFmtI8, 4>,  (const void *)scan_f64<kFmtI8, 8>,  (const void *)scan_f64<kFmtI8, 16>};
        if (f64_scan_lds(f) > 64 * 1024)
            for (const void *fn : scans) RT_F64_CREATE(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)f64_scan_lds(f)));
        if (f64_sort_lds(f) > 64 * 1024) {
            RT_F64_CREATE(hipFuncSetAttribute((const void *)detect_sparse_f64<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)f64_sort_lds(f)));
            RT_F64_CREATE(hipFuncSetAttribute((const void *)detect_sparse_f64<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)f64_sort_lds(f)));
        }
        RT_F64_CREATE(hipMalloc(&f->d_partial, S * (size_t)f->chunk_cap * (size_t)n * sizeof(double)));
        RT_F64_CREATE(hipMalloc(&f->d_row_sums, S * (size_t)n * sizeof(double)));
    } else {
        RT_F64_CREATE(hipMalloc(&f->d_map, std::max<size_t>(8, S * (size_t)f->max_seg * (size_t)n * sizeof(double))));
    }
    for (double *&t : f->d_tail) {
        RT_DEVICE_ZEROS(RT_F64_CREATE, t, S * (size_t)f->K * (size_t)n * sizeof(double));
    }
    for (F64Slot &sl : f->slot) {
        RT_DEVICE_ZEROS(RT_F64_CREATE, sl.d_raw_count, S * sizeof(int32_t));
        RT_F64_CREATE(hipMalloc(&sl.d_no_last, S * sizeof(int32_t)));
        RT_F64_CREATE(hipHostMalloc(&sl.h_meta, (2 * S + 1) * sizeof(int32_t)));
        if (cfg->flags & RT_FLAG_ROW_MEANS) RT_F64_CREATE(hipMalloc(&sl.d_row_means, S * (size_t)n * sizeof(double)));
        if (cfg->flags & RT_FLAG_RECORD_CELLS) {
            sl.cell_cap = std::max<int64_t>(64, std::min<int64_t>(kInitialPoolCells, 16 * (int64_t)S * f->rec_cap));
            RT_F64_CREATE(hipMalloc(&sl.d_cells, (size_t)sl.cell_cap * sizeof(double)));
            RT_F64_CREATE(hipMalloc(&sl.d_stream_cells, S * sizeof(long long)));
            RT_F64_CREATE(hipMalloc(&sl.d_stream_base, S * sizeof(long long)));
            RT_F64_CREATE(hipHostMalloc(&sl.h_cells_info, 2 * sizeof(unsigned long long)));
            sl.h_cells_info[0] = sl.h_cells_info[1] = 0ull;
        }
        if (f->sparse) {
            RT_F64_CREATE(hipMalloc(&sl.d_keys, S * (size_t)f->hot_cap * sizeof(uint32_t)));
            RT_F64_CREATE(hipMalloc(&sl.d_vals, S * (size_t)f->hot_cap * sizeof(double)));
            RT_DEVICE_ZEROS(RT_F64_CREATE, sl.d_cell_count, S * sizeof(int32_t));
            RT_F64_CREATE(hipHostMalloc(&sl.h_hot, S * sizeof(int32_t)));
        }
        RT_F64_CREATE(hipEventCreateWithFlags(&sl.ev_done, hipEventDisableTiming));
        if (f64_slot_areas(h, sl, f->rec_cap) != RT_OK) {
            destroy_f64(h);
            return fail_create(RT_E_NOMEM, "float64 handle: no memory for the record areas");
        }
    }
#undef RT_F64_CREATE
    *out = h;
    return RT_OK;
}

int rt_set_stream_params_f64(rt_handle *h, const double *threshold, const double *calibration_db) {
    if (!h) return RT_E_INVALID;
    if (!h->f64) {
        h->err = "rt_set_stream_params_f64 on a float32 handle: use rt_set_stream_params";
        return RT_E_INVALID;
    }
    F64State *f = h->f64;
    if (f64_oldest(f)) return f64_err(h, RT_E_INVALID, "rt_set_stream_params_f64 with unfetched calls pending: fetch them first");
    return set_stream_params_one<double>(h, f->c.threshold, f->h_thr_s, nullptr, f->d_thr_s, f->d_cal_s, threshold, calibration_db);
}

int rt_set_stream_settings_f64(rt_handle *h, const double *snr_threshold, const double *min_duration_s, const double *max_duration_s) {
    if (!h) return RT_E_INVALID;
    if (!h->f64) {
        h->err = "rt_set_stream_settings_f64 on a float32 handle: use rt_set_stream_settings";
        return RT_E_INVALID;
    }
    F64State *f = h->f64;
    const int rc = check_stream_settings<double>(h, "rt_set_stream_settings_f64", snr_threshold, min_duration_s, max_duration_s);
    if (rc != RT_OK) return rc;
    if (f64_oldest(f)) return f64_err(h, RT_E_INVALID, "rt_set_stream_settings_f64 with unfetched calls pending: fetch them first");
    return set_stream_settings_one<double>(h, f->c.snr_threshold, f->h_set_s, f->d_set_s, snr_threshold, min_duration_s, max_duration_s);
}

int rt_extract_f64(rt_handle *h, const double *spec_dev, int32_t n_seg, int32_t n_bins, const double *last_dev, int32_t n_seg_last) {
    if (!h) return RT_E_INVALID;
    forget_row_means(h);
    if (!h->f64) {
        h->err = "rt_extract_f64 on a float32 handle: use rt_extract";
        return RT_E_INVALID;
    }
    F64State *f = h->f64;
    if (n_seg < 0 || n_bins < 1 || (n_seg > 0 && !spec_dev) || (last_dev && n_seg_last < 0))
        return f64_err(h, RT_E_INVALID, "bad spectrogram arguments");
    if (n_seg == 1) return f64_err(h, RT_E_ONE_SEGMENT, "exactly one segment: the reference raises IndexError (times[1])");
    if (reinterpret_cast<uintptr_t>(spec_dev) % 8u != 0 || reinterpret_cast<uintptr_t>(last_dev) % 8u != 0)
        return f64_err(h, RT_E_INVALID, "spectrogram pointers must be 8-byte aligned (float64)");
    if ((int64_t)n_seg * n_bins > 0x7FFFFFFFll || (int64_t)h->cfg.n_streams * n_bins > 0x7FFFFFFFll)
        return f64_err(h, RT_E_UNSUPPORTED, "spectrogram too large");
    RT_HIP(h, hipSetDevice(h->cfg.device));
    F64Slot &sl = f64_claim(f);
    sl.pending = false;
    sl.is_extract = true;
    sl.lc.clear();  // (rt_extract_f64 takes nothing from the ledger and ignores the presence mask)
    sl.n_seg = n_seg;
    sl.ex_spec = spec_dev;
    sl.ex_bins = n_bins;
    sl.ex_last = last_dev;
    sl.ex_last_cols = last_dev ? n_seg_last : 0;
    return f64_start(h, sl);
}

int rt_fetch_f64(rt_handle *h, rt_record_f64 *out, size_t cap, size_t *n_out) {
    if (!h || !n_out) return RT_E_INVALID;
    if (!h->f64) {
        h->err = "rt_fetch_f64 on a float32 handle: use rt_fetch";
        return RT_E_INVALID;
    }
    F64State *f = h->f64;
    *n_out = 0;
    F64Slot *slp = f64_oldest(f);
    if (!slp) return f64_err(h, RT_E_INVALID, "rt_fetch_f64 without a preceding successful rt_process/rt_extract_f64");
    F64Slot &sl = *slp;
    const int S = h->cfg.n_streams;
    RT_HIP(h, hipSetDevice(h->cfg.device));
    RT_HIP(h, hipEventSynchronize(sl.ev_done));
    const bool sparse_call = f->sparse && !sl.is_extract;
    const bool rescue_call = sparse_call && f->rescue;
    // RT_FLAG_F64_RESCUE: the overflowing streams analysed again on their own.  A failure (RT_E_NOMEM: no scratch) consumes the
    // call like an overflow without the flag; the look-back tail the call wrote stays the next call's.
    const auto rescue = [&]() -> int {
        const int rc = f64_rescue(h, sl);
        if (rc != RT_OK) {
            sl.pending = false;
            f->rm_slot = kRowMeansNone;
        }
        return rc;
    };
    if (rescue_call) {
        const int rc = rescue();
        if (rc != RT_OK) return rc;
    } else if (sparse_call) {
        // RT_FLAG_F64_SPARSE: a stream emitted more cells than its list holds -- no result, the call is consumed (as
        // RT_MODE_SPARSE on a float32 handle); the look-back tail the call wrote stays the next call's
        for (int s = 0; s < S; ++s)
            if (sl.h_hot[s] > f->hot_cap) {
                sl.pending = false;
                f->rm_slot = kRowMeansNone;
                return f64_err(h, RT_E_HOT_OVERFLOW, "candidate-cell capacity exceeded (hot_capacity) on a float64 handle: stream " + std::to_string(s) +
                                                         " emitted " + std::to_string(sl.h_hot[s]) + " cells");
            }
    }
    bool truncated = false;
    for (;;) {
        int wanted = 0;
        for (int s = 0; s < S; ++s) wanted = std::max(wanted, sl.h_meta[S + 1 + s]);
        if (wanted <= sl.rec_cap) {
            // RT_FLAG_RECORD_CELLS: more cells than the slot's pool holds -- a larger pool, and the call analysed again (the map may be the next call's by now)
            if (sl.d_cells && !sl.is_extract && sl.n_seg > 0 && sl.h_cells_info[0] > (unsigned long long)sl.cell_cap &&
                grow_cells(h, sl.d_cells, sl.cell_cap, (int64_t)sl.h_cells_info[0]) == RT_OK) {
                f->cells_want = std::max(f->cells_want, sl.cell_cap);
                const int rc = f64_enqueue(h, sl);
                if (rc != RT_OK) {
                    sl.pending = false;
                    return rc;
                }
                RT_HIP(h, hipEventSynchronize(sl.ev_done));
                continue;
            }
            break;
        }
        if (sl.is_extract) {  // (the library does not keep the caller's spectrogram: the first records of each stream that fit)
            truncated = true;
            break;
        }
        // a stream found more records than the slot holds: grow the capacity and analyse the call again (its IQ is still valid)
        int cap2 = sl.rec_cap;
        while (cap2 < wanted) cap2 *= 2;
        int rc = f64_slot_areas(h, sl, cap2);
        if (rc != RT_OK) {
            sl.pending = false;
            return rc;
        }
        f->rec_cap = std::max(f->rec_cap, cap2);
        rc = f64_enqueue(h, sl);
        if (rc != RT_OK) {
            sl.pending = false;
            return rc;
        }
        RT_HIP(h, hipEventSynchronize(sl.ev_done));
        if (rescue_call) {  // (the whole call ran again: so do its overflowing streams)
            rc = rescue();
            if (rc != RT_OK) return rc;
        }
    }
    const size_t total = (size_t)sl.h_meta[S];
    *n_out = total;
    h->info = rt_call_info{};
    h->info.n_seg = sl.n_seg;
    h->info.mode_used = sparse_call ? RT_MODE_SPARSE : RT_MODE_DENSE;
    h->info.n_records = (int64_t)total;
    if (rescue_call) {
        h->info.n_dense_streams = sl.n_rescued;
        h->info.fell_back = sl.n_rescued > 0 ? 1 : 0;
    }
    // (the counters: cells emitted, not cells stored -- of every map-free call, with RT_FLAG_F64_RESCUE or without)
    for (int s = 0; sparse_call && s < S; ++s) h->info.n_hot += sl.h_hot[s];
    if (total && (!out || !cap)) return truncated ? RT_E_CAPACITY : RT_OK;  // size query: the call stays pending
    const size_t n = std::min(total, cap);
    if (n) std::memcpy(out, sl.h_out, n * sizeof(rt_record_f64));
    sl.pending = false;
    f->rm_slot = sl.is_extract ? kRowMeansExtract : (int)(&sl - f->slot);
    f->cells_full = !truncated && n == total;
    if (h->riq) {  // rt_fetch_record_iq, as in fetch_one
        RecordIq &q = *h->riq;
        if (sl.is_extract) q.delivered = kIqExtract;
        else if (!sl.lc.iq_on) q.delivered = kIqOff;
        else if (!f->cells_full) q.delivered = kIqTruncated;
        else iq_gather(h, (int)(&sl - f->slot), sl.lc.iq, sl.h_out, sizeof(rt_record_f64), total, sl.iq, sl.stream_stride);
    }
    if (truncated) return f64_err(h, RT_E_CAPACITY, "rt_extract_f64: a stream found more records than record_capacity");
    if (n < total) return f64_err(h, RT_E_CAPACITY, "output buffer too small: records lost");
    return RT_OK;
}

int rt_fetch_row_means_f64(rt_handle *h, double *out, size_t n) {
    if (!h) return RT_E_INVALID;
    if (!h->f64) {
        h->err = "rt_fetch_row_means_f64 on a float32 handle: use rt_fetch_row_means";
        return RT_E_INVALID;
    }
    const int rc = row_means_refused(h, out, n, h->f64->rm_slot);
    if (rc != RT_OK) return rc;
    // (T == 0: detect_f64<true> divided an empty sum by zero -- NaN, as np.mean of an empty row; the copy as in rt_fetch_row_means)
    RT_HIP(h, hipSetDevice(h->cfg.device));
    RT_HIP(h, hipMemcpy(out, h->f64->slot[h->f64->rm_slot].d_row_means, n * sizeof(double), hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_fetch_record_cells_f64(rt_handle *h, int64_t *offsets, size_t n_offsets, double *cells, size_t cap, size_t *n_cells) {
    if (!h || !n_cells) return RT_E_INVALID;
    *n_cells = 0;
    if (!h->f64) {
        h->err = "rt_fetch_record_cells_f64 on a float32 handle: use rt_fetch_record_cells";
        return RT_E_INVALID;
    }
    F64State *f = h->f64;
    int rc = record_cells_refused(h, f->rm_slot, f->cells_full);
    if (rc != RT_OK) return rc;
    const F64Slot &sl = f->slot[f->rm_slot];
    const size_t records = (size_t)sl.h_meta[h->cfg.n_streams];  // (delivered in full: all of the packed output)
    size_t total = 0;
    for (size_t i = 0; i < records; ++i) total += (size_t)(sl.h_out[i].end - sl.h_out[i].start);
    rc = record_cells_state(h, sl.h_cells_info, sl.cell_cap, total);
    if (rc != RT_OK) return rc;
    if (offsets && n_offsets != records + 1) {
        h->err = "rt_fetch_record_cells: n_offsets must be the number of records the last rt_fetch_f64 delivered, plus one";
        return RT_E_INVALID;
    }
    *n_cells = total;
    const bool query = !cells || cap == 0;
    if (!query && cap < total) {
        h->err = "rt_fetch_record_cells: output buffer too small";
        return RT_E_CAPACITY;
    }
    if (offsets) {
        offsets[0] = 0;
        for (size_t i = 0; i < records; ++i) offsets[i + 1] = offsets[i] + (sl.h_out[i].end - sl.h_out[i].start);
    }
    if (!query && total) {
        RT_HIP(h, hipSetDevice(h->cfg.device));
        RT_HIP(h, hipMemcpy(cells, sl.d_cells, total * sizeof(double), hipMemcpyDeviceToHost));
    }
    return RT_OK;
}

int rt_spectrogram_f64(rt_handle *h, const void *iq_dev, int64_t n_samples, int64_t stream_stride, double *spec_dev) {
    if (!h || !iq_dev || !spec_dev) return RT_E_INVALID;
    if (!h->f64) {
        h->err = "rt_spectrogram_f64 on a float32 handle: use rt_spectrogram";
        return RT_E_INVALID;
    }
    F64State *f = h->f64;
    if (n_samples < 0 || n_samples > h->cfg.max_samples || stream_stride < n_samples || reinterpret_cast<uintptr_t>(iq_dev) % 16u != 0 ||
        reinterpret_cast<uintptr_t>(spec_dev) % 8u != 0)
        return f64_err(h, RT_E_INVALID, "n_samples/stream_stride out of range for this handle, or misaligned pointer");
    RT_HIP(h, hipSetDevice(h->cfg.device));
    const int T = (int)(n_samples / f->N);
    if (T == 0) return RT_OK;
    RT_HIP(h, hipDeviceSynchronize());
    F64StftParams p{};
    p.iq = iq_dev;
    p.stream_stride = stream_stride;
    p.n_streams = h->cfg.n_streams;
    p.n_seg = T;
    p.nperseg = f->N;
    p.m = f->M;
    p.log2m = f->log2m;
    p.segs_per_block = f->SPB;
    p.tail_cols = f->K;
    p.scale = f->c.scale;
    p.window = f->d_window;
    p.cwin = f->d_cwin;
    p.bfilt = f->d_bfilt;
    p.tw = f->d_tw;
    p.spec = spec_dev;
    p.tail = nullptr;
    const int64_t grid = (int64_t)h->cfg.n_streams * ((T + f->SPB - 1) / f->SPB);
    const size_t lds = (size_t)f->SPB * f->M * sizeof(cd);
    if (f->blu) stft_f64<kFmtC64, true><<<(unsigned)grid, kF64Block, lds, h->s_scan>>>(p);
    else stft_f64<kFmtC64, false><<<(unsigned)grid, kF64Block, lds, h->s_scan>>>(p);
    RT_HIP(h, hipGetLastError());
    RT_HIP(h, hipStreamSynchronize(h->s_scan));
    return RT_OK;
}

}  // extern "C"
