/*
 * rt_analyze.h -- C-ABI of the MI355X-native signal-analysis path.
 *
 * This library replaces ONE path of Nature40/pyradiotracking: the per-buffer
 * callback SignalAnalyzer.process_samples (reference
 * radiotracking/analyze.py:192-268) -- STFT power (analyze.py:234-241, i.e.
 * scipy.signal.spectrogram), plateau extraction with look-back into the
 * previous buffer (analyze.py:330-452) and the shadow filter
 * (analyze.py:282-328) -- batched over many independent streams resident in
 * HBM.  The reference is pure Python and has no FFI of its own; these entry
 * points are what a ctypes binding inside the reference's SignalAnalyzer
 * would call (see INTEGRATION.md for that binding).
 *
 * Conventions
 *   - plain C types only; every function returns an rt_status (0 = ok, <0 =
 *     error) except where noted; no exception crosses the boundary.
 *   - one handle = one GPU + one HIP stream + the per-stream carried state
 *     (the look-back tail that replaces `_spectrogram_last`, analyze.py:268).
 *     A handle is not thread-safe.
 *   - IQ is complex64 (interleaved float32 I,Q), stream-major:
 *     sample b of stream s at iq[s * stream_stride + b].
 *   - results are integer cell coordinates plus float32 linear powers; the
 *     float64 / datetime part of a Signal (frequency, ts, duration, dB) is
 *     derived on the host from them (pyradiotracking_amd/analyze.py), so it is
 *     bit-exact by construction.
 */
#ifndef RT_ANALYZE_H
#define RT_ANALYZE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 6 (round 6): fft_nperseg 32 / 64 / 128 / 8192 / 16384 run fused scans (every mode they have); record_capacity is where a stream's
 * room starts, not a limit (rt_fetch); rt_format.h: rt_signal_rows_from_records, rt_host_set_threads; rt_match.h:
 * rt_match_add_many, rt_match_pending_count_many.  Nothing of version 5 was removed or changed in layout. */
#define RT_ABI_VERSION 6

typedef enum rt_status {
    RT_OK = 0,
    RT_E_INVALID = -1,      /* bad argument / configuration                     */
    RT_E_UNSUPPORTED = -2,  /* e.g. nperseg < 8, > 8192 and not a power of two  */
    RT_E_NO_DEVICE = -3,    /* no usable GPU / HIP failure at create            */
    RT_E_HIP = -4,          /* HIP runtime error (see rt_last_error)            */
    RT_E_CAPACITY = -5,     /* record capacity exceeded (results truncated, never dropped: rt_fetch) */
    RT_E_ONE_SEGMENT = -6,  /* exactly one segment: the reference raises
                               IndexError there (analyze.py:354, times[1])      */
    RT_E_NOMEM = -7,
    RT_E_HOT_OVERFLOW = -8  /* RT_MODE_SPARSE, and a float64 handle made with RT_FLAG_F64_SPARSE, only: a candidate
                               list overflowed (hot_capacity); the call produced NO result and has been dropped --
                               unlike RT_E_CAPACITY, which hands out a truncated result                            */
} rt_status;

/* how the batch is analysed */
typedef enum rt_mode {
    RT_MODE_AUTO = 0,   /* fused sparse path; a buffer whose candidate lists overflow is re-run one
                           level up (RT_MODE_PREFILTER, RT_MODE_RUNFILTER where available, then dense) and the handle stays
                           on that level for the next 16 buffers (32, 64 ... 1024 while the probes of
                           the level below keep overflowing) */
    RT_MODE_DENSE = 1,  /* materialise the power spectrogram (any input)        */
    RT_MODE_SPARSE = 2, /* fused sparse path only; overflow -> RT_E_HOT_OVERFLOW */
    RT_MODE_PREFILTER = 3, /* sparse path behind the run-length pre-filter (two scan passes: per chunk of
                             segments and bin "every cell passes the absolute threshold", then candidate
                             cells only from such chunks and their neighbours): for inputs whose noise
                             crosses the threshold.  Needs signal_min_duration >= 2 * segs_per_chunk hops
                             (else RT_E_UNSUPPORTED); overflow -> RT_E_HOT_OVERFLOW.  RT_MODE_AUTO goes
                             through it between the sparse and the dense path where it is available. */
    RT_MODE_RUNFILTER = 4 /* ABI v5: sparse path behind the EXACT run-length pre-filter: a first scan keeps the
                             threshold bit of every cell, a planning kernel keeps the cells of threshold runs of
                             at least the minimum plateau length (or through t = 0), a second scan transforms only
                             the segments that hold such cells.  The bits also ask for snr_threshold x the bin's
                             quiet level (from the buffer before, verified against this buffer's row means), so the
                             level stays selective with the noise floor over the absolute threshold.  Any
                             segs_per_chunk.  RT_MODE_AUTO uses it between the sparse (or RT_MODE_PREFILTER, where
                             that exists) and the dense path -- at the reference's defaults (300 kS/s, 8 ms) it is
                             the only level in between.  RT_E_UNSUPPORTED where the minimum plateau length does not
                             fit the planning tiles; overflow -> RT_E_HOT_OVERFLOW. */
} rt_mode;

/*
 * Analyzer configuration.  Mirrors the derived parameters of
 * SignalAnalyzer.__init__ (analyze.py:101-117) plus batch geometry.
 */
typedef struct rt_config {
    int32_t device;             /* HIP device ordinal                                    */
    int32_t n_streams;          /* S: independent streams analysed per call              */
    int32_t nperseg;            /* fft_nperseg (analyze.py:111; the reference passes any integer on to SciPy, __main__.py:59):
                                   any size from 8 to 8192, or a power of two up to 16384.  The powers of two 32 ... 16384 run the
                                   fused scan kernels (every rt_mode up to 4096; 8192 and 16384: RT_MODE_AUTO, RT_MODE_SPARSE and
                                   RT_MODE_DENSE); every other size runs a general transform on the dense path (8 and 16: radix-2
                                   in LDS; the rest: Bluestein's algorithm on it) -- RT_MODE_AUTO or RT_MODE_DENSE only, 16 bytes of
                                   traffic per sample; anything else: RT_E_UNSUPPORTED */
    int32_t mode;               /* rt_mode                                               */
    int64_t max_samples;        /* largest per-stream buffer length B accepted           */
    double sample_rate;         /* fs (analyze.py:101)                                   */
    const float *window;        /* host pointer, nperseg float32 coefficients: the
                                   window cast to the IQ dtype as SciPy does
                                   (scipy/signal/_spectral_py.py:2083-2084)              */
    float scale;                /* 1/(fs*sum(w*w)) in float32 (_spectral_py.py:2087)     */
    float threshold;            /* signal_threshold, linear (analyze.py:115)             */
    float snr_threshold;        /* snr_threshold, linear (analyze.py:116)                */
    float calibration_db;       /* only used to order maxima in the shadow filter        */
    double min_duration_s;      /* signal_min_duration (analyze.py:113)                  */
    double max_duration_s;      /* signal_max_duration (analyze.py:114)                  */
    int32_t hot_capacity;       /* sparse path: candidate cells kept per (stream, bin mod 16 bucket) and call
                                   (0 = default: one full bin row times max(1, nperseg / 1024), 1024..8192)      */
    int32_t record_capacity;    /* records per stream and call the handle has room for AT FIRST (0 = default 1024): a stream
                                   that finds more grows the capacity -- the call is analysed again inside rt_fetch --, as
                                   the reference appends without limit (analyze.py:449-450).  Only rt_extract truncates. */
    int32_t segs_per_chunk;     /* segments per lane-group chunk (0 = default)           */
    int32_t flags;              /* RT_FLAG_*                                             */
    void *hip_stream;           /* hipStream_t to launch on, or NULL for an own stream   */
    int32_t lanes;              /* 0 / 1 = one launch sequence per call.  n > 1: the streams are split into n
                                   contiguous groups, each analysed on its own HIP stream (hip_stream must be
                                   NULL), so that the detection kernels and launch gaps of one group overlap the
                                   scan of another; same records, rt_fetch still returns them in stream order     */
    int32_t record_pool;        /* records the pinned result pool of a call holds at first (0 = default:
                                   min(n_streams * record_capacity, 4 Mi)).  A call that needs more grows the pool
                                   and is analysed again when it is fetched, so nothing is lost up to
                                   record_capacity records per stream (the reference appends without limit,
                                   analyze.py:449-450)                                                            */
} rt_config;

#define RT_FLAG_TIMING 1u /* record HIP events around the kernels of each call */
#define RT_FLAG_NO_LIN_DETREND 2u /* always subtract the segment mean before windowing (scipy's order of operations);
                                     default: for hamming / hann / boxcar windows and complex64 input the constant
                                     detrend is applied to the transform instead (three bins), which is cheaper and
                                     equal within float32 round-off, except that a segment whose samples are all one finite
                                     value (a front end that clips for a segment) is recognised and gives the column of exact
                                     zeros that x - mean gives in the reference, in every input format -- other windows and
                                     uint8 input (where a saturated segment cancels exactly in the reference) use the
                                     subtract-first form anyway */
#define RT_FLAG_GROUP_DETECT 4u    /* sparse detection (analyze.py:330-452 on the candidate lists) with one wave per stream, or per quarter
                                     of a stream's sixteen lists, instead of one per list -- the same records; the default from 1 024
                                     streams per handle on, while the streams of the call fetched last held few candidate cells (<= 448 on
                                     average).  This flag: at any number of streams, whatever they hold.  Only where the fused kernels have
                                     the form (nperseg <= 256); ignored elsewhere */
#define RT_FLAG_NO_GROUP_DETECT 8u /* ... never */
#define RT_FLAG_ROW_MEANS 16u      /* keep each call's row means for rt_fetch_row_means[_f64] (rt_create and rt_create_f64) */
#define RT_FLAG_RECORD_CELLS 32u   /* keep the cells of every record of a call for rt_fetch_record_cells[_f64] (rt_create and rt_create_f64) */
#define RT_FLAG_F64_SPARSE 64u     /* rt_create_f64 only (rt_create: RT_E_INVALID): the map-free float64 path, see "float64 handles" below */
#define RT_FLAG_F64_RESCUE 128u    /* rt_create_f64 with RT_FLAG_F64_SPARSE only (else RT_E_INVALID): streams whose candidate lists overflow are
                                    * analysed again on their own inside rt_fetch_f64, see "float64 handles" below */

/*
 * One extracted plateau, before it becomes a Signal (analyze.py:442-449).
 * `start` may be negative: it then indexes the previous buffer from its end,
 * exactly like the reference's negative `start` (analyze.py:383-388, 422-423).
 */
typedef struct rt_record {
    int32_t stream;   /* stream index within the batch                                   */
    int32_t fi;       /* frequency bin, fftfreq order (analyze.py:357)                   */
    int32_t start;    /* first cell of `data` (analyze.py:437-440)                       */
    int32_t end;      /* one past the last cell                                          */
    float max_p;      /* max(data), linear                                               */
    float mean_p;     /* mean(data), linear                                              */
    float std_db;     /* std(10*log10(data)), population                                 */
    float row_mean;   /* mean of the bin's row over the whole buffer (`freq_avg`, :375)  */
    int32_t shadowed; /* 1 if filter_shadow_signals drops it (analyze.py:315-328)        */
    int32_t reserved;
} rt_record;

typedef struct rt_handle rt_handle;

int rt_abi_version(void);

/* Create an analyzer for `cfg` on cfg->device.  Allocates all device scratch. */
int rt_create(const rt_config *cfg, rt_handle **out);

void rt_destroy(rt_handle *h);

/* Forget the carried look-back state (== `_spectrogram_last = None`, analyze.py:128). */
int rt_reset(rt_handle *h);

/*
 * Forget the look-back state of ONE stream: what the reference's Runner does when it replaces a dead or
 * timed-out SDR's analyzer by a new one (__main__.py:153-190 -> a fresh SignalAnalyzer, analyze.py:128).
 * Takes effect with the next rt_process; the other streams keep their state.  [SURVEY 8(f) rank 4]
 */
int rt_reset_stream(rt_handle *h, int32_t stream);

/*
 * Per-stream thresholds: the reference runs one SignalAnalyzer per SDR, each with its own
 * `calibration_db` (__main__.py:140-141: zip(device, calibration)), and the absolute threshold depends
 * on it (analyze.py:115: from_dB(signal_threshold_dbw + calibration_db)).  `threshold` and
 * `calibration_db` are HOST arrays of n_streams float32 (linear threshold; calibration in dB, used as in
 * rt_config to order maxima in the shadow filter); either may be NULL = keep rt_config's value for every
 * stream.  Applies to calls enqueued afterwards; refused (RT_E_INVALID) while unfetched calls are pending, since
 * AUTO mode may still re-run those with the thresholds they were enqueued with.  A stream whose threshold CHANGES
 * starts its next buffer without look-back, as after rt_reset_stream: in the reference a threshold is fixed
 * when the SignalAnalyzer is built (analyze.py:115), so a new one means a new analyzer.  [SURVEY 8(f) rank 4]
 */
int rt_set_stream_params(rt_handle *h, const float *threshold, const float *calibration_db);

/*
 * Analyse one buffer per stream: the body of process_samples (analyze.py:234-251,
 * 268).  `iq_dev` is a DEVICE pointer to S*stream_stride complex64; n_samples =
 * len(buffer) (<= max_samples); stream_stride in samples (>= n_samples).
 * Asynchronous: enqueues on the handle's streams.  Results via rt_fetch.
 * Up to two calls may be in flight (enqueue call k+1 before fetching call k, so the
 * GPU never waits for the host; with cfg.lanes > 1 the lanes' kernels also overlap
 * each other); a third rt_process without
 * an rt_fetch drops the oldest unfetched result.  `iq_dev` must stay valid and
 * unchanged until the call has been fetched.  `iq_dev` must be 8-byte aligned (whole complex64
 * samples; rt_process_u8 and rt_process_i8: 2-byte aligned; rt_process_i16: 4-byte aligned) -- anything else is
 * refused with RT_E_INVALID, not launched.
 */
int rt_process(rt_handle *h, const void *iq_dev, int64_t n_samples, int64_t stream_stride);

/*
 * Same for the RTL-SDR wire format: `iq_u8_dev` is a DEVICE pointer to S*stream_stride samples
 * of interleaved uint8 (I, Q) -- 2 bytes per sample, what librtlsdr delivers before pyrtlsdr's
 * packed_bytes_to_iq (the producer of the buffer handed to process_samples, analyze.py:157).
 * The conversion (byte/127.5 - 1) is fused into the scan kernel's load (one float32 fma per
 * component, <= 1 float32 ulp from pyrtlsdr's float64 expression); everything after it is the
 * complex64 path.  n_samples / stream_stride count samples, not bytes.  [SURVEY 8(f) rank 1]
 */
int rt_process_u8(rt_handle *h, const void *iq_u8_dev, int64_t n_samples, int64_t stream_stride);

/*
 * Same for 16-bit signed IQ (SoapySDR CS16, UHD sc16, SigMF ci16_le): `iq_i16_dev` is a DEVICE pointer to
 * S*stream_stride samples of interleaved little-endian int16 (I, Q) -- 4 bytes per sample, 4-byte aligned.  A
 * component's value is (float)i * 2^-15 ((double)i * 2^-15 on a float64 handle): range [-1, 1 - 2^-15], -32768 is
 * legal and maps to -1.  Both the conversion and the multiplication are exact and happen in the scan kernel's load;
 * everything after it is the complex64 path, detrend by linearity and RT_FLAG_NO_LIN_DETREND included (unlike
 * rt_process_u8, which always subtracts the mean first).  So the call delivers, byte for byte, the records, row means
 * and record cells of rt_process on the complex64 (float64 handle: complex128) array q * 2^-15 -- with 4 bytes of
 * memory traffic a sample instead of 8 (16).  No other scale is offered: a radio whose full scale sits elsewhere
 * (12 bits in 16) differs by a constant, which calibration_db takes.  n_samples / stream_stride count samples.
 */
int rt_process_i16(rt_handle *h, const void *iq_i16_dev, int64_t n_samples, int64_t stream_stride);

/*
 * Same for 8-bit signed IQ (HackRF's native format, SoapySDR CS8, UHD sc8, SigMF ci8): `iq_i8_dev` is a DEVICE pointer
 * to S*stream_stride samples of interleaved two's-complement int8 (I, Q) -- 2 bytes per sample, 2-byte aligned (whole
 * I,Q pairs; anything else is refused with RT_E_INVALID, not launched).  A component's value is (float)i * 2^-7
 * ((double)i * 2^-7 on a float64 handle): range [-1, 1 - 2^-7], -128 is legal and maps to -1.  Both the conversion and
 * the multiplication are exact and happen in the scan kernel's load; everything after it is the complex64 path, detrend
 * by linearity and RT_FLAG_NO_LIN_DETREND included (unlike rt_process_u8, whose b / 127.5 - 1 lies half a step away
 * from these values and which always subtracts the mean first).  So the call delivers, byte for byte, the records, row
 * means and record cells of rt_process on the complex64 (float64 handle: complex128) array q * 2^-7 -- with 2 bytes of
 * memory traffic a sample instead of 8 (16).  No other scale is offered: a radio whose full scale sits elsewhere
 * differs by a constant, which calibration_db takes.  n_samples / stream_stride count samples.
 */
int rt_process_i8(rt_handle *h, const void *iq_i8_dev, int64_t n_samples, int64_t stream_stride);

/*
 * Same with IQ in host memory: copied (blocking) to an internal device buffer first -- one per call in flight, so
 * the caller may reuse its buffer as soon as the call returns and a call's samples stay in place until it is
 * fetched.  rt_process_u8_host takes what librtlsdr's read callback delivers (interleaved uint8 I,Q in host
 * memory): the direct replacement of `sdr.read_samples_async(self.process_samples, ...)` + packed_bytes_to_iq
 * (analyze.py:157) for a binding that registers a bytes callback instead.  rt_process_i16_host takes interleaved
 * int16 I,Q in host memory (what a CS16 / sc16 stream or a ci16_le recording delivers), 4 bytes a sample;
 * rt_process_i8_host interleaved int8 I,Q (a HackRF transfer, a CS8 / sc8 stream, a ci8 recording), 2 bytes a sample.
 */
int rt_process_host(rt_handle *h, const void *iq_host, int64_t n_samples, int64_t stream_stride);
int rt_process_u8_host(rt_handle *h, const void *iq_u8_host, int64_t n_samples, int64_t stream_stride);
int rt_process_i16_host(rt_handle *h, const void *iq_i16_host, int64_t n_samples, int64_t stream_stride);
int rt_process_i8_host(rt_handle *h, const void *iq_i8_host, int64_t n_samples, int64_t stream_stride);

/*
 * Wait for the OLDEST unfetched rt_process / rt_extract and copy its records, ordered by
 * (stream, fi, start) -- the reference's emission order per stream
 * (analyze.py:357, 364).  Records carry the shadow verdict; none is removed.
 * *n_out receives the number of records available; at most `cap` are written.
 * With out == NULL (or cap == 0) and records available the call is only a size
 * query: the result stays pending until it is fetched with a buffer.  A fetch
 * with a buffer consumes the call whatever `cap` is (records beyond `cap` are
 * lost; with cfg.lanes > 1 in every lane alike).
 * RT_E_CAPACITY: the result is truncated (and still delivered).  Neither the record
 * pool of a call (ABI v5) nor the per-stream record capacity (round 6) is a limit for
 * rt_process*: a call that finds more records than either holds grows it and is
 * analysed again inside this function -- only rt_extract (whose spectrogram the
 * library does not keep) or a device / host without memory for the larger areas end
 * in RT_E_CAPACITY, and then every stream still delivers the first records, in (bin,
 * start) order -- the reference's append order -- that fit (never an empty list).  RT_E_HOT_OVERFLOW (RT_MODE_SPARSE): no
 * result, the call is consumed.
 * If an rt_process fails, nothing stays enqueued for it (with lanes: in no lane),
 * and the look-back state is the one before the call.
 */
int rt_fetch(rt_handle *h, rt_record *out, size_t cap, size_t *n_out);

/*
 * extract_signals + filter_shadow_signals on a caller-supplied power
 * spectrogram (analyze.py:330-452 with explicit arguments): `spec_dev` is a
 * DEVICE pointer to [S][n_seg][n_bins] float32 (segment-major, the memory
 * layout SciPy's result has under its [F,T] view).  `last_dev` is the previous
 * spectrogram in the same layout with n_seg_last segments, or NULL
 * (`_spectrogram_last is None`).  n_bins is free (not tied to nperseg).
 * Does not touch the carried state.  Results via rt_fetch.
 */
int rt_extract(rt_handle *h, const float *spec_dev, int32_t n_seg, int32_t n_bins,
               const float *last_dev, int32_t n_seg_last);

/*
 * Debug / test entry: STFT power only.  Writes [S][T][nperseg] float32 to
 * `spec_dev` (device), T = n_samples / nperseg.  Synchronous.
 */
int rt_spectrogram(rt_handle *h, const void *iq_dev, int64_t n_samples, int64_t stream_stride,
                   float *spec_dev);

/*
 * Profiling aid: launches the scan kernel's load stream only (same grid, same
 * addresses, same prefetch; no arithmetic, no stores).  Its byte count is
 * known exactly -- S * (T + one halo segment per chunk) * nperseg * 8 -- so a
 * rocprofv3 --pmc FETCH_SIZE pass over it calibrates the counter for this
 * access shape (8-byte loads; MI355X_MICROARCH.md "HBM").  Synchronous.
 */
int rt_calibrate_read(rt_handle *h, const void *iq_dev, int64_t n_samples, int64_t stream_stride);

/* Per-call figures of the last rt_process (valid after rt_fetch). */
typedef struct rt_call_info {
    int32_t n_seg;            /* T of the call                                           */
    int32_t mode_used;        /* RT_MODE_DENSE, RT_MODE_SPARSE, RT_MODE_PREFILTER or RT_MODE_RUNFILTER */
    int32_t fell_back;        /* 1 if candidate lists overflowed and (part of) the call was re-run */
    int32_t n_dense_streams;  /* RT_MODE_AUTO: streams re-run dense on their own because only they overflowed
                                 (a few noisy SDRs in a batch; mode_used then still names the batch's path) */
    int64_t n_hot;            /* candidate cells emitted by the sparse scan              */
    int64_t n_records;        /* records produced                                        */
    float ms_stft;            /* RT_FLAG_TIMING: STFT/scan kernel, HIP events, ms        */
    float ms_detect;          /* RT_FLAG_TIMING: detect kernel(s), ms                    */
    float ms_total;           /* RT_FLAG_TIMING: first launch to last launch, ms         */
    int32_t segs_per_chunk;   /* the handle's chunk length (rt_config.segs_per_chunk, or what 0 chose); was reserved */
} rt_call_info;

int rt_get_call_info(rt_handle *h, rt_call_info *info);

/* Message of the last error on this handle (or of the last failed rt_create if h == NULL). */
const char *rt_last_error(rt_handle *h);

/*
 * ---- float64 handles (additive within ABI version 6) ----
 * pyrtlsdr delivers complex128 buffers and the reference then runs the whole path in float64 (SciPy keeps the input
 * dtype; thresholds and statistics are Python floats).  A handle made by rt_create_f64 does the same on the
 * GPU: the dense map in double precision, thresholds and statistics in float64.  Its limits:
 *   - rt_config.mode selects the dense path only: RT_MODE_AUTO means dense (rt_call_info.mode_used = RT_MODE_DENSE);
 *     RT_MODE_SPARSE, RT_MODE_PREFILTER and RT_MODE_RUNFILTER are RT_E_UNSUPPORTED.  The map-free path is opt-in by flag:
 *     RT_FLAG_F64_SPARSE (with RT_MODE_AUTO; any other mode: RT_E_INVALID) runs every call through a fused scan that
 *     transforms, sums the rows, keeps the look-back tail and emits only candidate cells (a cell not below the stream's
 *     absolute threshold, NaN included, or whose successor in time is one), and a detection that works from those lists:
 *     rt_call_info.mode_used = RT_MODE_SPARSE, no n_streams * T * nperseg * 8 byte map is allocated, the records are the
 *     dense path's (keys and verdicts; figures within float64 round-off of another summation order).  nperseg: a power of
 *     two 32 ... 4096 (else RT_E_UNSUPPORTED); max_samples / nperseg <= 2^20; not with RT_FLAG_RECORD_CELLS
 *     (RT_E_UNSUPPORTED).  On such a handle rt_config.hot_capacity counts candidate cells per stream and call: 0 = 4096,
 *     else 1024 ... 8192 (what one workgroup sorts in LDS; outside: RT_E_INVALID); a stream that emits more ends the call
 *     as RT_MODE_SPARSE does on a float32 handle -- rt_fetch_f64 returns RT_E_HOT_OVERFLOW, delivers nothing and consumes
 *     the call, whose look-back tail stays the next call's; there is no map to fall back to (create a dense handle, or set
 *     RT_FLAG_F64_RESCUE, below).
 *     rt_config.segs_per_chunk: segments of one stream a scan workgroup walks (0 = a default from the geometry); it sets
 *     the order of the row sums' partial sums, nothing else.  Everything listed below keeps its meaning, the four input
 *     formats, rt_set_present, rt_set_stream_params_f64 (the emission uses the stream's own threshold),
 *     rt_set_stream_settings_f64 and RT_FLAG_ROW_MEANS (every row's mean from the scan's sums) included; rt_extract_f64 and
 *     rt_spectrogram_f64 work on caller-supplied memory and are unchanged;
 *     RT_FLAG_F64_RESCUE (only together with RT_FLAG_F64_SPARSE; without it, or on rt_create: RT_E_INVALID, refused before
 *     any device is touched) takes the RT_E_HOT_OVERFLOW away.  A call in which no stream overflows runs exactly what it
 *     runs without the flag.  Otherwise rt_fetch_f64 analyses the present streams that emitted more than hot_capacity cells
 *     again, and only those: their segments are transformed once more with the scan's own arithmetic into a per-stream
 *     float64 map in a scratch area (allocated at first need, kept until rt_destroy; 256 MiB, or one stream's
 *     T * nperseg * 8 bytes where that is larger; more streams than it holds are taken in rounds), their rows are walked
 *     densely with the row sums of the scan and the call's look-back tail, and the call's records are ranked and packed
 *     again.  The records of such a stream are the ones a large enough hot_capacity would have given, byte for byte, the
 *     row means (RT_FLAG_ROW_MEANS) as well.  rt_call_info of a delivered call of such a handle: mode_used =
 *     RT_MODE_SPARSE, n_dense_streams = the streams analysed again, fell_back = 1 if there were any, n_hot = the cells the
 *     present streams emitted (the counters, not the cells stored; so on every RT_FLAG_F64_SPARSE handle).  No memory for the scratch: rt_fetch_f64 returns
 *     RT_E_NOMEM and consumes the call, whose look-back tail stays the next call's.  The cost is a second transform and
 *     a serial walk over T cells per bin for each such stream: a handle many of whose streams overflow belongs on the
 *     dense path (measured break-even at 4 096 streams x 300 kS, nperseg 256: about 4 % of the streams);
 *   - nperseg 8 ... 4096, or a power of two up to 8192 (a segment's transform in LDS: Bluestein's padded length M <= 8192
 *     complex doubles = 128 KiB); anything else is RT_E_UNSUPPORTED;
 *   - cfg->lanes must be 0 or 1 (RT_E_UNSUPPORTED otherwise): one launch sequence per call;
 *   - the native sinks of rt_format.h / rt_match.h take float32 rt_record arrays only.
 * rt_process / rt_process_host take complex128 (interleaved float64 I,Q; 16-byte aligned) on such a handle;
 * rt_process_u8 / rt_process_u8_host take the wire format and convert it as pyrtlsdr does, (double)b / 127.5 - 1.0;
 * rt_process_i16 / rt_process_i16_host take int16 pairs as (double)i * 2^-15 (exact), rt_process_i8 / rt_process_i8_host
 * int8 pairs as (double)i * 2^-7 (exact).
 * Every other rt_config field keeps its meaning (two calls in flight, record_capacity a starting size that grows,
 * rt_reset / rt_reset_stream, hip_stream); the float32 fields window / scale / threshold / snr_threshold /
 * calibration_db are replaced by rt_config_f64.  A float32 entry point that has a float64 twin (rt_fetch,
 * rt_set_stream_params, rt_extract, rt_spectrogram), or rt_calibrate_read, on a float64 handle -- and each twin on a
 * float32 handle -- is RT_E_INVALID, refused before anything is launched.
 */
typedef struct rt_config_f64 {
    const double *window;   /* host pointer, nperseg float64 coefficients                         */
    double scale;           /* 1/(fs*sum(w*w)) in float64 (_spectral_py.py:2087)                  */
    double threshold;       /* signal_threshold, linear (analyze.py:115), never rounded to float32 */
    double snr_threshold;   /* snr_threshold, linear (analyze.py:116)                             */
    double calibration_db;  /* only used to order maxima in the shadow filter                     */
} rt_config_f64;

/* rt_record with float64 figures (56 bytes) */
typedef struct rt_record_f64 {
    int32_t stream, fi, start, end; /* as in rt_record                                     */
    double max_p;                   /* max(data), linear                                   */
    double mean_p;                  /* mean(data), linear                                  */
    double std_db;                  /* std(10*log10(data)), population                     */
    double row_mean;                /* mean of the bin's row over the whole buffer         */
    int32_t shadowed;               /* 1 if filter_shadow_signals drops it                 */
    int32_t reserved;
} rt_record_f64;

/* Create a float64 handle.  `cfg` as for rt_create except its float32 window / scale / thresholds / calibration, which
 * `f64` replaces.  Arguments are checked before any device is touched; RT_E_NOMEM when the float64 map
 * (n_streams * (max_samples / nperseg) * nperseg * 8 bytes) does not fit. */
int rt_create_f64(const rt_config *cfg, const rt_config_f64 *f64, rt_handle **out);

/* rt_fetch of a float64 handle: the same contract, float64 records. */
int rt_fetch_f64(rt_handle *h, rt_record_f64 *out, size_t cap, size_t *n_out);

/* rt_set_stream_params of a float64 handle: HOST arrays of n_streams float64 (either may be NULL). */
int rt_set_stream_params_f64(rt_handle *h, const double *threshold, const double *calibration_db);

/* rt_extract of a float64 handle: `spec_dev` / `last_dev` are DEVICE pointers to [S][n_seg][n_bins] float64. */
int rt_extract_f64(rt_handle *h, const double *spec_dev, int32_t n_seg, int32_t n_bins, const double *last_dev,
                   int32_t n_seg_last);

/* rt_spectrogram of a float64 handle: complex128 `iq_dev` -> [S][T][nperseg] float64 at `spec_dev`.  Synchronous. */
int rt_spectrogram_f64(rt_handle *h, const void *iq_dev, int64_t n_samples, int64_t stream_stride, double *spec_dev);

/*
 * ---- row means: every bin's noise level (additive within ABI version 6) ----
 * The reference computes one noise figure per bin and buffer, `freq_avg = np.mean(row)` (analyze.py:373-375), and prints it
 * only as the `noise` of a Signal (analyze.py:446).  A handle created with RT_FLAG_ROW_MEANS (rt_create or rt_create_f64)
 * keeps that figure for EVERY bin of every stream; without the flag nothing is allocated or launched for it.
 *   - `out`: HOST memory, n == n_streams * nperseg entries, [stream][fi], fi in fftfreq order (the index of rt_record.fi).
 *   - the row means of the call the last rt_fetch / rt_fetch_f64 delivered (with RT_OK, or RT_E_CAPACITY).  Valid until the
 *     next rt_process*, rt_extract* or rt_reset on the handle; with two calls in flight: process k, process k + 1, fetch k,
 *     then the row means of k.
 *   - each entry is np.mean of the bin's row over the call's T segments in the handle's arithmetic (float32: the float64 sum
 *     of the partial row sums, rounded once and divided by T in float32; float64: the float64 sum divided by T).  For every
 *     record r of the call, out[r.stream * nperseg + r.fi] == r.row_mean bit for bit, in every mode and lane split, after
 *     AUTO's re-runs and after a re-analysis on record growth.
 *   - T == 0 (a buffer shorter than nperseg): every entry is NaN, as np.mean of an empty row.
 *   - RT_E_INVALID: null handle or `out`, a handle without the flag, a wrong n, no delivered call (or its row means are no
 *     longer valid, see above), a delivered call that was an rt_extract (the caller holds that map), and the float32 entry on
 *     a float64 handle or the reverse.
 * A laned handle gathers its lanes' row means in stream order.
 */
int rt_fetch_row_means(rt_handle *h, float *out, size_t n);       /* float32 handle */
int rt_fetch_row_means_f64(rt_handle *h, double *out, size_t n);  /* float64 handle */

/*
 * ---- record cells: the spectrogram cells behind every record (additive within ABI version 6) ----
 * For every plateau it reports the reference forms `data`, the cells the plateau consists of (analyze.py:437-440:
 * `fft[start:end]`, or `concatenate((_spectrogram_last[fi][start:], fft[:end]))` when it reaches back into the previous
 * buffer), reduces it to max / mean / std (analyze.py:442-445) and drops it.  A handle created with RT_FLAG_RECORD_CELLS
 * (rt_create or rt_create_f64) keeps those cells for every record of a call; without the flag nothing is allocated and no
 * launch is added, removed or changed.
 *   - the call concerned is the one the last rt_fetch / rt_fetch_f64 delivered IN FULL (RT_OK, cap >= *n_out).  Record i below
 *     is the i-th record that fetch wrote: all of them, shadowed ones included, in (stream, fi, start) order, over all lanes.
 *   - `offsets`: HOST memory, n_offsets == n_records + 1 entries (or NULL: not wanted); offsets[0] == 0,
 *     offsets[i + 1] - offsets[i] == end_i - start_i, *n_cells == offsets[n_records].
 *   - `cells`: HOST memory, `cap` entries.  Cell k of record i -- cells[offsets[i] + k] -- is the spectrogram cell of bin fi_i at
 *     segment start_i + k; a negative segment counts back from the end of the stream's previous buffer, exactly as
 *     rt_record.start does (analyze.py:383-388, 438).  Linear power, uncalibrated, in the handle's arithmetic.
 *   - each cell is bit for bit the value the detection used for the record's decision and statistics -- gathered from the map,
 *     the candidate lists and the look-back columns the detection read, not computed again.  Hence for every record
 *     max(cells) == max_p exactly (NaN as np.max propagates it), and mean_p, std_db are the canonical statistics (64 interleaved
 *     float64 partials, cell k to partial k mod 64, folded by halving) of them.
 *   - cells == NULL or cap == 0: a size query (*n_cells and, if given, the offsets); nothing is consumed.  The data stay valid
 *     until the next rt_process*, rt_extract* or rt_reset on the handle; with two calls in flight: process k, process k + 1,
 *     fetch k, then the cells of k.  cap < *n_cells with a buffer: RT_E_CAPACITY, nothing written to `cells`.
 *   - a call without records: offsets[0] = 0, *n_cells = 0, RT_OK.
 *   - RT_E_INVALID: null handle or `n_cells`, a wrong n_offsets, a handle without the flag, no delivered call (or one no longer
 *     valid, see above), a call delivered truncated (RT_E_CAPACITY from the fetch), a delivered rt_extract* call (the caller
 *     holds that map), and the float32 entry on a float64 handle or the reverse.  Refused before anything is launched or copied.
 *   - RT_E_NOMEM: the device could not hold the call's cells (the pool grows on demand, inside rt_fetch, like the record pool).
 */
int rt_fetch_record_cells(rt_handle *h, int64_t *offsets, size_t n_offsets, float *cells, size_t cap, size_t *n_cells);       /* float32 handle */
int rt_fetch_record_cells_f64(rt_handle *h, int64_t *offsets, size_t n_offsets, double *cells, size_t cap, size_t *n_cells);  /* float64 handle */

/*
 * ---- per-stream detection settings (additive within ABI version 6) ----
 * In the reference every SDR is a SignalAnalyzer of its own, built from its own snr_threshold_db, signal_min_duration_ms and
 * signal_max_duration_ms (analyze.py:113-116) beside the threshold and calibration of rt_set_stream_params.  These entries give
 * every stream of a handle its own values: HOST arrays of n_streams entries (linear SNR threshold; durations in seconds), each
 * of which may be NULL = rt_config's value for every stream.  All three NULL puts the handle back to rt_config's values.
 *   - rt_config.min_duration_s / max_duration_s are the handle's ENVELOPE: every stream's minimum must be >= the handle's, every
 *     maximum <= the handle's (RT_E_INVALID otherwise, the message names the stream).  The look-back depth, the availability of
 *     RT_MODE_PREFILTER and the run length of RT_MODE_RUNFILTER stay derived from the envelope -- supersets for every stream --
 *     while the detection applies each stream's own probe stride (analyze.py:354, 364) and duration gates (:427-433), and
 *     RT_MODE_RUNFILTER's per-bin thresholds take each stream's own SNR threshold.
 *   - RT_E_INVALID as well: a snr_threshold that is <= 0 or not finite, a duration that is not finite, unfetched calls pending
 *     (as rt_set_stream_params: AUTO may still re-run them with the settings they were enqueued with), the float32 entry on a
 *     float64 handle or the reverse.  min > max is accepted, as the reference accepts it: such a stream finds nothing.  Every
 *     refusal happens before anything is copied or launched; the handle then analyses on as if the call had not been made.
 *   - a stream whose settings CHANGE starts its next buffer without look-back, as after rt_reset_stream (a new setting is a new
 *     analyzer in the reference, analyze.py:128); streams whose values stay keep theirs.
 *   - applies to rt_process* and rt_extract* calls enqueued afterwards; with cfg.lanes > 1 every lane takes its slice.
 *   - a handle on which the entry was never called launches exactly what it launched before: no kernel, copy or allocation.
 * sample_rate, nperseg and the window stay per handle: they set the scan's geometry and scale.
 */
int rt_set_stream_settings(rt_handle *h, const float *snr_threshold, const double *min_duration_s,
                           const double *max_duration_s);      /* float32 handle */
int rt_set_stream_settings_f64(rt_handle *h, const double *snr_threshold, const double *min_duration_s,
                               const double *max_duration_s);  /* float64 handle */

/*
 * ---- streams that sit out a call (additive within ABI version 6) ----
 * In the reference every SDR is a SignalAnalyzer of its own: its callback comes when ITS radio delivers, and its
 * `_spectrogram_last` (analyze.py:268) is the buffer that radio delivered before, whatever the other radios did meanwhile.
 * `present` is a HOST array of n_streams bytes, non-zero = the stream takes part; NULL = every stream.
 *   - sticky: it applies to every rt_process* call enqueued afterwards, on float32 and float64 handles alike; with cfg.lanes > 1
 *     every lane takes its slice.  It may be called while calls are pending: each call keeps the mask it was enqueued with, and
 *     every re-analysis of that call inside rt_fetch* (AUTO's level-up, the partial dense re-run, stale thresholds, growth of the
 *     record pool, the record capacity or the cell pool, the detrend guard) uses that snapshot.
 *   - rt_extract*, rt_spectrogram* and rt_calibrate_read ignore the mask.
 *   - a handle on which the entry was never called launches exactly what it launched before: no kernel, copy or allocation is
 *     added and no kernel argument changes meaning.  The first call allocates the mask rows (RT_E_NOMEM if that fails).
 * A stream that is ABSENT from a call:
 *   - no effect from its row: its row of the IQ buffer is not read and has no effect on anything -- no records, no candidate
 *     cells, no contribution to rt_call_info, to AUTO's level decisions, to the overflow or inconsistency marks or to the
 *     detrend guard;
 *   - state as if no call happened: its next present buffer is analysed exactly as by a reference analyzer that was not called
 *     in between -- it looks back into its own last present buffer, and `start_min` (analyze.py:383) comes from THAT buffer's
 *     segment count, not from the handle's latest call.  After any number of absent calls;
 *   - deferred changes: a pending rt_reset_stream, or the restart a changed threshold or setting brings, takes effect at its
 *     next present call;
 *   - row means (RT_FLAG_ROW_MEANS): its [nperseg] entries for that call are NaN, as at T == 0;
 *   - record cells (RT_FLAG_RECORD_CELLS): it has no records, hence no cells;
 *   - whole-call errors stay: a call in which every stream is absent is legal (RT_OK, zero records), and what concerns the call
 *     as a whole is unchanged -- RT_E_ONE_SEGMENT, the alignment of the pointer, max_samples.
 * RT_E_INVALID: null handle.
 */
int rt_set_present(rt_handle *h, const uint8_t *present);

/*
 * ---- consecutive buffers of one recording in one call (additive within ABI version 6) ----
 * A recording is one stream; analysed callback by callback it costs one rt_process* + rt_fetch per buffer.  What buffer k + 1
 * needs from buffer k is only `_spectrogram_last` (analyze.py:268): the last K columns of buffer k, which every scan writes
 * anyway.  rt_set_chain lets the streams of ONE call be consecutive buffers: a contiguous recording is [links][B] with
 * stream_stride = B.
 *   - grouping: links >= 2 groups the handle's streams into RUNS of `links` consecutive indices (run r = streams r * links ...
 *     r * links + links - 1); n_streams % links != 0 is RT_E_INVALID.  Within one rt_process* call the present streams of a run
 *     are consecutive buffers of one analyzer of the reference, in index order.
 *   - look-back: the buffer at stream s looks back into the buffer of the nearest present stream before it in its run, in the
 *     same call; its `start_min` (analyze.py:383) comes from that buffer's segment count, the call's.  A run's first present
 *     stream looks back into the run's LAST present stream of the latest earlier call in which the run had a present stream,
 *     with that call's segment count; it has no look-back if there was no such call.
 *   - links 0 or 1 turns chaining off.  A call that changes the value forgets all look-back, as rt_reset.
 *   - refused: RT_E_INVALID (the message says "pending") while unfetched calls are pending; RT_E_UNSUPPORTED on a float64 handle
 *     and -- a limit of this version: lanes cut the streams into groups that a run may straddle -- on a handle created with
 *     lanes > 1.  Both before any device work.  RT_E_NOMEM if the first call with links >= 2 cannot allocate its two
 *     [n_streams][K][nperseg] float buffers (one per call slot).
 *   - rt_reset_stream(h, s), a changed threshold, a changed setting keep their per-index meaning: the buffer at stream s of the
 *     next call in which s is present starts without look-back -- a cut in the recording in front of it; the streams behind it
 *     in the run chain on as usual.  rt_reset cuts in front of every run's first stream.
 *   - uniform values per run: rt_set_stream_params / rt_set_stream_settings on a chained handle must give all streams of a run
 *     the same threshold, calibration and settings (RT_E_INVALID otherwise, the message names the run), and rt_set_chain on a
 *     handle whose current per-stream values differ inside a run is refused the same way: the sparse scans keep a look-back
 *     cell iff the later cells pass the WRITING stream's threshold.
 *   - rt_set_present works as documented for an absent stream's own row, records, row means and rt_call_info; the one
 *     difference is who follows whom, as above.  Any mask is legal ("the last call of a recording has fewer buffers",
 *     "recordings of different lengths in one batch").  n_samples and stream_stride stay per call: all links of a call have the
 *     same length, a recording's short last buffer is one more call with one link present.
 *   - unchanged: records (`stream` is the stream index, a negative `start` counts back from the end of the predecessor buffer),
 *     RT_FLAG_ROW_MEANS, RT_FLAG_RECORD_CELLS (gathered through the look-back the detection read), every rt_mode, every nperseg
 *     and input format of a float32 handle, two calls in flight, every re-analysis inside rt_fetch.  rt_extract, rt_spectrogram
 *     and rt_calibrate_read ignore chaining.
 *   - differences from `links` sequential calls of a plain handle: RT_MODE_RUNFILTER's quiet levels and the detrend guard's
 *     marks stay per stream INDEX.  The quiet levels only steer selectivity and are verified per call, so the records are exact
 *     either way.  A guard mark changes the form of the transform for that index from then on, so a chained run can differ in
 *     float32 round-off from a sequential run after a mark.
 *   - a handle on which the entry was never called with links >= 2 launches exactly what it launched before: no kernel, copy
 *     or allocation is added and no kernel argument changes meaning.
 * RT_E_INVALID as well: null handle, links < 0.
 */
int rt_set_chain(rt_handle *h, int32_t links);

/*
 * ---- record IQ: the samples behind every record (additive within ABI version 6) ----
 * The reference hands on a Signal's figures and drops the samples.  Whoever works with a detection afterwards -- a frequency
 * estimate finer than fs / nperseg, a pulse edge finer than one segment, a coded-ID decode, cutting bursts out of an archive --
 * needs the IQ of the pulse, and would have to keep every buffer of every stream (and the one before it, for records whose
 * `start` is negative) to slice it on the host.  rt_set_record_iq makes the handle keep what that takes -- the tail of every
 * stream's previous buffer, as samples -- and rt_fetch_record_iq hands out each record's samples, cut from the caller's own bytes.
 *   - rt_set_record_iq(h, m): 0 <= m <= 1024 turns the feature on with a margin of m whole segments on either side of a record;
 *     m < 0 turns it off.  On every handle kind: float32 handles in every mode, nperseg and lane count, chained handles, float64
 *     handles (dense, RT_FLAG_F64_SPARSE, with RT_FLAG_F64_RESCUE) -- the samples are gathered from the delivered records and the
 *     IQ alone.  Refused (RT_E_INVALID, the message says "pending") while unfetched calls are pending; RT_E_INVALID as well: null
 *     handle, m > 1024.  A call that changes m, or turns the feature off, forgets the held sample tails.  RT_E_NOMEM: no memory
 *     for the bookkeeping rows.
 *   - a handle on which the entry was never called with m >= 0 allocates, copies and launches exactly what it did before; no
 *     kernel argument changes meaning.  With the feature on every rt_process* adds one streaming copy in front of its scan (the
 *     last min(T, K + m) whole segments of every present stream, K = the handle's look-back columns) and every delivering rt_fetch
 *     one gather; the analysis -- records, row means, record cells -- is untouched, byte for byte.
 *   - memory: three tail rows per stream of (K + m) * nperseg samples, sized by the widest input format the handle has seen
 *     (allocated by the first rt_process* after the entry; RT_E_NOMEM from that call if the device cannot hold them, and the call
 *     is not enqueued), plus a byte pool per call slot that grows on demand inside rt_fetch.
 * What rt_fetch_record_iq delivers.  The call concerned is the one the last rt_fetch / rt_fetch_f64 delivered IN FULL (RT_OK,
 * cap >= *n_out), as for rt_fetch_record_cells; record i is the i-th record that fetch wrote, shadowed ones included, in (stream,
 * fi, start) order over all lanes.  With N = nperseg, T = the call's segment count and, for record i of stream s,
 *     D(s) = min(T_pred, K + m)  if the detection of this call had look-back for s and the predecessor buffer -- the one the
 *            detection looked back into: the stream's own last present buffer (after any number of absent calls); on a chained
 *            handle the nearest present stream before it in its run, in the same call, or for a run's first present stream the
 *            run's remembered stream of the earlier call -- came in the same input format and its tail is held;
 *     D(s) = 0  otherwise: the first call, after rt_reset / rt_reset_stream / a changed threshold or setting, T_pred == 0, another
 *            format, the first call after rt_set_record_iq turned the feature on or changed m;
 * record i delivers the WHOLE segments
 *     first_seg[i] = max(start_i - m, -D(s))   ...   min(end_i + m, T) - 1.
 * Segment t >= 0 is samples [t * N, (t + 1) * N) of the call's buffer of stream s.  Segment -d is samples [(T_pred - d) * N,
 * (T_pred - d + 1) * N) of the predecessor buffer: counted from that buffer's last WHOLE segment, exactly as rt_record.start counts
 * cells.  The predecessor's ragged remainder (its n_samples % N last samples, which no segment covers) is never delivered: in time
 * it lies between segment -1 and segment 0, so a snippet that crosses the boundary is contiguous in time only where that
 * remainder is empty.
 *   - the payload is the caller's own bytes in the call's input format, nothing is converted: *bytes_per_sample = 8 (complex64),
 *     16 (complex128 on a float64 handle), 2 (uint8, int8), 4 (int16).  Bit for bit the bytes at those places of the buffers the
 *     caller passed, device pointers and the _host entries (the staged copy) alike.
 *   - `offsets`: HOST memory, n_offsets == n_records + 1 entries (or NULL: not wanted), in SAMPLES; offsets[0] == 0,
 *     *n_bytes == offsets[n_records] * *bytes_per_sample.  `first_seg`: HOST memory, n_first == n_records entries (or NULL);
 *     first_seg[i] <= start_i, except where D(s) clips the lead: it is 0 for a negative start_i when D(s) == 0.
 *   - `iq`: HOST memory, cap_bytes bytes.  iq == NULL or cap_bytes == 0: a size query (*n_bytes, *bytes_per_sample and, if given,
 *     offsets and first_seg); nothing is consumed.  cap_bytes < *n_bytes with a buffer: RT_E_CAPACITY, nothing written to `iq`.
 *   - the data stay valid until the next rt_process*, rt_extract*, rt_reset or rt_set_record_iq on the handle; with two calls in
 *     flight: process k, process k + 1, fetch k, then the IQ of k.  (The samples are gathered inside the delivering rt_fetch, so
 *     the call's IQ need not outlive that fetch.)
 *   - a call without records: offsets[0] = 0, *n_bytes = 0, RT_OK.  An absent stream (rt_set_present) has no records; its held
 *     tail stays its own for its next present call.  A failed rt_process* leaves the held tails as they were before it.
 *   - RT_E_INVALID, refused before anything is copied or launched: null handle, `n_bytes` or `bytes_per_sample`; the feature is
 *     off; a wrong n_offsets / n_first; no delivered call, or one no longer valid (see above), or one enqueued before the feature
 *     was turned on; a call delivered truncated (RT_E_CAPACITY from the fetch, or cap < *n_out); a delivered rt_extract* call.
 *   - RT_E_NOMEM: the device could not hold the call's samples (the pool grows on demand, inside rt_fetch, like the cell pool).
 */
int rt_set_record_iq(rt_handle *h, int32_t margin_segments);   /* >= 0: on, with that margin; < 0: off */
int rt_fetch_record_iq(rt_handle *h, int64_t *offsets, size_t n_offsets, int32_t *first_seg, size_t n_first,
                       void *iq, size_t cap_bytes, size_t *n_bytes, int32_t *bytes_per_sample);

/*
 * ---- record STFT: one complex STFT value per delivered segment (additive within ABI version 6) ----
 * A frequency finer than fs / nperseg or a phase track over a pulse needs, per segment, one complex number: the STFT value of the
 * record's bin.  Its |.|^2 is the cell rt_fetch_record_cells delivers; its phase is what the scans compute and drop.  That is
 * nperseg times less data than the snippet rt_fetch_record_iq hands out (8 bytes a segment instead of nperseg * 8), computed on
 * the device from the snippets the delivering rt_fetch gathered.
 *   - the call and the records are those of rt_fetch_record_iq: the call the last rt_fetch / rt_fetch_f64 delivered in full; record
 *     i is the i-th record that fetch wrote, shadowed ones included, over all lanes; it delivers the same whole segments
 *     first_seg[i] ... min(end_i + m, T) - 1, margin included.  rt_set_record_iq must be on; there is no switch of its own.
 *   - `offsets`: HOST memory, n_offsets == n_records + 1 entries (or NULL), in SEGMENTS: rt_fetch_record_iq's offsets divided by
 *     nperseg.  `first_seg`: as there.  *n_cells == offsets[n_records].
 *   - `values`: HOST memory, cap_cells interleaved (re, im) pairs -- 2 * cap_cells floats (doubles: the _f64 entry).  values == NULL
 *     or cap_cells == 0: a size query.  cap_cells < *n_cells with a buffer: RT_E_CAPACITY, nothing written.
 *   - a value, for record (s, fi) and a delivered segment whose N = nperseg samples are x[0 .. N), converted as the scans convert
 *     the call's format (complex64 as is; uint8 b / 127.5 - 1 by the scan kernels' one float32 fma; int16 * 2^-15; int8 * 2^-7; a
 *     float64 handle: complex128 as is and the float64 conversions):
 *         value = sqrt(scale) * sum_n w[n] * (x[n] - mean(x)) * exp(-2 pi i fi n / N)
 *     w = the handle's window, scale = rt_config.scale (rt_config_f64.scale), fi = rt_record.fi (fftfreq order).  This is
 *     scipy.signal.spectrogram(..., noverlap=0, return_onesided=False, mode='complex') at that bin and segment; in exact
 *     arithmetic |value|^2 is the spectrogram cell.  On a float32 handle sqrt(scale) is evaluated in float64 and rounded once.
 *   - the value depends on the snippet and the bin alone: the same samples give the same bytes on every handle kind (mode, lanes,
 *     chained, masked) and on every fetch of the same call.  A segment whose samples are all one finite value gives exactly 0 + 0i
 *     (the mean is taken about the segment's first sample), at every nperseg.  A non-finite sample makes the values of its segment
 *     non-finite (NaN for NaN) and of no other.
 *   - lazy: rt_process* and rt_fetch do nothing for it.  The first call of the entry on a handle allocates an nperseg-entry
 *     twiddle table (and a float32 handle's copy of the window); the first call for a delivered call builds that call's values in a
 *     pool per call slot that grows on demand, by one kernel on the gather's stream, waited for.  A repeated call copies them again.
 *     A handle that never calls the entry allocates and launches what it did before.
 *   - validity: exactly as the record IQ (until the next rt_process*, rt_extract*, rt_reset or rt_set_record_iq).
 *   - RT_E_INVALID, before anything is launched or copied: all that rt_fetch_record_iq refuses, with its messages under this
 *     entry's name; a null `n_cells`; a wrong n_offsets / n_first; rt_fetch_record_stft on a float64 handle and
 *     rt_fetch_record_stft_f64 on a float32 one.  RT_E_NOMEM: the table or the value pool could not be allocated.
 */
int rt_fetch_record_stft(rt_handle *h, int64_t *offsets, size_t n_offsets, int32_t *first_seg, size_t n_first,
                         float *values, size_t cap_cells, size_t *n_cells);      /* float32 handle */
int rt_fetch_record_stft_f64(rt_handle *h, int64_t *offsets, size_t n_offsets, int32_t *first_seg, size_t n_first,
                             double *values, size_t cap_cells, size_t *n_cells); /* float64 handle */

/*
 * ---- record STFT at a sub-segment hop: one complex value per FRAME (additive within ABI version 6) ----
 * rt_fetch_record_stft's values lie a whole segment apart, so a phase advance between them gives a frequency only within half a
 * bin, and an edge only to a segment.  This entry delivers the same single-bin transform for frames every h = N / k samples
 * (N = nperseg, k = hop_div): the advance between frames is 2 pi delta / k for a tone delta bins off the centre, and the
 * amplitude is sampled k times a segment.  A frame is a segment that starts elsewhere.
 *   - `hop_div`: 1 <= k <= 16 and N % k == 0; anything else is RT_E_INVALID, the message names k and N, and it is refused before
 *     anything is launched or copied.
 *   - the call, the records and `first_seg` are exactly those of rt_fetch_record_stft: record i has the delivered segments
 *     first_seg[i] ... last_i.  Its PREDECESSOR PART are the Lp segments below 0 (Lp = clamp(-first_seg[i], 0, L) of its L
 *     delivered segments), its OWN PART the Lc = L - Lp from 0 on.
 *   - frames: a part of L >= 1 segments has (L - 1) * k + 1 frames, frame j the N samples from sample j * h of the part; a part
 *     of no segment has none.  A record delivers its predecessor part's frames, then its own part's.  No frame straddles the two
 *     parts, on any handle kind, also where the predecessor buffer left no ragged remainder: one rule.
 *   - `offsets`: HOST memory, n_offsets == n_records + 1 entries (or NULL), counting FRAMES.  *n_frames == offsets[n_records].
 *   - `values`: HOST memory, cap_frames interleaved (re, im) pairs.  values == NULL or cap_frames == 0: a size query.
 *     cap_frames < *n_frames with a buffer: RT_E_CAPACITY, nothing written.
 *   - a value is rt_fetch_record_stft's formula on the frame's N samples x[0 .. N): the same conversions, window, sqrt(scale),
 *     bin fi and mean (over the frame), the phase reference frame-local:
 *         value = sqrt(scale) * sum_n w[n] * (x[n] - mean(x)) * exp(-2 pi i fi n / N)        n from the frame's start
 *     i.e. scipy.signal.spectrogram(part, nperseg=N, noverlap=N - h, detrend='constant', return_onesided=False,
 *     mode='complex')[fi, j].  (The bin's own rotation over a hop, exp(2 pi i fi / k), is left in between consecutive frames.)
 *   - bit identity: frame j with j % k == 0 is a delivered segment, and its value is the bytes rt_fetch_record_stft gives for
 *     that segment; with k == 1 the whole output is that entry's.  A value depends on the frame's samples and the bin alone: the
 *     same samples give the same bytes on every handle kind, on every fetch and in every order of calls.  A frame whose samples
 *     are all one finite value is exactly 0 + 0i; a non-finite sample makes exactly the frames that cover it non-finite.
 *   - lazy: rt_process*, rt_fetch and rt_fetch_record_stft allocate, copy and launch what they do without this entry.  The
 *     entry's first call for a delivered call builds the values for that k in a pool of its own per call slot (it grows on
 *     demand, is separate from rt_fetch_record_stft's and remembers the k it holds), by one kernel on the gather's stream, waited
 *     for.  A repeated call with the same k copies; another k builds again.  The twiddle table and the float32 window copy are
 *     the ones rt_fetch_record_stft uses, made by whichever of the two entries is called first.
 *   - size query, RT_E_CAPACITY, validity, RT_E_NOMEM and every refusal: rt_fetch_record_stft's, under this entry's name; the
 *     wrong twin is refused too.
 */
int rt_fetch_record_stft_hop(rt_handle *h, int32_t hop_div, int64_t *offsets, size_t n_offsets, int32_t *first_seg, size_t n_first,
                             float *values, size_t cap_frames, size_t *n_frames);      /* float32 handle */
int rt_fetch_record_stft_hop_f64(rt_handle *h, int32_t hop_div, int64_t *offsets, size_t n_offsets, int32_t *first_seg, size_t n_first,
                                 double *values, size_t cap_frames, size_t *n_frames); /* float64 handle */

/*
 * ---- the bins beside each record's bin: 2 w + 1 complex values per FRAME (additive within ABI version 6) ----
 * rt_fetch_record_stft_hop looks at one bin, rt_record.fi.  What the pulse looks like beside it -- a keyed carrier about
 * 1 / duration wide or a broadband click, how much energy the neighbour bin holds, where the peak of a record with a single
 * inside frame lies between bins -- takes the neighbouring bins of the same frames.  This entry delivers them.
 *   - the call, the records, their order, `first_seg`, the two parts and the frames are exactly those of
 *     rt_fetch_record_stft_hop at the same `hop_div` = k.  `offsets` counts FRAMES; *n_frames == offsets[n_records].
 *   - `hop_div`: 1 <= k <= 16 and N % k == 0 (N = nperseg).  `half_width`: 0 <= w <= 8 with B = 2 w + 1 <= N.  Anything else is
 *     RT_E_INVALID, the message names k, w and N, and it is refused before anything is launched or copied.
 *   - `values`: HOST memory, cap_frames * B interleaved (re, im) pairs, frame-major.  Column order: column j of a frame belongs
 *     to d = j - w, and its bin is (fi + d) mod N in the index space of rt_record.fi (fftfreq order).  The band is circular:
 *     beside bin N - 1 lies bin 0, and beside N / 2 - 1 lies the most negative frequency.  values == NULL or cap_frames == 0: a
 *     size query.  cap_frames < *n_frames with a buffer: RT_E_CAPACITY, nothing written.
 *   - a value is rt_fetch_record_stft_hop's formula with the column's bin in place of fi: the same conversions, window,
 *     sqrt(scale), mean about the frame's first sample, and the phase counted from the frame's start,
 *         value[j] = sqrt(scale) * sum_n w[n] * (x[n] - mean(x)) * exp(-2 pi i ((fi + j - w) mod N) n / N)
 *     Per bin the operations and their order are that entry's -- four fmas a sample against the table twiddle, then the group
 *     butterfly -- so a value depends on the frame's samples and the bin alone.  (The centre bin's products are NOT rotated by
 *     W^(d n) into the neighbours: cheaper, and it would round differently.)
 *   - bit identity: (1) column w (d = 0) is the bytes of rt_fetch_record_stft_hop at that k; with half_width == 0 the whole
 *     output is that entry's.  (2) For two records of one stream whose bins lie d apart, and frames of the same part at the same
 *     position, column w + d of the one is the bytes of column w of the other.  (3) The same samples give the same bytes on every
 *     handle kind, on every fetch and in every order of calls.  (4) A frame whose samples are all one finite value is exactly
 *     0 + 0i in every column.  (5) A non-finite sample makes exactly the frames that cover it non-finite, in every column.
 *   - lazy: rt_process*, rt_fetch and the other record entries allocate, copy and launch what they do without this one.  The
 *     entry's first call for a delivered call builds the values for (k, w) in a pool of its own per call slot (it grows on
 *     demand, its bytes computed in 64 bits, and remembers the (k, w) it holds), by one kernel on the gather's stream, waited
 *     for.  The same (k, w) again copies; another pair builds again.  The twiddle table and the float32 window copy are the ones
 *     the STFT entries share, made by whichever entry is called first.
 *   - validity, RT_E_NOMEM (the handle is left as it was, the bytes are in the message) and every refusal:
 *     rt_fetch_record_stft_hop's, under this entry's name; the wrong twin is refused too.
 */
int rt_fetch_record_band(rt_handle *h, int32_t hop_div, int32_t half_width, int64_t *offsets, size_t n_offsets, int32_t *first_seg,
                         size_t n_first, float *values, size_t cap_frames, size_t *n_frames);      /* float32 handle */
int rt_fetch_record_band_f64(rt_handle *h, int32_t hop_div, int32_t half_width, int64_t *offsets, size_t n_offsets, int32_t *first_seg,
                             size_t n_first, double *values, size_t cap_frames, size_t *n_frames); /* float64 handle */

/*
 * ---- per-record estimates from the frames, reduced on the device (additive within ABI version 6) ----
 * What a caller makes of rt_fetch_record_stft_hop's frames is one row per record: the tone's offset from its bin (pulse pair),
 * its coherence, the pulse's level and its rise and fall.  This entry reduces the frames where they lie; they are not copied to the
 * host.  One entry serves float32 and float64 handles: the rows are float64 either way, only the frames read differ.
 *   - `hop_div`: k as for rt_fetch_record_stft_hop (1 ... 16, a divisor of N = nperseg; k == 1: the frames are the segments);
 *     anything else is RT_E_INVALID, refused before anything is launched or copied.  h = N / k.
 *   - the call, the records and their order are rt_fetch_record_stft_hop's; rt_set_record_iq must be on.
 *   - `out`: HOST memory, `cap` rows.  out == NULL or cap == 0: a size query, *n_out = the records.  cap < *n_out with a buffer:
 *     RT_E_CAPACITY, nothing written.  Validity, RT_E_NOMEM and every refusal: rt_fetch_record_stft_hop's, under this entry's name.
 *   - a frame's position is its first sample relative to sample 0 of the call's buffer (frames of the predecessor part are
 *     negative: segment -1 starts at -N).  The INSIDE frames of record (start, end) are those with start * N <= position and
 *     position + N <= end * N.  |c| = sqrt(re * re + im * im) in float64, +inf where a component is infinite.
 *   - pairs are consecutive inside frames of the same part; no pair spans the predecessor part and the record's own, at any k.
 *       R = sum c[t + 1] conj(c[t]), multiplied by exp(-2 pi i (fi mod k) / k) where k > 1 (the bin's own turn over one hop)
 *       M = sum |c[t + 1]| |c[t]|
 *       offset_bins = atan2(r_im, r_re) / (2 pi) * k  (bins; times sample_rate / N for Hz), coherence = |R| / M
 *     R is formed as record_fine forms it, re + 1j * im: r_re is NaN where r_im is infinite or NaN.
 *     both NaN when n_pairs == 0; M == 0 gives coherence 0 / 0 = NaN; where R is exactly zero the sign of offset_bins is atan2's
 *     and no part of the contract.
 *   - level: the exact median of |c| over the inside frames (the mean of the two middle values of an even count); NaN when there
 *     is none, and when any of them is NaN.
 *   - rise, fall: half = level / 2; unless half > 0, both are NaN.  up0 is the first inside frame with |c| >= half, q the nearest
 *     earlier frame of the same part -- among all delivered frames, not only the inside ones -- with |c[q]| < half (a NaN |c| is
 *     passed over).  rise = position[q] + (half - |c[q]|) / (|c[q + 1]| - |c[q]|) * h + N / 2; NaN where the part ends before such
 *     a q.  fall mirrors it forward from the last inside frame with |c| >= half.
 *   - the same frames give the same row bytes: on every handle kind, on every fetch and in every order of calls.
 *   - lazy: rt_process*, rt_fetch and the other fetch entries allocate, copy and launch what they do without this entry (the gather
 *     notes the records' start and end on the host).  The entry's first call for a delivered call and k makes sure the hop pool
 *     holds the frames for k (as rt_fetch_record_stft_hop would, without the copy), uploads a plan of 48 bytes a record, runs one
 *     kernel on the gather's stream, waits, and copies the rows down.  A repeated call with the same k copies the rows again; a
 *     later rt_fetch_record_stft_hop with the same k copies without rebuilding.
 */
typedef struct rt_record_estimate {
    double r_re, r_im;     /* R, turned back                                                  */
    double pair_mag;       /* M                                                               */
    double offset_bins;    /* NaN when n_pairs == 0                                           */
    double coherence;      /* NaN when n_pairs == 0                                           */
    double level;          /* NaN when n_inside == 0                                          */
    double rise, fall;     /* samples relative to sample 0 of the call's buffer, or NaN       */
    int32_t n_pairs, n_inside;
} rt_record_estimate;      /* 72 bytes */

int rt_fetch_record_estimates(rt_handle *h, int32_t hop_div, rt_record_estimate *out, size_t cap, size_t *n_out);

/*
 * ---- per-record band spectrum, reduced on the device (additive within ABI version 6) ----
 * What a caller makes of rt_fetch_record_band's frames is one short row per record: how wide the pulse is, where its peak lies
 * between bins, how much of it sits in the centre bin.  This entry reduces the band where it lies; the frames are not copied to
 * the host.  One entry serves float32 and float64 handles: rows, means and peaks are float64 either way, only the frames read
 * differ (a float32 value is widened first).
 *   - the call, the records, their order, the two parts and the frames are exactly rt_fetch_record_band's at the same
 *     (hop_div, half_width) = (k, w); rt_set_record_iq must be on.  B = 2 w + 1, column j belongs to d_j = j - w as there.
 *   - `hop_div`: 1 <= k <= 16 and N % k == 0 (N = nperseg).  `half_width`: 0 <= w <= 8 with 2 w + 1 <= N.  Anything else is
 *     RT_E_INVALID, the message names k, w and N, and it is refused before anything is launched or copied.
 *   - `rows`: HOST memory, `cap` rows.  `mean`, `peak`: HOST memory, cap * B doubles each, record-major; either may be NULL: not
 *     wanted.  rows == NULL or cap == 0: a size query, *n_out = the records.  cap < *n_out with a buffer: RT_E_CAPACITY, nothing
 *     written.  Validity, RT_E_NOMEM (the handle is left as it was) and every refusal: rt_fetch_record_band's, under this
 *     entry's name.
 *   - the INSIDE frames of record (start, end) are rt_fetch_record_estimates': start * N <= position and position + N <= end * N.
 *     They are numbered i = 0, 1, ...: part 0's run first, then part 1's.  n_inside counts them.
 *   - per column j and inside frame, p = re * re + im * im in float64, every product and sum rounded once (no contraction).
 *     mean[j]: the project's canonical order, the one the record cells' statistics use -- 64 partials, inside frame i adds into
 *     partial i mod 64 in increasing i, the partials are folded by halving (each takes its neighbour at distance 32, 16, ... 1),
 *     and the sum is divided by n_inside.  peak[j]: the largest p over the inside frames; a NaN propagates (numpy.max).
 *     n_inside == 0: every mean, peak and scalar of the row is NaN, peak_col is -1.
 *   - the scalars are computed from the row's means m_0 ... m_2w in float64, left to right:
 *       total        = ((m_0 + m_1) + ...)
 *       centre_share = m_w / total
 *       centroid     = (sum m_j d_j) / total                             bins off the record's bin
 *       width        = sqrt((sum m_j ((d_j - centroid) (d_j - centroid))) / total)
 *       peak_col     = the lowest j with m_j equal to the row's maximum
 *       peak_bins    = d_p + 0.5 (a - c) / ((a - 2 b) + c),  a, b, c = log m_(p-1), log m_p, log m_(p+1),  p = peak_col,
 *                      where 0 < p < 2 w and the three means are finite and > 0; NaN elsewhere (w == 0, a peak on the band's edge)
 *     If any m_j is NaN, peak_col is -1 and every scalar is NaN.  A record of constant frames has total == 0, and the divisions
 *     give NaN as IEEE gives them.  Times sample_rate / N, centroid, width and peak_bins are Hz.
 *   - the same frames give the same bytes: on every handle kind (mode, lanes, chained, masked, float64 dense / map-free /
 *     rescue), on every fetch and in any order of calls with the other record entries.  A NaN mean or peak is the one quiet NaN.
 *   - lazy: rt_process*, rt_fetch and every other fetch entry allocate, copy and launch what they do without this entry.  The
 *     entry's first call for a delivered call and (k, w) makes sure the band pool holds (k, w) (as rt_fetch_record_band would,
 *     without the copy to the host), uploads a plan of 28 bytes a record, runs one kernel on the gather's stream, waits, and
 *     copies rows, means and peaks down from a pool of its own per call slot.  The same (k, w) again copies only; another pair
 *     builds again.  A later rt_fetch_record_band(k, w) copies without rebuilding.
 */
typedef struct rt_record_spectrum {
    double total;          /* sum of the column means                                         */
    double centre_share;   /* mean[w] / total                                                 */
    double centroid;       /* bins off the record's bin                                       */
    double width;          /* RMS width in bins about the centroid                            */
    double peak_bins;      /* log-parabolic peak position, bins off the record's bin          */
    int32_t peak_col;      /* lowest column whose mean is the largest; -1: a NaN mean         */
    int32_t n_inside;      /* frames wholly inside the record's own cells                     */
} rt_record_spectrum;      /* 48 bytes */

int rt_fetch_record_spectrum(rt_handle *h, int32_t hop_div, int32_t half_width, rt_record_spectrum *rows, double *mean, double *peak,
                             size_t cap, size_t *n_out);

/*
 * ---- input statistics: level, DC and clipping of every stream's raw input (additive within ABI version 6) ----
 * Everything above describes a buffer's spectrum; this describes the buffer.  A radio at fixed gain clips, a dead one delivers
 * constant bytes instead of no callbacks, and a record only exists where the detection worked -- so the caller wants, per stream
 * and call: how many components sat at full scale, the level, the DC, whether the samples still move.  With the feature on every
 * rt_process* reads its input once more on the device (one streaming kernel and a fold, on the scan's stream, in front of the
 * scan) and leaves one 64-byte row per stream in pinned host memory; rt_fetch_input_stats copies the rows.
 *   - a RAW COMPONENT is, per input format: uint8 2 b - 255 (an odd integer; (2 b - 255) / 255 is exactly b / 127.5 - 1); int8 and
 *     int16 the integer itself; complex64 / complex128 the value.  value = raw / unit.
 *   - integer formats: the three sums are exact integers of 64 bits, converted to double once, so every field is
 *     (double)(the exact sum) at any buffer length; peak is exact.
 *   - float formats: every sum is formed in float64 over the FINITE components alone, in an order that depends on the sample index
 *     and nothing else -- not on the pointer's alignment, the stride, the lanes, the _host entries -- so the same samples give
 *     the same bytes in all of them, and from run to run.  A NaN or an infinite component is counted in n_nonfinite and takes part
 *     in nothing else.
 *   - rt_set_input_stats(h, on): on != 0 turns the feature on, 0 off.  RT_E_INVALID ("pending") while unfetched calls are pending,
 *     as rt_set_record_iq.  Every handle kind: float32 in every mode, nperseg and lane count, chained (every link is a stream),
 *     float64 dense and with RT_FLAG_F64_SPARSE / RT_FLAG_F64_RESCUE.  The first call that turns it on allocates the partial rows
 *     and the pinned rows of the two call slots (RT_E_NOMEM); a handle on which it was never on allocates, copies and launches
 *     exactly what it did without this entry.
 *   - rt_fetch_input_stats(h, out, n): `out` HOST memory, n == n_streams rows, of the call the last rt_fetch / rt_fetch_f64
 *     delivered (RT_OK or RT_E_CAPACITY).  Valid until the next rt_process*, rt_extract*, rt_reset or rt_set_input_stats on the
 *     handle; with two calls in flight: process k, process k + 1, fetch k, stats k.  RT_E_INVALID: a null handle or `out`, a wrong
 *     n, the feature off, no delivered call, a delivered call enqueued before the feature was on, a delivered rt_extract*.  A
 *     laned handle gathers its lanes' rows in stream order.
 *   - a stream absent from the call (rt_set_present) has n_samples 0, zero counts and sums, peak 0; format and unit are set.
 *   - the rows are computed once, at enqueue, from ALL n_samples (the remainder past the last whole segment included; a call of
 *     fewer than nperseg samples has rows too).  What rt_fetch analyses again -- AUTO's level-ups, the partial dense re-run, pool
 *     and capacity growth, the detrend guard, the float64 rescue -- does not recompute them; a failed rt_process* leaves none.
 *     The analysis itself is the same bytes with the feature on or off.
 */
typedef struct rt_input_stats {
    int64_t n_samples;     /* samples of this stream the call covered; 0 for a stream absent from the call                       */
    int64_t n_rail;        /* components (I and Q counted separately) at full scale: uint8 0 or 255; int8 -128 or 127; int16
                              -32768 or 32767; complex64 / complex128: finite with |c| >= 1.0                                     */
    int64_t n_nonfinite;   /* NaN or +-Inf components (0 for the integer formats)                                                */
    double sum_i, sum_q;   /* sums of the raw components                                                                          */
    double sum_sq;         /* sum of I * I + Q * Q, raw                                                                           */
    double peak;           /* max |raw component|, 0 if there is none                                                             */
    int32_t format;        /* the call's input format: 0 complex, 1 uint8, 2 int16, 3 int8                                        */
    int32_t unit;          /* raw full scale: uint8 255, int8 128, int16 32768, complex 1                                         */
} rt_input_stats;          /* 64 bytes */

int rt_set_input_stats(rt_handle *h, int32_t on);
int rt_fetch_input_stats(rt_handle *h, rt_input_stats *out, size_t n);

/* Plain device-memory helpers so that a host without its own HIP binding
 * (ctypes-only integration) can stage IQ: thin hipMalloc/hipFree/hipMemcpy. */
int rt_dev_alloc(int32_t device, size_t bytes, void **out);
int rt_dev_free(int32_t device, void *ptr);
int rt_dev_upload(int32_t device, void *dst_dev, const void *src_host, size_t bytes);
int rt_dev_download(int32_t device, void *dst_host, const void *src_dev, size_t bytes);
int rt_device_count(int *count);

#ifdef __cplusplus
}
#endif
#endif /* RT_ANALYZE_H */
