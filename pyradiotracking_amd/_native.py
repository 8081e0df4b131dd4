"""ctypes binding of the C-ABI in include/rt_analyze.h (librt_analyze.so).

The library is the product: if it cannot be loaded, or no GPU is usable, every
entry point here raises -- there is no CPU fallback.
"""
from __future__ import annotations

import collections
import ctypes as C
import os
from typing import Optional

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "librt_analyze.so")

RT_OK = 0
RT_E_INVALID = -1
RT_E_UNSUPPORTED = -2
RT_E_NO_DEVICE = -3
RT_E_HIP = -4
RT_E_CAPACITY = -5
RT_E_ONE_SEGMENT = -6
RT_E_NOMEM = -7
RT_E_HOT_OVERFLOW = -8  # RT_MODE_SPARSE: a candidate list overflowed, the call has no result and is consumed

RT_MODE_AUTO, RT_MODE_DENSE, RT_MODE_SPARSE, RT_MODE_PREFILTER, RT_MODE_RUNFILTER = 0, 1, 2, 3, 4
RT_FLAG_TIMING = 1
RT_FLAG_NO_LIN_DETREND = 2  # subtract the segment mean before windowing even for hamming / hann / boxcar windows
RT_FLAG_GROUP_DETECT = 4  # sparse detection by groups of candidate lists at any number of streams (default: from 1 024 streams per handle)
RT_FLAG_NO_GROUP_DETECT = 8  # ... never
RT_FLAG_ROW_MEANS = 16  # keep each call's row means (every bin's noise level) for rt_fetch_row_means[_f64]
RT_FLAG_RECORD_CELLS = 32  # keep the spectrogram cells of every record of a call (the reference's ``data``) for rt_fetch_record_cells[_f64]
RT_FLAG_F64_RESCUE = 128  # rt_create_f64 with RT_FLAG_F64_SPARSE only: overflowing streams are analysed again on their own inside rt_fetch_f64
RT_FLAG_F64_SPARSE = 64  # rt_create_f64 only: the map-free float64 path (fused scan + detection from candidate-cell lists)

SUPPORTED_NPERSEG = tuple(range(8, 8193)) + (16384,)  # 8 .. 8192 and 16384 (32 .. 4096 powers of two: the fused scans; everything else: general transforms, dense path)
FUSED_NPERSEG = (256, 512, 1024, 2048, 4096)


class RtConfig(C.Structure):
    _fields_ = [
        ("device", C.c_int32),
        ("n_streams", C.c_int32),
        ("nperseg", C.c_int32),
        ("mode", C.c_int32),
        ("max_samples", C.c_int64),
        ("sample_rate", C.c_double),
        ("window", C.POINTER(C.c_float)),
        ("scale", C.c_float),
        ("threshold", C.c_float),
        ("snr_threshold", C.c_float),
        ("calibration_db", C.c_float),
        ("min_duration_s", C.c_double),
        ("max_duration_s", C.c_double),
        ("hot_capacity", C.c_int32),
        ("record_capacity", C.c_int32),
        ("segs_per_chunk", C.c_int32),
        ("flags", C.c_int32),
        ("hip_stream", C.c_void_p),
        ("lanes", C.c_int32),
        ("record_pool", C.c_int32),
    ]


class RtCallInfo(C.Structure):
    _fields_ = [
        ("n_seg", C.c_int32),
        ("mode_used", C.c_int32),
        ("fell_back", C.c_int32),
        ("n_dense_streams", C.c_int32),
        ("n_hot", C.c_int64),
        ("n_records", C.c_int64),
        ("ms_stft", C.c_float),
        ("ms_detect", C.c_float),
        ("ms_total", C.c_float),
        ("segs_per_chunk", C.c_int32),
    ]


#: numpy view of ``rt_record`` (40 bytes)
RECORD_DTYPE = np.dtype(
    [
        ("stream", "<i4"),
        ("fi", "<i4"),
        ("start", "<i4"),
        ("end", "<i4"),
        ("max_p", "<f4"),
        ("mean_p", "<f4"),
        ("std_db", "<f4"),
        ("row_mean", "<f4"),
        ("shadowed", "<i4"),
        ("reserved", "<i4"),
    ]
)

#: numpy view of ``rt_record_estimate`` (72 bytes): a row of ``rt_fetch_record_estimates``
ESTIMATE_DTYPE = np.dtype(
    [
        ("r_re", "<f8"),
        ("r_im", "<f8"),
        ("pair_mag", "<f8"),
        ("offset_bins", "<f8"),
        ("coherence", "<f8"),
        ("level", "<f8"),
        ("rise", "<f8"),
        ("fall", "<f8"),
        ("n_pairs", "<i4"),
        ("n_inside", "<i4"),
    ]
)
assert ESTIMATE_DTYPE.itemsize == 72

#: numpy view of ``rt_record_spectrum`` (48 bytes): a row of ``rt_fetch_record_spectrum``
SPECTRUM_DTYPE = np.dtype(
    [
        ("total", "<f8"),
        ("centre_share", "<f8"),
        ("centroid", "<f8"),
        ("width", "<f8"),
        ("peak_bins", "<f8"),
        ("peak_col", "<i4"),
        ("n_inside", "<i4"),
    ]
)
assert SPECTRUM_DTYPE.itemsize == 48

#: numpy view of ``rt_input_stats`` (64 bytes): a row of ``rt_fetch_input_stats``
INPUT_STATS_DTYPE = np.dtype(
    [
        ("n_samples", "<i8"),
        ("n_rail", "<i8"),
        ("n_nonfinite", "<i8"),
        ("sum_i", "<f8"),
        ("sum_q", "<f8"),
        ("sum_sq", "<f8"),
        ("peak", "<f8"),
        ("format", "<i4"),
        ("unit", "<i4"),
    ]
)
assert INPUT_STATS_DTYPE.itemsize == 64


class RtConfigF64(C.Structure):
    """``rt_config_f64``: the float64 window / scale / thresholds / calibration of a float64 handle (``rt_create_f64``)."""

    _fields_ = [
        ("window", C.POINTER(C.c_double)),
        ("scale", C.c_double),
        ("threshold", C.c_double),
        ("snr_threshold", C.c_double),
        ("calibration_db", C.c_double),
    ]


#: numpy view of ``rt_record_f64`` (56 bytes): a float64 handle's records
RECORD_F64_DTYPE = np.dtype(
    [
        ("stream", "<i4"),
        ("fi", "<i4"),
        ("start", "<i4"),
        ("end", "<i4"),
        ("max_p", "<f8"),
        ("mean_p", "<f8"),
        ("std_db", "<f8"),
        ("row_mean", "<f8"),
        ("shadowed", "<i4"),
        ("reserved", "<i4"),
    ]
)

#: nperseg a float64 handle takes: 8 .. 4096 and the powers of two up to 8192
SUPPORTED_NPERSEG_F64 = tuple(range(8, 4097)) + (8192,)

#: every symbol include/rt_analyze.h declares
ABI_SYMBOLS = (
    "rt_abi_version",
    "rt_create",
    "rt_destroy",
    "rt_reset",
    "rt_reset_stream",
    "rt_set_stream_params",
    "rt_process",
    "rt_process_u8",
    "rt_process_host",
    "rt_process_u8_host",
    "rt_process_i16",
    "rt_process_i16_host",
    "rt_process_i8",
    "rt_process_i8_host",
    "rt_fetch",
    "rt_extract",
    "rt_spectrogram",
    "rt_calibrate_read",
    "rt_get_call_info",
    "rt_last_error",
    "rt_dev_alloc",
    "rt_dev_free",
    "rt_dev_upload",
    "rt_dev_download",
    "rt_device_count",
    "rt_create_f64",
    "rt_fetch_f64",
    "rt_set_stream_params_f64",
    "rt_extract_f64",
    "rt_spectrogram_f64",
    "rt_fetch_row_means",
    "rt_fetch_row_means_f64",
    "rt_fetch_record_cells",
    "rt_fetch_record_cells_f64",
    "rt_set_stream_settings",
    "rt_set_stream_settings_f64",
    "rt_set_present",
    "rt_set_chain",
    "rt_set_record_iq",
    "rt_fetch_record_iq",
    "rt_fetch_record_stft",
    "rt_fetch_record_stft_f64",
    "rt_fetch_record_stft_hop",
    "rt_fetch_record_stft_hop_f64",
    "rt_fetch_record_estimates",
    "rt_fetch_record_band",
    "rt_fetch_record_band_f64",
    "rt_fetch_record_spectrum",
    "rt_set_input_stats",
    "rt_fetch_input_stats",
)

_lib = None


class NativeError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"rt_analyze error {code}: {message}")
        self.code = code


def load_library(path: Optional[str] = None):
    """dlopen librt_analyze.so (built in-tree by pyradiotracking_amd.build).

    If torch is importable it is imported first, so both share one HIP
    runtime (torch ships its own libamdhip64 with the same soname)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("RT_ANALYZE_LIB") or LIB_PATH  # env override: A/B builds of the kernels
    if not os.path.exists(p):
        raise ImportError(
            f"{p} is missing: build it with `python -m pyradiotracking_amd.build` "
            "(hipcc --offload-arch=gfx950); this package has no CPU fallback"
        )
    if not os.environ.get("RT_NO_TORCH"):
        try:
            import torch  # noqa: F401
        except Exception:  # pragma: no cover - torch is optional for the product
            pass
    lib = C.CDLL(p, mode=getattr(os, "RTLD_NOW", 2) | getattr(os, "RTLD_GLOBAL", 0x100))
    vp = C.c_void_p
    lib.rt_abi_version.restype = C.c_int
    lib.rt_create.argtypes = [C.POINTER(RtConfig), C.POINTER(vp)]
    lib.rt_destroy.argtypes = [vp]
    lib.rt_destroy.restype = None
    lib.rt_reset.argtypes = [vp]
    lib.rt_reset_stream.argtypes = [vp, C.c_int32]
    lib.rt_set_stream_params.argtypes = [vp, vp, vp]
    lib.rt_process.argtypes = [vp, vp, C.c_int64, C.c_int64]
    lib.rt_process_u8.argtypes = [vp, vp, C.c_int64, C.c_int64]
    lib.rt_process_host.argtypes = [vp, vp, C.c_int64, C.c_int64]
    lib.rt_process_u8_host.argtypes = [vp, vp, C.c_int64, C.c_int64]
    lib.rt_process_i16.argtypes = [vp, vp, C.c_int64, C.c_int64]
    lib.rt_process_i16_host.argtypes = [vp, vp, C.c_int64, C.c_int64]
    lib.rt_process_i8.argtypes = [vp, vp, C.c_int64, C.c_int64]
    lib.rt_process_i8_host.argtypes = [vp, vp, C.c_int64, C.c_int64]
    lib.rt_fetch.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.rt_extract.argtypes = [vp, vp, C.c_int32, C.c_int32, vp, C.c_int32]
    lib.rt_spectrogram.argtypes = [vp, vp, C.c_int64, C.c_int64, vp]
    lib.rt_calibrate_read.argtypes = [vp, vp, C.c_int64, C.c_int64]
    lib.rt_get_call_info.argtypes = [vp, C.POINTER(RtCallInfo)]
    lib.rt_last_error.argtypes = [vp]
    lib.rt_last_error.restype = C.c_char_p
    lib.rt_dev_alloc.argtypes = [C.c_int32, C.c_size_t, C.POINTER(vp)]
    lib.rt_dev_free.argtypes = [C.c_int32, vp]
    lib.rt_dev_upload.argtypes = [C.c_int32, vp, vp, C.c_size_t]
    lib.rt_dev_download.argtypes = [C.c_int32, vp, vp, C.c_size_t]
    lib.rt_device_count.argtypes = [C.POINTER(C.c_int)]
    lib.rt_create_f64.argtypes = [C.POINTER(RtConfig), C.POINTER(RtConfigF64), C.POINTER(vp)]
    lib.rt_fetch_f64.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.rt_set_stream_params_f64.argtypes = [vp, vp, vp]
    lib.rt_extract_f64.argtypes = [vp, vp, C.c_int32, C.c_int32, vp, C.c_int32]
    lib.rt_spectrogram_f64.argtypes = [vp, vp, C.c_int64, C.c_int64, vp]
    lib.rt_fetch_row_means.argtypes = [vp, vp, C.c_size_t]
    lib.rt_fetch_row_means_f64.argtypes = [vp, vp, C.c_size_t]
    lib.rt_fetch_record_cells.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, vp]
    lib.rt_fetch_record_cells_f64.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, vp]
    lib.rt_set_stream_settings.argtypes = [vp, vp, vp, vp]
    lib.rt_set_stream_settings_f64.argtypes = [vp, vp, vp, vp]
    lib.rt_set_present.argtypes = [vp, vp]
    lib.rt_set_chain.argtypes = [vp, C.c_int32]
    lib.rt_set_record_iq.argtypes = [vp, C.c_int32]
    lib.rt_fetch_record_iq.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int32)]
    for fn in (lib.rt_fetch_record_stft, lib.rt_fetch_record_stft_f64):
        fn.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    for fn in (lib.rt_fetch_record_stft_hop, lib.rt_fetch_record_stft_hop_f64):
        fn.argtypes = [vp, C.c_int32, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.rt_fetch_record_estimates.argtypes = [vp, C.c_int32, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    for fn in (lib.rt_fetch_record_band, lib.rt_fetch_record_band_f64):
        fn.argtypes = [vp, C.c_int32, C.c_int32, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.rt_fetch_record_spectrum.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.rt_set_input_stats.argtypes = [vp, C.c_int32]
    lib.rt_fetch_input_stats.argtypes = [vp, vp, C.c_size_t]
    for name in ABI_SYMBOLS:
        getattr(lib, name)  # AttributeError if the build lost a symbol
    if path is None:
        _lib = lib
    return lib


def device_count() -> int:
    lib = load_library()
    n = C.c_int(0)
    lib.rt_device_count(C.byref(n))
    return n.value


def _raise(lib, handle, code):
    msg = lib.rt_last_error(handle)
    text = msg.decode("utf-8", "replace") if msg else ""
    if code == RT_E_ONE_SEGMENT:
        # the reference indexes times[1] and raises IndexError (analyze.py:354)
        raise IndexError("index 1 is out of bounds for axis 0 with size 1")
    raise NativeError(code, text)


class DeviceBuffer:
    """A raw hipMalloc allocation owned through the C-ABI (torch-free staging)."""

    def __init__(self, device: int, nbytes: int):
        self._lib = load_library()
        self.device = device
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        rc = self._lib.rt_dev_alloc(device, self.nbytes, C.byref(p))
        if rc != RT_OK:
            _raise(self._lib, None, rc)
        self.ptr = p.value

    def upload(self, arr: np.ndarray):
        a = np.ascontiguousarray(arr)
        assert a.nbytes <= self.nbytes
        rc = self._lib.rt_dev_upload(self.device, self.ptr, a.ctypes.data, a.nbytes)
        if rc != RT_OK:
            _raise(self._lib, None, rc)

    def download(self, dtype, count: int) -> np.ndarray:
        out = np.empty(count, dtype=dtype)
        assert out.nbytes <= self.nbytes
        rc = self._lib.rt_dev_download(self.device, out.ctypes.data, self.ptr, out.nbytes)
        if rc != RT_OK:
            _raise(self._lib, None, rc)
        return out

    def free(self):
        if self.ptr:
            self._lib.rt_dev_free(self.device, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class NativeAnalyzer:
    """Owns one ``rt_handle``."""

    def __init__(
        self,
        *,
        n_streams: int,
        nperseg: int,
        max_samples: int,
        sample_rate: float,
        window_f32: np.ndarray,
        scale: float,
        threshold: float,
        snr_threshold: float,
        calibration_db: float,
        min_duration_s: float,
        max_duration_s: float,
        device: int = 0,
        mode: int = RT_MODE_AUTO,
        hot_capacity: int = 0,
        record_capacity: int = 0,
        segs_per_chunk: int = 0,
        timing: bool = False,
        hip_stream: Optional[int] = None,
        lanes: int = 1,
        subtract_first: bool = False,
        record_pool: int = 0,
        group_detect: Optional[bool] = None,
        precision: str = "float32",
        row_means: bool = False,
        record_cells: bool = False,
        f64_sparse: bool = False,
        f64_rescue: bool = False,
    ):
        """``precision="float64"``: a float64 handle (``rt_create_f64``) -- ``window_f32`` then holds the float64 window and
        ``scale`` / ``threshold`` / ``snr_threshold`` / ``calibration_db`` are passed on as float64, never rounded to float32;
        the analysis takes complex128 (or uint8) IQ and the records are ``RECORD_F64_DTYPE``.  ``row_means``:
        ``RT_FLAG_ROW_MEANS`` (``fetch_row_means``); ``record_cells``: ``RT_FLAG_RECORD_CELLS`` (``fetch_record_cells``).
        ``f64_sparse``: ``RT_FLAG_F64_SPARSE`` -- a float64 handle without the float64 map (``mode`` must be ``RT_MODE_AUTO``;
        ``hot_capacity`` then counts candidate cells per stream and call, 0 or 1024 ... 8192).
        ``f64_rescue``: ``RT_FLAG_F64_RESCUE`` (needs ``f64_sparse``) -- a stream that emits more than ``hot_capacity`` cells no
        longer ends the call with ``RT_E_HOT_OVERFLOW``: the fetch analyses it again on its own from a per-stream float64 map
        (``call_info``: ``n_dense_streams``, ``fell_back``)."""
        if precision not in ("float32", "float64"):
            raise ValueError(f"precision must be 'float32' or 'float64', not {precision!r}")
        if f64_sparse:
            if precision != "float64":
                raise ValueError("f64_sparse needs precision='float64'")
            if mode != RT_MODE_AUTO:
                raise ValueError("f64_sparse selects the path by itself: mode must be 'auto'")
            if record_cells:
                raise ValueError("f64_sparse keeps no map: record_cells is not available with it")
        if f64_rescue and not f64_sparse:
            raise ValueError("f64_rescue re-runs the overflowing streams of the map-free path: it needs f64_sparse=True")
        self.f64 = precision == "float64"
        self._lib = load_library()
        self._handle = C.c_void_p()
        w = np.ascontiguousarray(window_f32, dtype=np.float64 if self.f64 else np.float32)
        if w.shape != (nperseg,):
            raise ValueError("window must have nperseg coefficients")
        cfg = RtConfig()
        cfg.device = device
        cfg.n_streams = n_streams
        cfg.nperseg = nperseg
        cfg.mode = mode
        cfg.max_samples = max_samples
        cfg.sample_rate = float(sample_rate)
        cfg.window = w.ctypes.data_as(C.POINTER(C.c_float)) if not self.f64 else None
        cfg.scale = float(scale)
        cfg.threshold = float(threshold)
        cfg.snr_threshold = float(snr_threshold)
        cfg.calibration_db = float(calibration_db)
        cfg.min_duration_s = float(min_duration_s)
        cfg.max_duration_s = float(max_duration_s)
        cfg.hot_capacity = hot_capacity
        cfg.record_capacity = record_capacity
        cfg.segs_per_chunk = segs_per_chunk
        cfg.flags = ((RT_FLAG_TIMING if timing else 0) | (RT_FLAG_NO_LIN_DETREND if subtract_first else 0)
                     | (0 if group_detect is None else RT_FLAG_GROUP_DETECT if group_detect else RT_FLAG_NO_GROUP_DETECT)
                     | (RT_FLAG_ROW_MEANS if row_means else 0)
                     | (RT_FLAG_RECORD_CELLS if record_cells else 0)
                     | (RT_FLAG_F64_SPARSE if f64_sparse else 0)
                     | (RT_FLAG_F64_RESCUE if f64_rescue else 0))
        cfg.hip_stream = hip_stream
        cfg.lanes = int(lanes)
        cfg.record_pool = int(record_pool)
        if self.f64:
            c64 = RtConfigF64()
            c64.window = w.ctypes.data_as(C.POINTER(C.c_double))
            c64.scale = float(scale)
            c64.threshold = float(threshold)
            c64.snr_threshold = float(snr_threshold)
            c64.calibration_db = float(calibration_db)
            rc = self._lib.rt_create_f64(C.byref(cfg), C.byref(c64), C.byref(self._handle))
        else:
            rc = self._lib.rt_create(C.byref(cfg), C.byref(self._handle))
        if rc != RT_OK:
            self._handle = C.c_void_p()
            _raise(self._lib, None, rc)
        self.n_streams = n_streams
        self.nperseg = nperseg
        self.device = device
        self.max_samples = max_samples
        self._fed = collections.deque(maxlen=2)  # the formats of the calls in flight (a third enqueue drops the oldest, as the handle does)
        self.fetched_format = None               # ... and of the call ``fetch`` consumed last: "c", "u8", "i16", "i8" or "extract"

    # -- lifecycle --------------------------------------------------------
    def close(self):
        if getattr(self, "_handle", None) and self._handle.value:
            self._lib.rt_destroy(self._handle)
            self._handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != RT_OK:
            _raise(self._lib, self._handle, rc)

    def reset(self):
        self._check(self._lib.rt_reset(self._handle))

    def reset_stream(self, stream: int):
        self._check(self._lib.rt_reset_stream(self._handle, int(stream)))

    def set_stream_params(self, threshold: Optional[np.ndarray], calibration_db: Optional[np.ndarray]):
        """Per-stream linear thresholds / calibration (float32 ``[S]`` each -- float64 on a float64 handle --, or None = the
        handle's value)."""
        dt = np.float64 if self.f64 else np.float32

        def arr(a):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dt)
            if a.shape != (self.n_streams,):
                raise ValueError(f"expected {self.n_streams} values")
            return a

        t, c = arr(threshold), arr(calibration_db)
        fn = self._lib.rt_set_stream_params_f64 if self.f64 else self._lib.rt_set_stream_params
        self._check(
            fn(
                self._handle, t.ctypes.data if t is not None else None, c.ctypes.data if c is not None else None
            )
        )

    def set_stream_settings(self, snr_threshold: Optional[np.ndarray], min_duration_s: Optional[np.ndarray],
                            max_duration_s: Optional[np.ndarray]):
        """``rt_set_stream_settings`` (``rt_set_stream_settings_f64`` on a float64 handle): per-stream linear SNR thresholds
        (float32 ``[S]``, float64 on a float64 handle) and duration gates in seconds (float64 ``[S]``), each or None = the
        handle's value.  The durations must lie inside the handle's ``min_duration_s`` / ``max_duration_s``."""

        def arr(a, dt):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dt)
            if a.shape != (self.n_streams,):
                raise ValueError(f"expected {self.n_streams} values")
            return a

        s = arr(snr_threshold, np.float64 if self.f64 else np.float32)
        lo, hi = arr(min_duration_s, np.float64), arr(max_duration_s, np.float64)
        fn = self._lib.rt_set_stream_settings_f64 if self.f64 else self._lib.rt_set_stream_settings
        self._check(fn(self._handle, *(a.ctypes.data if a is not None else None for a in (s, lo, hi))))

    def set_present(self, present: Optional[np.ndarray]):
        """``rt_set_present``: one flag per stream (non-zero = the stream takes part in the calls enqueued from now on), or None =
        every stream.  A stream that sits a call out keeps its look-back, its pending reset and its previous segment count for
        its next present buffer; may be called with calls pending."""
        if present is None:
            self._check(self._lib.rt_set_present(self._handle, None))
            return
        m = np.ascontiguousarray(np.asarray(present).astype(bool), dtype=np.uint8)
        if m.shape != (self.n_streams,):
            raise ValueError(f"expected {self.n_streams} flags")
        self._check(self._lib.rt_set_present(self._handle, m.ctypes.data))

    def set_chain(self, links: int):
        """``rt_set_chain``: ``links >= 2`` groups the streams into runs of ``links`` consecutive indices whose present streams
        are, within one call, consecutive buffers of one recording (stream ``s`` looks back into its predecessor of the same
        call); 0 or 1 turns it off.  Refused with calls pending, on a float64 handle and on a handle with ``lanes > 1``."""
        self._check(self._lib.rt_set_chain(self._handle, int(links)))

    # -- analysis ---------------------------------------------------------
    def process_device(self, iq_ptr: int, n_samples: int, stream_stride: Optional[int] = None):
        self._check(self._lib.rt_process(self._handle, iq_ptr, n_samples, stream_stride or n_samples))
        self._fed.append("c")

    def process_device_u8(self, iq_ptr: int, n_samples: int, stream_stride: Optional[int] = None):
        self._check(self._lib.rt_process_u8(self._handle, iq_ptr, n_samples, stream_stride or n_samples))
        self._fed.append("u8")

    def process_device_i16(self, iq_ptr: int, n_samples: int, stream_stride: Optional[int] = None):
        self._check(self._lib.rt_process_i16(self._handle, iq_ptr, n_samples, stream_stride or n_samples))
        self._fed.append("i16")

    def process_device_i8(self, iq_ptr: int, n_samples: int, stream_stride: Optional[int] = None):
        self._check(self._lib.rt_process_i8(self._handle, iq_ptr, n_samples, stream_stride or n_samples))
        self._fed.append("i8")

    def process_host(self, iq: np.ndarray):
        """``[S, B]`` complex IQ in host memory: complex64 (complex128 on a float64 handle, where complex64 is widened exactly)."""
        a = np.ascontiguousarray(iq, dtype=np.complex128 if self.f64 else np.complex64)
        if a.ndim == 1:
            a = a[None, :]
        if a.shape[0] != self.n_streams:
            raise ValueError(f"expected {self.n_streams} streams, got {a.shape[0]}")
        self._keep = a  # async H2D copy reads it until the fetch
        self._check(self._lib.rt_process_host(self._handle, a.ctypes.data, a.shape[1], a.shape[1]))
        self._fed.append("c")

    def process_host_u8(self, raw: np.ndarray):
        """``[S, 2*B]`` uint8 (interleaved I, Q) in host memory; staged by the library (one buffer per call in flight)."""
        a = np.ascontiguousarray(raw, dtype=np.uint8)
        if a.ndim == 1:
            a = a[None, :]
        if a.shape[0] != self.n_streams or a.shape[1] % 2:
            raise ValueError(f"expected uint8 [{self.n_streams}, 2*B]")
        self._check(self._lib.rt_process_u8_host(self._handle, a.ctypes.data, a.shape[1] // 2, a.shape[1] // 2))
        self._fed.append("u8")

    def process_host_i16(self, raw: np.ndarray):
        """``[S, 2*B]`` int16 (interleaved I, Q) in host memory; staged by the library (one buffer per call in flight)."""
        a = np.asarray(raw)
        if a.dtype != np.int16:
            raise TypeError("expected int16 (interleaved I, Q)")
        a = np.ascontiguousarray(a)
        if a.ndim == 1:
            a = a[None, :]
        if a.ndim != 2 or a.shape[0] != self.n_streams or a.shape[1] % 2:
            raise ValueError(f"expected int16 [{self.n_streams}, 2*B]")
        self._check(self._lib.rt_process_i16_host(self._handle, a.ctypes.data, a.shape[1] // 2, a.shape[1] // 2))
        self._fed.append("i16")

    def process_host_i8(self, raw: np.ndarray):
        """``[S, 2*B]`` int8 (interleaved I, Q) in host memory; staged by the library (one buffer per call in flight)."""
        a = np.asarray(raw)
        if a.dtype != np.int8:
            raise TypeError("expected int8 (interleaved I, Q)")
        a = np.ascontiguousarray(a)
        if a.ndim == 1:
            a = a[None, :]
        if a.ndim != 2 or a.shape[0] != self.n_streams or a.shape[1] % 2:
            raise ValueError(f"expected int8 [{self.n_streams}, 2*B]")
        self._check(self._lib.rt_process_i8_host(self._handle, a.ctypes.data, a.shape[1] // 2, a.shape[1] // 2))
        self._fed.append("i8")

    def fetch(self, allow_truncated: bool = False) -> np.ndarray:
        """Records of the oldest enqueued call.  A call whose records were truncated (``RT_E_CAPACITY``: an ``rt_extract``
        call with more records in a stream than ``record_capacity``, or no memory to grow) raises unless ``allow_truncated`` -- then the truncated list is
        returned and ``last_truncated`` is set; either way it is consumed, so the next fetch belongs to the next
        call.  A call without any result (``RT_E_HOT_OVERFLOW``: sparse mode, candidate lists overflowed) always
        raises: an empty array would read as "no signals"."""
        n = C.c_size_t(0)
        self.last_truncated = False
        fetch = self._lib.rt_fetch_f64 if self.f64 else self._lib.rt_fetch
        self.fetched_format = self._fed.popleft() if self._fed else None  # (whatever follows consumes the call)
        rc = fetch(self._handle, None, 0, C.byref(n))  # size query: the call stays pending
        if rc != RT_OK and rc != RT_E_CAPACITY:
            self._check(rc)  # incl. RT_E_HOT_OVERFLOW: the library has dropped the call
        out = np.zeros(n.value, dtype=RECORD_F64_DTYPE if self.f64 else RECORD_DTYPE)
        if n.value:
            rc = fetch(self._handle, out.ctypes.data, n.value, C.byref(n))
        if rc == RT_E_CAPACITY:
            self.last_truncated = True
        if rc != RT_OK and not (allow_truncated and rc == RT_E_CAPACITY):
            self._check(rc)
        self._n_fetched = len(out)
        self._last_fetched = out  # (fetch_record_fine reads the records' start and end)
        return out

    def fetch_record_cells(self):
        """``rt_fetch_record_cells`` (``rt_fetch_record_cells_f64`` on a float64 handle): ``(offsets, cells)`` of the call
        ``fetch`` delivered last (in full) -- ``offsets`` int64 ``[n_records + 1]``, ``cells`` float32 (float64); the cells of
        record ``i``, the reference's ``data`` of that plateau (analyze.py:437-440), are ``cells[offsets[i]:offsets[i + 1]]``."""
        fn = self._lib.rt_fetch_record_cells_f64 if self.f64 else self._lib.rt_fetch_record_cells
        offsets = np.zeros(getattr(self, "_n_fetched", 0) + 1, dtype=np.int64)
        n = C.c_size_t(0)
        self._check(fn(self._handle, offsets.ctypes.data, offsets.size, None, 0, C.byref(n)))  # size query
        cells = np.empty(n.value, dtype=np.float64 if self.f64 else np.float32)
        if n.value:
            self._check(fn(self._handle, offsets.ctypes.data, offsets.size, cells.ctypes.data, cells.size, C.byref(n)))
        return offsets, cells

    def set_record_iq(self, margin_segments: int):
        """``rt_set_record_iq``: ``margin_segments >= 0`` makes the handle keep the sample tail of every stream's previous
        buffer, so that ``fetch_record_iq`` can hand out each record's samples with that many whole segments on either side;
        a negative value turns it off.  Refused with calls pending."""
        self._check(self._lib.rt_set_record_iq(self._handle, int(margin_segments)))

    def fetch_record_iq(self):
        """``rt_fetch_record_iq``: ``(offsets, first_segment, payload, bytes_per_sample)`` of the call ``fetch`` delivered last
        (in full) -- ``offsets`` int64 ``[n_records + 1]`` in samples, ``first_segment`` int32 ``[n_records]``, ``payload`` the
        caller's own bytes (uint8) of the whole segments ``first_segment[i] ... `` of record ``i``, back to back."""
        n_rec = getattr(self, "_n_fetched", 0)
        offsets = np.zeros(n_rec + 1, dtype=np.int64)
        first = np.zeros(n_rec, dtype=np.int32)
        n, bps = C.c_size_t(0), C.c_int32(0)
        fn = self._lib.rt_fetch_record_iq
        self._check(fn(self._handle, offsets.ctypes.data, offsets.size, first.ctypes.data, first.size, None, 0, C.byref(n), C.byref(bps)))
        payload = np.empty(n.value, dtype=np.uint8)
        if n.value:
            self._check(fn(self._handle, offsets.ctypes.data, offsets.size, first.ctypes.data, first.size, payload.ctypes.data,
                           payload.size, C.byref(n), C.byref(bps)))
        return offsets, first, payload, int(bps.value)

    def fetch_record_stft(self, hop_div: int = 1):
        """``rt_fetch_record_stft`` (``rt_fetch_record_stft_f64`` on a float64 handle): ``(offsets, first_segment, values)`` of
        the call ``fetch`` delivered last (in full) -- ``offsets`` int64 ``[n_records + 1]`` in segments, ``first_segment`` int32
        ``[n_records]``, ``values`` complex64 (complex128): the STFT value of record ``i``'s bin in each of the whole segments
        ``first_segment[i] ... `` that ``fetch_record_iq`` delivers for it.  ``hop_div`` k > 1: ``rt_fetch_record_stft_hop``
        (``_f64``), the values of the frames every ``nperseg / k`` samples, ``offsets`` in frames."""
        n_rec = getattr(self, "_n_fetched", 0)
        offsets = np.zeros(n_rec + 1, dtype=np.int64)
        first = np.zeros(n_rec, dtype=np.int32)
        n = C.c_size_t(0)
        if int(hop_div) != 1:
            hop = self._lib.rt_fetch_record_stft_hop_f64 if self.f64 else self._lib.rt_fetch_record_stft_hop

            def fn(*args):
                return hop(args[0], int(hop_div), *args[1:])
        else:
            fn = self._lib.rt_fetch_record_stft_f64 if self.f64 else self._lib.rt_fetch_record_stft
        self._check(fn(self._handle, offsets.ctypes.data, offsets.size, first.ctypes.data, first.size, None, 0, C.byref(n)))
        values = np.empty(n.value, dtype=np.complex128 if self.f64 else np.complex64)
        if n.value:
            self._check(fn(self._handle, offsets.ctypes.data, offsets.size, first.ctypes.data, first.size, values.ctypes.data, values.size, C.byref(n)))
        return offsets, first, values

    def fetch_record_estimates(self, hop_div: int = 4) -> np.ndarray:
        """``rt_fetch_record_estimates``: one ``ESTIMATE_DTYPE`` row per record of the call ``fetch`` delivered last (in full),
        reduced on the device from the frames every ``nperseg / hop_div`` samples; the frames are not copied."""
        n = C.c_size_t(0)
        self._check(self._lib.rt_fetch_record_estimates(self._handle, int(hop_div), None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=ESTIMATE_DTYPE)
        if n.value:
            self._check(self._lib.rt_fetch_record_estimates(self._handle, int(hop_div), out.ctypes.data, out.size, C.byref(n)))
        return out

    def fetch_record_band(self, hop_div: int = 1, half_width: int = 2):
        """``rt_fetch_record_band`` (``_f64`` on a float64 handle): ``(offsets, first_segment, values)`` of the call ``fetch``
        delivered last (in full) -- the frames of ``fetch_record_stft(hop_div)``, ``values`` complex64 (complex128)
        ``[n_frames, 2 * half_width + 1]``: column ``j`` is the bin ``(fi + j - half_width) mod nperseg``."""
        n_rec = getattr(self, "_n_fetched", 0)
        k, w = int(hop_div), int(half_width)
        offsets = np.zeros(n_rec + 1, dtype=np.int64)
        first = np.zeros(n_rec, dtype=np.int32)
        n = C.c_size_t(0)
        fn = self._lib.rt_fetch_record_band_f64 if self.f64 else self._lib.rt_fetch_record_band
        self._check(fn(self._handle, k, w, offsets.ctypes.data, offsets.size, first.ctypes.data, first.size, None, 0, C.byref(n)))
        values = np.empty((n.value, 2 * w + 1), dtype=np.complex128 if self.f64 else np.complex64)
        if n.value:
            self._check(fn(self._handle, k, w, offsets.ctypes.data, offsets.size, first.ctypes.data, first.size, values.ctypes.data, n.value, C.byref(n)))
        return offsets, first, values

    def fetch_record_spectrum(self, hop_div: int = 4, half_width: int = 2):
        """``rt_fetch_record_spectrum``: ``(rows, mean, peak)`` of the call ``fetch`` delivered last (in full) -- one
        ``SPECTRUM_DTYPE`` row per record and float64 ``[n_records, 2 * half_width + 1]`` arrays of each column's mean and largest
        ``|value| ** 2`` over the record's inside frames, reduced on the device from the frames of ``fetch_record_band``; the frames
        are not copied."""
        k, w = int(hop_div), int(half_width)
        n = C.c_size_t(0)
        fn = self._lib.rt_fetch_record_spectrum
        self._check(fn(self._handle, k, w, None, None, None, 0, C.byref(n)))
        cols = max(2 * w + 1, 0)
        rows = np.zeros(n.value, dtype=SPECTRUM_DTYPE)
        mean = np.zeros((n.value, cols), dtype=np.float64)
        peak = np.zeros((n.value, cols), dtype=np.float64)
        if n.value:
            self._check(fn(self._handle, k, w, rows.ctypes.data, mean.ctypes.data, peak.ctypes.data, rows.size, C.byref(n)))
        return rows, mean, peak

    def set_input_stats(self, on: bool):
        """``rt_set_input_stats``: every later ``rt_process*`` also leaves one ``INPUT_STATS_DTYPE`` row per stream, computed
        on the device from the raw input (``fetch_input_stats``); refused while calls are pending."""
        self._check(self._lib.rt_set_input_stats(self._handle, 1 if on else 0))

    def fetch_input_stats(self) -> np.ndarray:
        """``rt_fetch_input_stats``: ``[n_streams]`` ``INPUT_STATS_DTYPE`` rows of the call ``fetch`` delivered last."""
        out = np.zeros(self.n_streams, dtype=INPUT_STATS_DTYPE)
        self._check(self._lib.rt_fetch_input_stats(self._handle, out.ctypes.data, out.size))
        return out

    def fetch_row_means(self) -> np.ndarray:
        """``rt_fetch_row_means`` (``rt_fetch_row_means_f64`` on a float64 handle): ``[S, nperseg]`` float32 (float64), the
        mean of every bin's row over the segments of the call ``fetch`` delivered last, bins in fftfreq order."""
        out = np.empty((self.n_streams, self.nperseg), dtype=np.float64 if self.f64 else np.float32)
        fn = self._lib.rt_fetch_row_means_f64 if self.f64 else self._lib.rt_fetch_row_means
        self._check(fn(self._handle, out.ctypes.data, out.size))
        return out

    def extract_device(self, spec_ptr: int, n_seg: int, n_bins: int, last_ptr: Optional[int], n_seg_last: int):
        """``rt_extract`` (float32 maps), or ``rt_extract_f64`` (float64 maps) on a float64 handle."""
        fn = self._lib.rt_extract_f64 if self.f64 else self._lib.rt_extract
        self._check(fn(self._handle, spec_ptr, n_seg, n_bins, last_ptr, n_seg_last))
        self._fed.append("extract")

    def spectrogram_device(self, iq_ptr: int, n_samples: int, stream_stride: int, out_ptr: int):
        """``rt_spectrogram`` (complex64 -> float32), or ``rt_spectrogram_f64`` (complex128 -> float64) on a float64 handle."""
        fn = self._lib.rt_spectrogram_f64 if self.f64 else self._lib.rt_spectrogram
        self._check(fn(self._handle, iq_ptr, n_samples, stream_stride, out_ptr))

    def calibrate_read(self, iq_ptr: int, n_samples: int, stream_stride: int):
        self._check(self._lib.rt_calibrate_read(self._handle, iq_ptr, n_samples, stream_stride))

    def call_info(self) -> RtCallInfo:
        info = RtCallInfo()
        self._check(self._lib.rt_get_call_info(self._handle, C.byref(info)))
        return info
