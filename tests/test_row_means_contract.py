"""Every bin's noise level (RT_FLAG_ROW_MEANS, rt_fetch_row_means[_f64]) without a GPU: the flag and the two entry points are
declared and exported, a null handle is refused, and a flagged handle fails loudly where no device is present."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from pyradiotracking_amd import _native, build
from pyradiotracking_amd.analyze import BatchSignalAnalyzer, SignalAnalyzer

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _native.load_library()


def _no_gpu(lib):
    n = C.c_int(0)
    lib.rt_device_count(C.byref(n))
    if n.value > 0:
        pytest.skip("a GPU is present")


def test_flag_value_in_header_and_binding():
    text = open(os.path.join(REPO, "include", "rt_analyze.h")).read()
    m = re.search(r"#define\s+RT_FLAG_ROW_MEANS\s+(\d+)u", text)
    assert m and int(m.group(1)) == 16
    assert _native.RT_FLAG_ROW_MEANS == 16
    # a bit of its own: none of the other flags
    assert _native.RT_FLAG_ROW_MEANS & (_native.RT_FLAG_TIMING | _native.RT_FLAG_NO_LIN_DETREND | _native.RT_FLAG_GROUP_DETECT
                                        | _native.RT_FLAG_NO_GROUP_DETECT) == 0


def test_symbols_exported_and_null_handle_refused(lib):
    raw = C.CDLL(_native.LIB_PATH)
    for name in ("rt_fetch_row_means", "rt_fetch_row_means_f64"):
        assert name in _native.ABI_SYMBOLS
        assert hasattr(raw, name), name
    out32 = np.zeros(16, dtype=np.float32)
    out64 = np.zeros(16, dtype=np.float64)
    assert lib.rt_fetch_row_means(None, out32.ctypes.data, out32.size) == _native.RT_E_INVALID
    assert lib.rt_fetch_row_means_f64(None, out64.ctypes.data, out64.size) == _native.RT_E_INVALID
    assert lib.rt_fetch_row_means(None, None, 0) == _native.RT_E_INVALID
    assert lib.rt_fetch_row_means_f64(None, None, 0) == _native.RT_E_INVALID


def _cfg(nperseg=256, lanes=1):
    cfg = _native.RtConfig()
    cfg.n_streams, cfg.nperseg, cfg.mode, cfg.max_samples, cfg.sample_rate = 4, nperseg, _native.RT_MODE_AUTO, 1 << 16, 300000.0
    cfg.min_duration_s, cfg.max_duration_s, cfg.lanes = 0.008, 0.04, lanes
    cfg.scale, cfg.threshold, cfg.snr_threshold = 1.0, 1e-9, 3.0
    cfg.flags = _native.RT_FLAG_ROW_MEANS
    return cfg


def test_create_with_flag_without_gpu_fails_loudly(lib):
    _no_gpu(lib)
    for nperseg, lanes in ((256, 1), (300, 1), (8192, 1), (256, 2)):
        cfg = _cfg(nperseg, lanes)
        w = np.hamming(nperseg).astype(np.float32)
        cfg.window = w.ctypes.data_as(C.POINTER(C.c_float))
        h = C.c_void_p()
        assert lib.rt_create(C.byref(cfg), C.byref(h)) == _native.RT_E_NO_DEVICE, (nperseg, lanes)
    for nperseg in (256, 300):
        cfg = _cfg(nperseg)
        w64 = np.hamming(nperseg)
        c64 = _native.RtConfigF64()
        c64.window = w64.ctypes.data_as(C.POINTER(C.c_double))
        c64.scale, c64.threshold, c64.snr_threshold = 1.0, 1e-9, 3.0
        h = C.c_void_p()
        assert lib.rt_create_f64(C.byref(cfg), C.byref(c64), C.byref(h)) == _native.RT_E_NO_DEVICE, nperseg
    for precision in ("float32", "float64"):
        with pytest.raises(_native.NativeError) as ei:
            BatchSignalAnalyzer(["0", "1"], row_means=True, precision=precision, sdr_callback_length=4096)
        assert ei.value.code == _native.RT_E_NO_DEVICE
    with pytest.raises(_native.NativeError) as ei:
        SignalAnalyzer("0", row_means=True, sdr_callback_length=4096)
    assert ei.value.code == _native.RT_E_NO_DEVICE
