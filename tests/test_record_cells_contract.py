"""The cells behind every record (RT_FLAG_RECORD_CELLS, rt_fetch_record_cells[_f64]) without a GPU: the flag and the two entry
points are declared and exported and refuse null handles; and the indexing convention -- ``rt::record_cell``, the function the
gather kernels run -- on the planted maps of ``tests/golden/extract_cases.npz`` with ``hc_extract``'s records: a gather of the
very map, whose canonical statistics are the records' own."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import analyze_oracle as oracle
from pyradiotracking_amd import _native, build
from pyradiotracking_amd.analyze import BatchSignalAnalyzer, SignalAnalyzer
from tests import golden_util as gu
from tests import record_cells_util as rcu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _native.load_library()


@pytest.fixture(scope="module")
def hc():
    lib = C.CDLL(build.build_hostcheck())
    vp = C.c_void_p
    lib.hc_extract.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_double,
                               C.c_float, C.c_float, C.c_float, C.c_double, C.c_double, vp, C.c_int]
    lib.hc_extract_f64.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_double,
                                   C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, vp, C.c_int]
    for fn in (lib.hc_record_cells, lib.hc_record_cells_f64):
        fn.argtypes = [vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, vp, C.c_longlong]
        fn.restype = C.c_longlong
    return lib


def test_flag_value_in_header_and_binding():
    text = open(os.path.join(REPO, "include", "rt_analyze.h")).read()
    m = re.search(r"#define\s+RT_FLAG_RECORD_CELLS\s+(\d+)u", text)
    assert m and int(m.group(1)) == 32
    assert _native.RT_FLAG_RECORD_CELLS == 32
    assert _native.RT_FLAG_RECORD_CELLS & (_native.RT_FLAG_TIMING | _native.RT_FLAG_NO_LIN_DETREND | _native.RT_FLAG_GROUP_DETECT
                                           | _native.RT_FLAG_NO_GROUP_DETECT | _native.RT_FLAG_ROW_MEANS) == 0
    m = re.search(r"#define\s+RT_ABI_VERSION\s+(\d+)", text)
    assert m and int(m.group(1)) == 6
    assert _native.load_library().rt_abi_version() == 6


def test_symbols_exported_and_null_handle_refused(lib):
    raw = C.CDLL(_native.LIB_PATH)
    for name in ("rt_fetch_record_cells", "rt_fetch_record_cells_f64"):
        assert name in _native.ABI_SYMBOLS
        assert hasattr(raw, name), name
    off = np.zeros(4, dtype=np.int64)
    n = C.c_size_t(7)
    for fn, dt in ((lib.rt_fetch_record_cells, np.float32), (lib.rt_fetch_record_cells_f64, np.float64)):
        cells = np.zeros(16, dtype=dt)
        assert fn(None, off.ctypes.data, off.size, cells.ctypes.data, cells.size, C.byref(n)) == _native.RT_E_INVALID
        assert fn(None, None, 0, None, 0, C.byref(n)) == _native.RT_E_INVALID
        assert fn(None, None, 0, None, 0, None) == _native.RT_E_INVALID


def test_create_with_flag_without_gpu_fails_loudly(lib):
    n = C.c_int(0)
    lib.rt_device_count(C.byref(n))
    if n.value > 0:
        pytest.skip("a GPU is present")
    for precision in ("float32", "float64"):
        with pytest.raises(_native.NativeError) as ei:
            BatchSignalAnalyzer(["0", "1"], record_cells=True, precision=precision, sdr_callback_length=4096)
        assert ei.value.code == _native.RT_E_NO_DEVICE
    with pytest.raises(_native.NativeError) as ei:
        SignalAnalyzer("0", record_cells=True, sdr_callback_length=4096)
    assert ei.value.code == _native.RT_E_NO_DEVICE


def _extract(hc, c, f64):
    kw = c["kwargs"]
    p = oracle.ExtractParams(kw["signal_threshold_dbw"], kw["snr_threshold_db"], kw["signal_min_duration_ms"],
                             kw["signal_max_duration_ms"], kw["calibration_db"])
    dt = np.float64 if f64 else np.float32
    cur = np.ascontiguousarray(c["cur"].T, dtype=dt)  # [T][F]
    n_seg, n_bins = cur.shape
    last = np.ascontiguousarray(c["last"].T, dtype=dt) if c["has_last"] else None
    n_last = last.shape[0] if last is not None else 0
    last_ptr = None if last is None else (last.ctypes.data if last.size else C.c_void_p(8))
    out = np.zeros(512, dtype=_native.RECORD_F64_DTYPE if f64 else _native.RECORD_DTYPE)
    cast = (lambda v: float(v)) if f64 else np.float32
    n = (hc.hc_extract_f64 if f64 else hc.hc_extract)(
        cur.ctypes.data, n_seg, n_bins, last_ptr, n_last, n_last, 256, float(kw["sample_rate"]),
        cast(p.signal_threshold), cast(p.snr_threshold), cast(kw["calibration_db"]),
        p.signal_min_duration, p.signal_max_duration, out.ctypes.data, len(out))
    assert n <= len(out)
    rec = out[:n]
    offsets = np.full(n + 1, -1, dtype=np.int64)
    want_total = int(np.sum(rec["end"] - rec["start"]))
    cells = np.full(want_total + 3, -1.0, dtype=dt)
    fn = hc.hc_record_cells_f64 if f64 else hc.hc_record_cells
    total = fn(cur.ctypes.data, n_bins, last_ptr, n_last, rec.ctypes.data, n, offsets.ctypes.data, cells.ctypes.data, want_total)
    assert total == want_total
    assert np.all(cells[want_total:] == -1.0)  # nothing written past the cells
    return cur, last, rec, offsets, cells[:want_total]


@pytest.mark.parametrize("f64", [False, True], ids=["float32", "float64"])
def test_host_record_cells_on_all_planted_maps(hc, f64):
    index = gu.extract_index()
    assert len(index) == 160
    n_records = n_back = 0
    for i in range(len(index)):
        c = gu.extract_case(i)
        cur, last, rec, offsets, cells = _extract(hc, c, f64)
        assert offsets[0] == 0 and np.array_equal(np.diff(offsets), rec["end"] - rec["start"]), i
        for r, o0, o1 in zip(rec, offsets[:-1], offsets[1:]):
            fi, start, end = int(r["fi"]), int(r["start"]), int(r["end"])
            row = cur[:, fi]
            want = np.concatenate((last[:, fi][start:], row[:end])) if start < 0 else row[start:end]  # analyze.py:437-440
            got = cells[o0:o1]
            assert len(want) == end - start and np.array_equal(rcu.bits(got), rcu.bits(want)), (i, fi, start, end)
            mx, mean, std = rcu.run_stats(got)
            assert np.array_equal(rcu.bits(np.array([mx, mean])), rcu.bits(np.array([r["max_p"], r["mean_p"]]))), (i, fi, start, end)
            assert (np.isnan(std) and np.isnan(r["std_db"])) or abs(float(std) - float(r["std_db"])) <= 1e-4, (i, fi, start, end)
            n_records += 1
            n_back += start < 0
    assert n_records > 100 and n_back > 0  # (the cases hold records, some of them reaching back into the previous map)


def test_host_record_cells_reports_the_size_when_the_buffer_is_short(hc):
    for i in range(len(gu.extract_index())):
        c = gu.extract_case(i)
        cur, last, rec, offsets, cells = _extract(hc, c, False)
        if len(cells) < 2:
            continue
        short = np.full(len(cells), -1.0, dtype=np.float32)
        off2 = np.zeros(len(rec) + 1, dtype=np.int64)
        n_last = last.shape[0] if last is not None else 0
        last_ptr = None if last is None else (last.ctypes.data if last.size else C.c_void_p(8))
        total = hc.hc_record_cells(cur.ctypes.data, cur.shape[1], last_ptr, n_last, rec.ctypes.data, len(rec), off2.ctypes.data,
                                   short.ctypes.data, len(cells) - 1)
        assert total == len(cells) and np.array_equal(off2, offsets) and np.all(short == -1.0)
        return
    pytest.fail("no case with cells")
