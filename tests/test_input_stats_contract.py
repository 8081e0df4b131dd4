"""rt_set_input_stats / rt_fetch_input_stats without a GPU: the entries exist and check their arguments first; the kernels' own
arithmetic -- chunks, threads, butterfly, fold, run on the host through ``rt_hostcheck`` (``hc_input_stats``) -- against the NumPy
model on every case of the table (tests/input_stats_cases.py), at every alignment of the row; the packed 8-bit form against the
per-component rule on every byte value; the same as a stand-alone program under AddressSanitizer and UBSan
(tests/c/input_stats_work.cpp); five planted faults in a NumPy restatement that the table rejects; ``input_levels`` against plain
NumPy."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from pyradiotracking_amd import _native, build
from pyradiotracking_amd.analyze import input_levels
from tests import input_stats_cases as isc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hc():
    lib = C.CDLL(build.build_hostcheck())
    lib.hc_input_stats_chunk.restype = C.c_int
    lib.hc_input_stats.argtypes = [C.c_int, C.c_void_p, C.c_longlong, C.c_void_p]
    lib.hc_input_stats_words8.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    return lib


@pytest.fixture(scope="module")
def chunk(hc):
    return int(hc.hc_input_stats_chunk())


def host_row(hc, fmt, comps, shift=0):
    """``hc_input_stats`` on a copy of the row that begins ``shift`` samples into a 16-byte aligned block"""
    comps = np.ascontiguousarray(comps, dtype=isc.DTYPE[fmt])
    raw = np.zeros(comps.nbytes + 64, dtype=np.uint8)
    off = (-raw.ctypes.data) % 16 + shift * isc.SAMPLE_BYTES[fmt]
    raw[off:off + comps.nbytes] = comps.view(np.uint8)
    out = np.zeros(1, dtype=_native.INPUT_STATS_DTYPE)
    assert hc.hc_input_stats(isc.FMT_CODE[fmt], raw.ctypes.data + off, comps.size // 2, out.ctypes.data) == 0
    return out[0]


def test_the_entries_exist_and_check_their_arguments_first():
    build.build_library()
    lib = _native.load_library()
    raw = C.CDLL(_native.LIB_PATH)
    for name in ("rt_set_input_stats", "rt_fetch_input_stats"):
        assert hasattr(raw, name) and name in _native.ABI_SYMBOLS
    out = np.zeros(3, dtype=_native.INPUT_STATS_DTYPE)
    assert lib.rt_set_input_stats(None, 1) == _native.RT_E_INVALID               # a null handle
    assert lib.rt_fetch_input_stats(None, out.ctypes.data, 3) == _native.RT_E_INVALID
    assert lib.rt_fetch_input_stats(None, None, 0) == _native.RT_E_INVALID
    assert _native.INPUT_STATS_DTYPE.itemsize == 64 and lib.rt_abi_version() == 6
    assert [_native.INPUT_STATS_DTYPE.fields[n][1] for n in _native.INPUT_STATS_DTYPE.names] == [0, 8, 16, 24, 32, 40, 48, 56, 60]


def test_the_chunk_length_is_a_whole_number_of_pieces_and_segments(chunk):
    assert chunk >= 1024 and chunk % 256 == 0  # (the GPU suite's sizes C - 1, C, C + 1 hold more than one segment of 256)


def test_the_host_form_equals_the_model_on_every_case(hc, chunk):
    worst = {}
    for name, fmt, comps in isc.table(chunk):
        model = isc.model_row(fmt, comps)
        rows = [host_row(hc, fmt, comps, shift) for shift in range(16 // isc.SAMPLE_BYTES[fmt])]
        for shift, got in enumerate(rows):
            r = isc.compare(fmt, got, model, f"{name} shift {shift}")
            worst[fmt] = max(worst.get(fmt, 0.0), r)
            # the same samples at another alignment: the same bytes
            assert got.tobytes() == rows[0].tobytes(), (name, shift)
    print("hc_input_stats against the model, worst |got - fsum| / bound:", {k: round(v, 4) for k, v in worst.items()})
    out = np.zeros(1, dtype=_native.INPUT_STATS_DTYPE)
    assert hc.hc_input_stats(5, None, 0, out.ctypes.data) == -1 and hc.hc_input_stats(-1, None, 0, out.ctypes.data) == -1


@pytest.mark.parametrize("fmt", ["u8", "i8"])
def test_the_packed_form_equals_the_rule_on_every_byte(hc, fmt):
    rng = np.random.default_rng(5)
    packed, rule = np.zeros(5, dtype=np.int64), np.zeros(5, dtype=np.int64)
    for b in range(256):
        for pos in range(4):
            words = rng.integers(0, 2 ** 32, 8, dtype=np.uint64).astype(np.uint32)
            words[3] = (int(words[3]) & ~(0xFF << (8 * pos))) | (b << (8 * pos))
            words[5] = 0x01010101 * b
            assert hc.hc_input_stats_words8(isc.FMT_CODE[fmt], words.ctypes.data, 8, packed.ctypes.data, rule.ctypes.data) == 0
            assert packed.tolist() == rule.tolist(), (fmt, b, pos)
            comps = words.view(isc.DTYPE[fmt])
            m = isc.model_row(fmt, comps)
            assert rule.tolist() == [m["n_rail"], int(m["sum_i"]), int(m["sum_q"]), int(m["sum_sq"]), int(m["peak"])], (fmt, b, pos)


def test_the_host_form_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "input_stats_work"
    # (the runtimes linked statically: the program then runs the same whatever else the environment loads into a process)
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "pyradiotracking_amd", "csrc"), "-o", str(exe),
                    os.path.join(REPO, "tests", "c", "input_stats_work.cpp")], check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr)


def test_the_restatement_without_a_fault_passes_every_case(chunk):
    for name, fmt, comps in isc.table(chunk):
        assert not isc.rejects(fmt, isc.restated_row(fmt, comps), isc.model_row(fmt, comps)), name


@pytest.mark.parametrize("fault", isc.FAULTS)
def test_a_planted_fault_is_rejected_by_the_table(chunk, fault):
    caught = [name for name, fmt, comps in isc.table(chunk) if isc.rejects(fmt, isc.restated_row(fmt, comps, fault), isc.model_row(fmt, comps))]
    print(f"{fault}: rejected by {len(caught)} cases, e.g. {caught[:3]}")
    assert caught, fault
    want = {"square32": "i16 all -32768", "low_rail": "i8 all -128", "ragged": "u8 random n=255", "nan_added": "c64 all NaN", "u8_minus_128": "u8 all 255"}[fault]
    assert want in caught, (fault, caught)


def test_input_levels_against_plain_numpy(chunk):
    rows, want = [], []
    for fmt in isc.FORMATS:
        comps = isc.random_row(fmt, chunk + 17, 3, chunk, specials=False)
        rows.append(isc.model_row(fmt, comps))
        v = isc.raw_int(fmt, comps).astype(np.float64) / isc.UNIT[fmt] if not isc.is_float(fmt) else comps.astype(np.float64)
        n = comps.size // 2
        want.append((np.mean(v[0::2]), np.mean(v[1::2]), 10 * np.log10(np.sum(v * v) / n), np.count_nonzero(np.abs(v) >= 1.0 if isc.is_float(fmt) else
                     np.isin(comps, isc.RAILS[fmt])) / (2 * n), np.max(np.abs(v))))
    rows.append(dict(isc.model_row("u8", np.zeros(0, np.uint8))))  # a stream without samples
    got = input_levels(isc.stats_array(rows))
    assert got.shape == (len(isc.FORMATS) + 1,)
    for g, w in zip(got, want):
        np.testing.assert_allclose([g["dc_i"], g["dc_q"], g["power_dbfs"], g["rail_fraction"], g["peak"]], w, rtol=1e-12, atol=1e-15)
        assert g["nonfinite"] == 0
    last = got[-1]
    assert all(np.isnan(last[f]) for f in ("dc_i", "dc_q", "power_dbfs", "rail_fraction", "peak")) and last["nonfinite"] == 0
    # uint8: the documented value b / 127.5 - 1, and a full-scale square wave is 0 dBFS with every component at a rail
    sq = isc.stats_array([isc.model_row("u8", np.tile(np.array([0, 255, 255, 0], np.uint8), 64))])
    lv = input_levels(sq)[0]
    assert lv["power_dbfs"] == pytest.approx(10 * np.log10(2.0)) and lv["rail_fraction"] == 1.0 and lv["peak"] == 1.0 and lv["dc_i"] == 0.0
    nf = isc.stats_array([isc.model_row("c64", np.array([np.nan, 0.5, 0.25, np.inf], np.float32))])
    assert input_levels(nf)[0]["nonfinite"] == 2 and input_levels(nf[0])[0]["dc_i"] == 0.125
