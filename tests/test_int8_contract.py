"""8-bit signed IQ (rt_process_i8 / rt_process_i8_host, enqueue_int8, process_int8) without a GPU: the conversions of
``synth`` are exact, the entry points are declared and exported, a null handle is refused, argument errors are raised in
Python before any native call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from pyradiotracking_amd import _native, build, synth
from pyradiotracking_amd.analyze import BatchSignalAnalyzer, SignalAnalyzer

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rt_process_i8", "rt_process_i8_host")


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _native.load_library()


def test_every_int8_value_converts_exactly():
    i = np.arange(-128, 128, dtype=np.int8)
    raw = np.stack([i, i[::-1]], axis=-1).reshape(1, -1)  # sample k = (i[k], i[-1 - k]): every value on I and on Q
    for conv, dt in ((synth.i8_to_complex64, np.complex64), (synth.i8_to_complex128, np.complex128)):
        c = conv(raw)
        assert c.dtype == dt and c.shape == (1, 256)
        assert np.array_equal(c.real.astype(np.float64) * 128, i.astype(np.float64)[None, :])
        assert np.array_equal(c.imag.astype(np.float64) * 128, i[::-1].astype(np.float64)[None, :])
    assert synth.I8_SCALE == 2.0 ** -7
    c = synth.i8_to_complex64(np.array([-128, 127], dtype=np.int8))
    assert c.shape == (1,) and c[0].real == -1.0 and float(c[0].imag) == 1.0 - 2.0 ** -7
    # quantising what was converted gives the integers back, from either precision
    assert np.array_equal(synth.quantize_i8(synth.i8_to_complex64(raw)), raw)
    assert np.array_equal(synth.quantize_i8(synth.i8_to_complex128(raw)), raw)


def test_all_byte_pairs_convert_exactly():
    """Every (I, Q) pair: the conversion keeps the components apart (no byte swapped, no sign carried from Q into I)."""
    i, q = np.meshgrid(np.arange(-128, 128), np.arange(-128, 128), indexing="ij")
    raw = np.stack([i.ravel(), q.ravel()], axis=-1).astype(np.int8).reshape(1, -1)
    c = synth.i8_to_complex64(raw)
    assert np.array_equal(c.real[0] * 128, i.ravel()) and np.array_equal(c.imag[0] * 128, q.ravel())


def test_quantize_rounds_clips_and_interleaves():
    x = np.array([0.25 + 0.5j, -1.0 + (1.0 - 2.0 ** -7) * 1j, 1.0 - 3.0j, 1.5 / 128 + 2.5j / 128, -0.5 / 128 - 1.5j / 128])
    q = synth.quantize_i8(x)
    assert q.dtype == np.int8 and q.shape == (10,)
    # I then Q; 1.0 and -3.0 clip; ties go to even (np.rint)
    assert q.tolist() == [32, 64, -128, 127, 127, -128, 2, 2, 0, -2]
    g = synth.quantize_i8(np.array([[0.01 - 0.02j, 0.5 - 0.5j]]), gain=4.0)
    assert g.shape == (1, 4) and g.tolist() == [[5, -10, 127, -128]]
    assert np.array_equal(g, np.clip(np.rint(np.array([[0.01, -0.02, 0.5, -0.5]]) * 4.0 * 128), -128, 127).astype(np.int8))
    x2 = np.random.default_rng(1).standard_normal((3, 50)) + 1j * np.random.default_rng(2).standard_normal((3, 50))
    q2 = synth.quantize_i8(x2, gain=3.0)
    assert q2.shape == (3, 100) and q2.min() == -128 and q2.max() == 127
    c = synth.i8_to_complex128(q2)
    inside = (np.abs(x2.real * 3.0) < 0.99) & (np.abs(x2.imag * 3.0) < 0.99)
    assert inside.any() and np.all(np.abs(c - x2 * 3.0)[inside] <= 2.0 ** -7)  # half a step per component


def test_entry_points_declared_exported_and_null_handle_refused(lib):
    text = open(os.path.join(REPO, "include", "rt_analyze.h")).read()
    raw = C.CDLL(_native.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*rt_handle\s*\*\s*h\s*,\s*const\s+void\s*\*\s*\w+\s*,\s*int64_t\s+n_samples\s*,\s*int64_t\s+stream_stride\s*\)\s*;", text), name
        assert name in _native.ABI_SYMBOLS
        assert hasattr(raw, name), name
    buf = np.zeros(64, dtype=np.int8)
    assert lib.rt_process_i8(None, buf.ctypes.data, 32, 32) == _native.RT_E_INVALID
    assert lib.rt_process_i8_host(None, buf.ctypes.data, 32, 32) == _native.RT_E_INVALID
    assert lib.rt_process_i8(None, None, 0, 0) == _native.RT_E_INVALID
    assert lib.rt_process_i8_host(None, None, 0, 0) == _native.RT_E_INVALID


class _NoNative:
    """Stands where the native analyzer would: any call into the library is a test failure."""

    def __getattr__(self, name):
        raise AssertionError(f"native call {name} before the arguments were checked")


def _batch_without_device(n_streams=2, blen=64, precision="float32"):
    b = BatchSignalAnalyzer.__new__(BatchSignalAnalyzer)
    b.devices = [str(i) for i in range(n_streams)]
    b.sdr_callback_length = blen
    b.precision = precision
    b._native = _NoNative()
    b._hip_stream = None
    b._held = []
    return b


@pytest.mark.parametrize("precision", ["float32", "float64"])
def test_enqueue_int8_argument_errors_come_before_any_native_call(precision):
    b = _batch_without_device(precision=precision)
    try:
        for bad in (np.zeros((2, 64), dtype=np.uint8), np.zeros((2, 64), dtype=np.int16), np.zeros((2, 64), dtype=np.float32),
                    np.zeros((2, 32), dtype=np.complex64)):
            with pytest.raises(TypeError):
                b.enqueue_int8(bad)
        with pytest.raises(ValueError):
            b.enqueue_int8(np.zeros((2, 63), dtype=np.int8))  # an I without its Q
        with pytest.raises(ValueError):
            b.enqueue_int8(np.zeros((3, 64), dtype=np.int8))  # three streams for two
        with pytest.raises(ValueError):
            b.enqueue_int8(np.zeros(64, dtype=np.int8))  # one stream for two
        with pytest.raises(ValueError):
            b.enqueue_int8(np.zeros((2, 2, 32), dtype=np.int8))
        with pytest.raises(ValueError, match="sdr_callback_length"):
            b.enqueue_int8(np.zeros((2, 2 * 65), dtype=np.int8))
        with pytest.raises(ValueError, match="n_samples"):
            b.enqueue_int8(4096)  # a raw pointer without its length
    finally:
        b._native = None  # (nothing to close)


def test_process_int8_argument_errors_come_before_any_native_call():
    sa = SignalAnalyzer.__new__(SignalAnalyzer)
    sa._batch = _batch_without_device(1, 64)
    clock = []
    sa._clock = lambda n: clock.append(n)
    for bad in (np.zeros(64, dtype=np.uint8), np.zeros(64, dtype=np.int16), np.zeros(32, dtype=np.complex64)):
        with pytest.raises(TypeError):
            sa.process_int8(bad)
    with pytest.raises(ValueError):
        sa.process_int8(np.zeros(63, dtype=np.int8))
    with pytest.raises(ValueError, match="sdr_callback_length"):
        sa.process_int8(np.zeros(2 * 65, dtype=np.int8))
    assert clock == []  # a refused buffer does not move the clock
    sa._batch._native = None


def test_native_binding_checks_shape_and_dtype_itself():
    n = _native.NativeAnalyzer.__new__(_native.NativeAnalyzer)
    n.n_streams = 2
    n._lib = _NoNative()
    n._handle = None
    try:
        with pytest.raises(TypeError):
            n.process_host_i8(np.zeros((2, 64), dtype=np.uint8))
        with pytest.raises(TypeError):
            n.process_host_i8(np.zeros((2, 64), dtype=np.int16))
        with pytest.raises(ValueError):
            n.process_host_i8(np.zeros((2, 63), dtype=np.int8))
        with pytest.raises(ValueError):
            n.process_host_i8(np.zeros((1, 64), dtype=np.int8))
    finally:
        n._lib = None
