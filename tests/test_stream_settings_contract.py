"""Per-stream detection settings (rt_set_stream_settings[_f64]) without a GPU: the two entry points are declared and exported
within ABI version 6, a null handle is refused, a per-device keyword of the wrong length is refused before the library is asked
for a device, the decoder adds every stream's own centre frequency, and BatchRunner hands each GPU its devices' values."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from pyradiotracking_amd import _native, build
from pyradiotracking_amd import analyze as analyze_mod
from pyradiotracking_amd.analyze import BatchSignalAnalyzer, _RecordDecoder
from pyradiotracking_amd.runner import BatchRunner

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rt_set_stream_settings", "rt_set_stream_settings_f64")
PER_DEVICE = ("snr_threshold_db", "signal_min_duration_ms", "signal_max_duration_ms", "signal_threshold_dbw", "center_freq")


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _native.load_library()


def test_both_entries_are_declared_and_exported(lib):
    text = open(os.path.join(REPO, "include", "rt_analyze.h")).read()
    raw = C.CDLL(_native.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*rt_handle\s*\*", text), name
        assert name in _native.ABI_SYMBOLS
        assert hasattr(raw, name), name


def test_null_handle_is_refused(lib):
    snr32, snr64, dur = np.full(4, 3.0, np.float32), np.full(4, 3.0), np.full(4, 0.01)
    assert lib.rt_set_stream_settings(None, snr32.ctypes.data, dur.ctypes.data, dur.ctypes.data) == _native.RT_E_INVALID
    assert lib.rt_set_stream_settings_f64(None, snr64.ctypes.data, dur.ctypes.data, dur.ctypes.data) == _native.RT_E_INVALID
    assert lib.rt_set_stream_settings(None, None, None, None) == _native.RT_E_INVALID
    assert lib.rt_set_stream_settings_f64(None, None, None, None) == _native.RT_E_INVALID


def test_abi_version_is_still_6(lib):
    text = open(os.path.join(REPO, "include", "rt_analyze.h")).read()
    assert re.search(r"#define\s+RT_ABI_VERSION\s+6\b", text)
    assert lib.rt_abi_version() == 6
    assert all(name in text for name in ENTRIES)  # ... with the new entries in it


class _NoNative:
    """stands in for _native.NativeAnalyzer: a length mismatch must be refused before the library is asked for a device"""

    def __init__(self, **kw):
        raise AssertionError("the native library was asked for a handle")


@pytest.mark.parametrize("name", PER_DEVICE)
def test_wrong_length_raises_before_any_native_call(monkeypatch, name):
    monkeypatch.setattr(analyze_mod._native, "NativeAnalyzer", _NoNative)
    value = {"center_freq": [150000000]}.get(name, [5.0])
    with pytest.raises(ValueError, match=name):
        BatchSignalAnalyzer(["0", "1"], sdr_callback_length=4096, **{name: value})
    with pytest.raises(ValueError, match=name):
        BatchSignalAnalyzer(["0", "1"], sdr_callback_length=4096, **{name: value * 3})
    # (the right length gets as far as the native handle)
    with pytest.raises(AssertionError, match="asked for a handle"):
        BatchSignalAnalyzer(["0", "1"], sdr_callback_length=4096, **{name: value * 2})


def test_decoder_adds_every_streams_own_centre_frequency():
    nperseg, fs = 256, 300000
    centers = [150150000, 433920000]
    dec = _RecordDecoder(nperseg, fs, centers, 0.0)
    rec = np.zeros(4, dtype=_native.RECORD_DTYPE)
    rec["stream"] = [0, 0, 1, 1]
    rec["fi"] = [3, 200, 3, 200]
    rec["start"], rec["end"] = 2, 14
    rec["max_p"] = rec["mean_p"] = rec["row_mean"] = 1e-9
    frequency = dec.decode(rec)[2]
    want = [dec.freqs[fi] + centers[s] for s, fi in zip(rec["stream"], rec["fi"])]  # analyze.py:360, per SDR
    assert frequency.tolist() == want
    assert frequency[2] - frequency[0] == centers[1] - centers[0]
    import datetime

    import pytz

    ts = datetime.datetime(2024, 1, 1, tzinfo=pytz.utc)
    sigs = dec.signals(rec, ["a", "b"], [ts, ts])
    assert [s.frequency for s in sigs] == want and [s.device for s in sigs] == ["a", "a", "b", "b"]
    assert [s.frequency for s in dec.signal_batch(rec, ["a", "b"], [ts, ts])] == want
    # one value for all streams: as before
    assert _RecordDecoder(nperseg, fs, centers[0], 0.0).decode(rec)[2].tolist() == [dec.freqs[fi] + centers[0] for fi in rec["fi"]]


class _FakeBatch:
    created = []

    def __init__(self, devices, calibration_db=0.0, gpu=0, **kw):
        self.devices, self.calibration_db, self.gpu, self.kw = list(devices), calibration_db, gpu, kw
        _FakeBatch.created.append(self)

    def close(self):
        pass


def test_batch_runner_slices_per_device_keywords_per_gpu():
    _FakeBatch.created = []
    devices = list("abcde")
    r = BatchRunner(device=devices, calibration=[0.0, 1.0, 2.0, 3.0, 4.0], gpus=[0, 1], analyzer_factory=_FakeBatch, sample_rate=300000,
                    snr_threshold_db=[3.0, 4.0, 5.0, 6.0, 7.0], signal_min_duration_ms=[8, 9, 10, 11, 12], signal_max_duration_ms=40,
                    signal_threshold_dbw=[-90.0, -89.0, -88.0, -87.0, -86.0], center_freq=[1, 2, 3, 4, 5], fft_window=np.hamming(5))
    r.start_analyzers()
    first, second = _FakeBatch.created
    assert first.devices == ["a", "b", "c"] and second.devices == ["d", "e"]
    assert first.calibration_db == [0.0, 1.0, 2.0] and second.calibration_db == [3.0, 4.0]
    assert first.kw["snr_threshold_db"] == [3.0, 4.0, 5.0] and second.kw["snr_threshold_db"] == [6.0, 7.0]
    assert first.kw["signal_min_duration_ms"] == [8, 9, 10] and second.kw["signal_min_duration_ms"] == [11, 12]
    assert first.kw["signal_threshold_dbw"] == [-90.0, -89.0, -88.0] and second.kw["signal_threshold_dbw"] == [-87.0, -86.0]
    assert first.kw["center_freq"] == [1, 2, 3] and second.kw["center_freq"] == [4, 5]
    # scalars, and sequences that are not per-device settings, go to every analyzer as they are
    assert first.kw["signal_max_duration_ms"] == 40 and second.kw["signal_max_duration_ms"] == 40
    assert len(first.kw["fft_window"]) == 5 and len(second.kw["fft_window"]) == 5
    r.stop_analyzers()
    with pytest.raises(ValueError, match="snr_threshold_db"):
        BatchRunner(device=devices, gpus=[0, 1], analyzer_factory=_FakeBatch, snr_threshold_db=[3.0, 4.0])
