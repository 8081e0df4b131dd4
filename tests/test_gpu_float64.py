"""The HIP kernels against a float64 transform of the same inputs, within the float32 round-off model of
``tests/precision64.py`` (the model itself is tested on the CPU in ``tests/test_precision_model.py``): every cell of the
dense map of every transform family, and the float fields of every record of every detection path.  The records' identity
(bin, start, end, shadow verdict) must still equal the oracle's.  Each test adds its worst ratio (|gpu - f64| / bound) per
family to ``WORST``; the last test prints them beside SciPy's."""
import datetime

import numpy as np
import pytest

from oracle import analyze_oracle as oracle
from pyradiotracking_amd import _native, synth
from pyradiotracking_amd.analyze import BatchSignalAnalyzer
from tests import precision64 as p64

pytestmark = pytest.mark.gpu

WORST = {}  # (family, what) -> worst ratio
LIN_WINDOWS = ("hamming", "hann", "boxcar")
_TS0 = datetime.datetime(2024, 1, 1, tzinfo=datetime.timezone.utc)


def _need_gpu():
    if _native.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")


def family(nperseg):
    if nperseg in (8, 16):
        return "general"
    if nperseg & (nperseg - 1):
        return "bluestein"
    if nperseg <= 128:
        return "scan_lanegroups"
    return {4096: "scan64", 8192: "wg", 16384: "wg"}.get(nperseg, "scan")


def form_of(nperseg, window, subtract_first=False, u8=False):
    """The detrend form the handle runs: the fused scans up to 4096 take the linearity form for cosine-sum windows of order
    <= 1 on complex64 input unless asked not to (rt_create); everything else subtracts the mean first."""
    lin = (isinstance(window, str) and window in LIN_WINDOWS and 32 <= nperseg <= 4096 and nperseg & (nperseg - 1) == 0
           and not subtract_first and not u8)
    return "lin" if lin else "sub"


def _note(fam, what, r):
    WORST[(fam, what)] = max(WORST.get((fam, what), 0.0), float(r))


def _batch(n_streams, blen, fs, nperseg, window, mode, **extra):
    return BatchSignalAnalyzer([str(i) for i in range(n_streams)], sdr_callback_length=blen, mode=mode, sample_rate=fs,
                               fft_nperseg=nperseg, fft_window=window, **extra)


def _streams(S, n, fs, nperseg, window, seed, dc=None, pulses=3, peak=(-80.0, -60.0), dur_ms=(2, 6), sigma=synth.NOISE_SIGMA):
    w = oracle.window_coefficients(window, nperseg)
    out = []
    for s in range(S):
        rng = np.random.default_rng([seed, s])
        p = synth.random_pulses(rng, n, fs, w, pulses, dur_ms=dur_ms, peak_dbw=peak) if pulses else []
        out.append(synth.make_stream(synth.StreamSpec(n, fs, p, noise_sigma=sigma, dc=(dc[s] if dc else 0j)), seed * 1000 + s))
    return np.stack(out)


# ----------------------------------------------------------------------------------------------------------------------
# dense map, every cell
# ----------------------------------------------------------------------------------------------------------------------
def _check_map(iq, fs, nperseg, window, streams=None, stride=None, subtract_first=False, lanes=1):
    S, n = iq.shape
    T = n // nperseg
    b = _batch(S, n, fs, nperseg, window, "dense", subtract_first=subtract_first, lanes=lanes)
    stride = stride or n
    host = np.zeros((S, stride), np.complex64)
    host[:, :n] = iq
    d_iq = _native.DeviceBuffer(0, host.nbytes)
    d_iq.upload(host)
    d_out = _native.DeviceBuffer(0, S * T * nperseg * 4)
    b.native.spectrogram_device(d_iq.ptr, n, stride, d_out.ptr)
    got = d_out.download(np.float32, S * T * nperseg).reshape(S, T, nperseg)
    d_iq.free()
    d_out.free()
    b.close()
    form = form_of(nperseg, window, subtract_first)
    worst = 0.0
    for s in (range(S) if streams is None else streams):
        ref = p64.stft_power_f64(iq[s], fs, window, nperseg)
        r = p64.cell_ratios(got[s], ref, p64.cell_bounds(ref, form))
        t, k = np.unravel_index(np.argmax(r), r.shape)
        assert r.max() <= 1.0, (f"nperseg {nperseg} {window} {form} stream {s}: cell (t={t}, k={k}) at {r.max():.3f} of its bound: "
                                f"{got[s][t, k]!r} vs {ref.P[t, k]!r}")
        worst = max(worst, r.max())
    _note(family(nperseg), f"cells ({form})", worst)
    return worst


_MAP_CASES = ([(n, "hamming") for n in (32, 64, 128, 256, 512, 1024, 2048, 4096)]
              + [(128, "blackmanharris"), (1024, "hann"), (8192, "hann"), (8192, "blackmanharris"), (16384, "hamming"),
                 (16384, ("tukey", 0.3)), (8, "hann"), (16, "hamming")]
              + [(n, "hann") for n in (9, 17, 129, 257, 300, 1000, 1025, 2049, 4097, 8191)])


@pytest.mark.parametrize("nperseg,window", _MAP_CASES, ids=[f"{n}-{w if isinstance(w, str) else w[0]}" for n, w in _MAP_CASES])
def test_dense_map_every_cell(nperseg, window):
    """Three streams (clean; an offset of 2e-3 and pulses; pulses), a ragged tail; both detrend forms where they exist."""
    _need_gpu()
    fs = 2048000
    T = int(np.clip(400000 // nperseg, 12, 200))
    n = T * nperseg + nperseg // 3
    iq = _streams(3, n, fs, nperseg, window, seed=nperseg, dc=[0j, complex(2e-3, -1e-3), 0j])
    iq[0] = synth.make_stream(synth.StreamSpec(n, fs, []), 5)
    _check_map(iq, fs, nperseg, window)
    if form_of(nperseg, window) == "lin":
        _check_map(iq, fs, nperseg, window, subtract_first=True)


def test_dense_map_lanes_and_a_stride_longer_than_the_buffer():
    _need_gpu()
    fs, nperseg = 2048000, 512
    n = 150 * nperseg + 77
    iq = _streams(4, n, fs, nperseg, "hann", seed=31, dc=[complex(1e-3, 1e-3)] * 4)
    _check_map(iq, fs, nperseg, "hann", lanes=2)
    _check_map(iq, fs, nperseg, "hann", stride=n + 1000)


def test_dense_map_with_several_work_items_per_workgroup():
    """64 streams x 4 000 segments at nperseg 256: streams x chunks (64 x 125) far over what the chip holds at once, so the
    persistent grid hands every workgroup several items; the first, a middle and the last stream checked in full."""
    _need_gpu()
    fs, nperseg, S = 2048000, 256, 64
    n = 4000 * nperseg
    iq = _streams(S, n, fs, nperseg, "hamming", seed=64, pulses=6)
    _check_map(iq, fs, nperseg, "hamming", streams=(0, 33, 63))
    _check_map(iq, fs, nperseg, "hamming", streams=(0, 63), subtract_first=True)


# ----------------------------------------------------------------------------------------------------------------------
# records
# ----------------------------------------------------------------------------------------------------------------------
def _shadow_flags(signals):
    return [oracle.shadow_index(s, signals) is not None for s in signals]


def _check_records(bufs, fs, nperseg, window, mode, streams=None, u8=False, sub_streams=(), expect=None, oracle_kw=None, **extra):
    """``bufs`` [S, n_buffers, B]: complex64, or uint8 wire bytes [S, n_buffers, 2 B].  Every buffer goes through one handle;
    the records of the checked streams must have the oracle's identity and float64 fields within the model."""
    S, nb = bufs.shape[:2]
    B = bufs.shape[2] // (2 if u8 else 1)
    b = _batch(S, B, fs, nperseg, window, mode, **extra, **(oracle_kw or {}))
    kw = dict(sample_rate=fs, fft_nperseg=nperseg, fft_window=window, **(oracle_kw or {}))
    streams = range(S) if streams is None else streams
    oas = {s: oracle.OracleAnalyzer(**kw) for s in streams}
    prev = {s: None for s in streams}
    fam = family(nperseg)
    n_rec = n_neg = 0
    infos = []
    for k in range(nb):
        chunk = np.ascontiguousarray(bufs[:, k])
        (b.enqueue_bytes if u8 else b.enqueue)(chunk)
        rec = b.fetch_records()
        info = b.native.call_info()
        infos.append((info.mode_used, info.fell_back, info.n_dense_streams))
        L = max(1, int(info.segs_per_chunk))
        for s in streams:
            x = synth.u8_to_complex64_like_kernel(chunk[s]) if u8 else chunk[s]
            freqs, times, spec = oracle.stft_power(x, fs, window, nperseg)
            recs = oracle.extract_records(times, spec, oas[s].spec_last, oas[s].params)
            sigs = oracle.records_to_signals(recs, freqs, _TS0, str(s), 0)
            oas[s].spec_last = spec
            mine = rec[rec["stream"] == s]
            assert [(int(r["fi"]), int(r["start"]), int(r["end"])) for r in mine] == [(r.fi, r.start, r.end) for r in recs], (mode, k, s)
            assert [bool(r["shadowed"]) for r in mine] == _shadow_flags(sigs), (mode, k, s)
            ref = p64.stft_power_f64(x, fs, window, nperseg)
            form = "sub" if s in sub_streams else form_of(nperseg, window, extra.get("subtract_first", False), u8)
            bd = p64.cell_bounds(ref, form)
            pr = prev[s]
            chk = p64.check_records(mine, ref, bd, L, pr[0] if pr else None, pr[1] if pr else None, what=f"{mode} buffer {k} stream {s}")
            assert not chk.failures, "\n".join(chk.failures[:8])
            for f, v in chk.worst.items():
                _note(fam, f"{f} ({form})", v)
            prev[s] = (ref, bd)
            n_rec += len(mine)
            n_neg += int((mine["start"] < 0).sum())
    b.close()
    assert n_rec > 0
    if expect is not None:
        assert expect(infos, n_neg) is not False, infos
    return n_rec, n_neg


def _split(iq, nb):
    S, n = iq.shape
    return iq[:, : (n // nb) * nb].reshape(S, nb, n // nb)


@pytest.mark.parametrize("mode,group_detect", [("sparse", False), ("sparse", True), ("dense", None), ("auto", None)])
def test_records_clean_input(mode, group_detect):
    _need_gpu()
    fs, nperseg = 2048000, 256
    B = 600 * nperseg
    iq = _streams(5, 2 * B, fs, nperseg, "hamming", seed=7, pulses=8, dur_ms=(9, 14))
    _check_records(_split(iq, 2), fs, nperseg, "hamming", mode, group_detect=group_detect, oracle_kw=dict(signal_min_duration_ms=5))


def _floor_batch(S, B, fs, nperseg, floor_dbw, seed, nb=2):
    sigma = float(np.sqrt(10.0 ** (floor_dbw / 10.0) * fs / 2.0))
    w = oracle.window_coefficients("hamming", nperseg)
    out = []
    for s in range(S):
        rng = np.random.default_rng([seed, s])
        p = synth.random_pulses(rng, nb * B, fs, w, 6 * nb, dur_ms=(15, 15), peak_dbw=(floor_dbw + 20, floor_dbw + 34))
        p.append(synth.Pulse(B - int(0.005 * fs) - 11 * s, int(0.015 * fs), (0.05 + 0.04 * s) * fs, synth.amp_for_peak_dbw(floor_dbw + 34, w, fs)))
        out.append(synth.make_stream(synth.StreamSpec(nb * B, fs, p, noise_sigma=sigma), seed=900 + s))
    return _split(np.stack(out), nb)


def test_records_prefilter_under_a_noise_floor():
    _need_gpu()
    fs, nperseg = 2048000, 256
    bufs = _floor_batch(4, 1500 * nperseg, fs, nperseg, -160.0, 160)
    _check_records(bufs, fs, nperseg, "hamming", "prefilter", oracle_kw=dict(signal_threshold_dbw=-160.0),
                   expect=lambda infos, n_neg: all(m == _native.RT_MODE_PREFILTER for m, _, _ in infos))


@pytest.mark.parametrize("group_detect", [False, True])
def test_records_runfilter_under_a_noise_floor(group_detect):
    _need_gpu()
    fs, nperseg = 2048000, 256
    bufs = _floor_batch(4, 1000 * nperseg + 24, fs, nperseg, -90.0, 90)
    _check_records(bufs, fs, nperseg, "hamming", "runfilter", group_detect=group_detect,
                   expect=lambda infos, n_neg: all(m == _native.RT_MODE_RUNFILTER for m, _, _ in infos) and n_neg >= 0)


@pytest.mark.parametrize("lanes", [1, 2])
def test_records_auto_with_a_partial_dense_rerun(lanes):
    """Two noisy streams of twelve overflow their candidate lists: AUTO re-runs them alone on the dense path."""
    _need_gpu()
    fs, nperseg, B, S = 300000, 256, 256 * 700, 12
    w = oracle.window_coefficients("hamming", nperseg)
    noisy = {3, 10}
    iq = []
    for s in range(S):
        rng = np.random.default_rng([44, s])
        p = synth.random_pulses(rng, 2 * B, fs, w, 6, peak_dbw=(-80.0, -62.0))
        p.append(synth.Pulse(B - int(0.006 * fs), int(0.015 * fs), (0.1 + 0.02 * s) * fs, synth.amp_for_peak_dbw(-66.0, w, fs)))
        sigma = float(np.sqrt(10 ** (-88.0 / 10) * fs / 2)) if s in noisy else synth.NOISE_SIGMA
        iq.append(synth.make_stream(synth.StreamSpec(2 * B, fs, p, noise_sigma=sigma), seed=700 + s))

    def expect(infos, n_neg):
        assert all(nd == len(noisy) for _, _, nd in infos), infos

    _check_records(_split(np.stack(iq), 2), fs, nperseg, "hamming", "auto", streams=(0, 3, 10, 11), lanes=lanes,
                   record_capacity=2048, expect=expect)


def test_records_at_config2_geometry():
    """T = 8 000 segments, 16 streams, AUTO (which stays sparse): the first, a middle and the last stream in full."""
    _need_gpu()
    fs, nperseg, S = 2048000, 256, 16
    B = 8000 * nperseg
    iq = _streams(S, B, fs, nperseg, "hamming", seed=2, pulses=8, dur_ms=(15, 15))
    _check_records(iq.reshape(S, 1, B), fs, nperseg, "hamming", "auto", streams=(0, 8, 15), lanes=2)


@pytest.mark.parametrize("mode", ["sparse", "dense"])
def test_records_short_buffers_with_look_back(mode):
    """Three consecutive buffers of 23 segments each (not a multiple of 32), pulses across their boundaries."""
    _need_gpu()
    fs, nperseg, T = 300000, 256, 23
    B = T * nperseg
    w = oracle.window_coefficients("hamming", nperseg)
    iq = []
    for s in range(4):
        p = [synth.Pulse(B - 6 * nperseg + 50 * s, 9 * nperseg, (0.1 + 0.05 * s) * fs, synth.amp_for_peak_dbw(-70.0, w, fs)),
             synth.Pulse(2 * B - 3 * nperseg, 7 * nperseg, (-0.2 + 0.05 * s) * fs, synth.amp_for_peak_dbw(-64.0, w, fs)),
             synth.Pulse(5 * nperseg, 4 * nperseg, 0.3 * fs, synth.amp_for_peak_dbw(-75.0, w, fs))]
        iq.append(synth.make_stream(synth.StreamSpec(3 * B, fs, p), seed=40 + s))
    n_rec, n_neg = _check_records(_split(np.stack(iq), 3), fs, nperseg, "hamming", mode, oracle_kw=dict(signal_min_duration_ms=2))
    assert n_neg > 0


_SIZE_CASES = [(32, "sparse"), (64, "sparse"), (128, "sparse"), (512, "sparse"), (1024, "sparse"), (2048, "sparse"), (4096, "sparse"),
               (8192, "sparse"), (16384, "auto"), (8, "auto"), (16, "auto"), (300, "auto"), (1000, "auto"), (4097, "auto")]


@pytest.mark.parametrize("nperseg,mode", _SIZE_CASES)
def test_records_every_size_family(nperseg, mode):
    _need_gpu()
    fs = 2048000
    T = int(np.clip(300000 // nperseg, 30, 400))
    B = T * nperseg
    hop_ms = 1e3 * nperseg / fs
    iq = _streams(3, 2 * B, fs, nperseg, "hann", seed=nperseg + 3, pulses=5, dur_ms=(max(1.0, 4 * hop_ms), max(2.0, 9 * hop_ms)))
    _check_records(_split(iq, 2), fs, nperseg, "hann", mode,
                   oracle_kw=dict(signal_min_duration_ms=min(8.0, 2.5 * hop_ms), signal_max_duration_ms=1e3 * T * hop_ms))


@pytest.mark.parametrize("nperseg,mode", [(256, "sparse"), (300, "auto")])
def test_records_uint8_wire_format(nperseg, mode):
    _need_gpu()
    fs = 2048000
    B = 400 * nperseg
    iq = _streams(3, 2 * B, fs, nperseg, "hamming", seed=8, pulses=6, peak=(-50.0, -40.0), dur_ms=(8, 12), sigma=0.012)
    raw = synth.quantize_u8(iq).reshape(3, 2, 2 * B)
    _check_records(raw, fs, nperseg, "hamming", mode, u8=True, oracle_kw=dict(signal_min_duration_ms=4))


def test_records_dc_over_the_guard_meet_the_subtract_first_bound():
    """A default handle; stream 1 carries an offset 80 dB over its noise (over the guard's 60 dB): from the guard on it is
    detrended in SciPy's order and must meet the subtract-first bound, every other stream the linearity bound."""
    _need_gpu()
    fs, nperseg = 2048000, 256
    B = 600 * nperseg
    iq = _streams(3, 2 * B, fs, nperseg, "hamming", seed=17, pulses=6, dur_ms=(9, 14), peak=(-60.0, -40.0),
                  dc=[0j, complex(0.1, -0.07), complex(1e-3, 0)])
    _check_records(_split(iq, 2), fs, nperseg, "hamming", "sparse", sub_streams=(1,), oracle_kw=dict(signal_min_duration_ms=5))


def test_zz_print_worst_ratios():
    """The worst |gpu - f64| / bound per family and field over the tests above (``-s`` shows it)."""
    for (fam, what), v in sorted(WORST.items()):
        print(f"gpu-f64 {fam:16s} {what:22s} {v:.3f}")
    assert all(v <= 1.0 for v in WORST.values())
