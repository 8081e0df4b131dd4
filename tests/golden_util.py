"""Loading helpers for tests/golden/*.npz (data written by make_golden.py)."""
import datetime
import hashlib
import json
import os

import numpy as np

from pyradiotracking_amd import synth

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TS0 = datetime.datetime(2024, 1, 1, 0, 0, 0)
TS0_UTC = TS0.replace(tzinfo=datetime.timezone.utc)

_cache = {}


def _npz(name):
    if name not in _cache:
        _cache[name] = np.load(os.path.join(GOLDEN_DIR, name), allow_pickle=False)
    return _cache[name]


def iq_index():
    return json.loads(str(_npz("iq_cases.npz")["index_json"]))


def iq_case_names():
    return [m["name"] for m in iq_index()]


def iq_case(name):
    """-> (meta, buffers, ts_starts, expected) with expected[b] = dict(table, kept, reprs, rows?)."""
    z = _npz("iq_cases.npz")
    meta = next(m for m in iq_index() if m["name"] == name)
    sp = meta["spec"]
    spec = synth.StreamSpec(
        n_samples=sp["n_samples"],
        sample_rate=sp["sample_rate"],
        pulses=[synth.Pulse(int(a), int(b), float(c), float(d), float(e)) for a, b, c, d, e in sp["pulses"]],
        noise_sigma=sp.get("noise_sigma", synth.NOISE_SIGMA),
        dc=complex(*sp["dc"]) if "dc" in sp else 0j,
    )
    iq = synth.make_stream(spec, meta["seed"])
    digest = hashlib.sha256(iq.tobytes()).hexdigest()
    assert digest == meta["iq_sha256"], f"regenerated IQ of {name} differs from the pinned bytes"
    blen = meta["buffer_len"]
    buffers = [iq[i * blen : (i + 1) * blen] for i in range(meta["n_buffers"])]
    ts_starts = [TS0 + datetime.timedelta(microseconds=o) for o in meta["ts_offsets_us"]]
    expected = []
    for b in range(meta["n_buffers"]):
        e = dict(
            table=z[f"{name}/b{b}/table"],
            kept=z[f"{name}/b{b}/kept"],
            reprs=[str(s) for s in z[f"{name}/b{b}/reprs"]],
            spec_shape=tuple(z[f"{name}/b{b}/spec_shape"]),
            row_means=z[f"{name}/b{b}/row_means"],
        )
        if f"{name}/b{b}/rows" in z:
            e["rows"] = z[f"{name}/b{b}/rows"]
        expected.append(e)
    kwargs = dict(meta["kwargs"])
    if isinstance(kwargs.get("fft_window"), list):
        w = kwargs["fft_window"]
        kwargs["fft_window"] = tuple(w) if isinstance(w[0], str) else np.asarray(w, dtype=np.float64)
    return meta, kwargs, buffers, ts_starts, expected


def extract_index():
    return json.loads(str(_npz("extract_cases.npz")["index_json"]))


def extract_case(i):
    z = _npz("extract_cases.npz")
    meta = extract_index()[i]
    d = {k: z[f"c{i}/{k}"] for k in ("cur", "last", "freqs", "times", "table", "kept")}
    d["kwargs"] = meta["kwargs"]
    d["has_last"] = meta["has_last"]
    return d


def us(delta: datetime.timedelta) -> int:
    return delta.days * 86400 * 1000000 + delta.seconds * 1000000 + delta.microseconds


def signals_table(signals, ts_start_utc):
    """Same 8 columns as make_golden.signals_to_table, from any objects with
    ts/frequency/duration/max/avg/std/noise/snr attributes."""
    tab = np.zeros((len(signals), 8), dtype=np.float64)
    for i, s in enumerate(signals):
        tab[i] = [us(s.ts - ts_start_utc), s.frequency, us(s.duration), s.max, s.avg, s.std, s.noise, s.snr]
    return tab


# ---------------------------------------------------------------------------
# Inputs of the checks against the reference's own outputs (reference_cases.npz, written by
# make_golden_reference.py from exactly these builders: the tests regenerate the inputs and compare
# with the stored outputs)
# ---------------------------------------------------------------------------
def reference_stream_case(seed):
    """Random geometry and pulses, three consecutive buffers of one stream -> (buffers, ts_starts, kwargs)."""
    import scipy.signal

    rng = np.random.default_rng(1000 + seed)
    nperseg = int(rng.choice([256, 256, 1024]))
    fs = int(rng.choice([300000, 1000000, 2048000]))
    wname = str(rng.choice(["hamming", "hann"]))
    w = scipy.signal.get_window(wname, nperseg)
    blen = int(rng.integers(120, 400)) * nperseg + int(rng.integers(0, nperseg))
    nbuf = 3
    pulses = synth.random_pulses(rng, nbuf * blen, fs, w, 10, dur_ms=(6, 45), peak_dbw=(-88, -60))
    iq = synth.make_stream(synth.StreamSpec(nbuf * blen, fs, pulses, dc=complex(1e-3, 5e-4) * (seed % 2)), seed)
    bufs = [iq[i * blen : (i + 1) * blen] for i in range(nbuf)]
    tss = [TS0 + datetime.timedelta(seconds=i * blen / fs) for i in range(nbuf)]
    return bufs, tss, dict(sample_rate=fs, fft_nperseg=nperseg, fft_window=wname)


def reference_noise_floor_case(floor_db):
    """The reference's default geometry and thresholds with the noise floor `floor_db` over the -90 dBW threshold,
    two consecutive buffers -> (buffers, ts_starts, kwargs)."""
    import scipy.signal

    fs, nperseg, thr_dbw = 300000, 256, -90.0
    rng = np.random.default_rng(int(100 + floor_db))
    w = scipy.signal.get_window("hamming", nperseg)
    blen = 330 * nperseg + 17
    nbuf = 2
    sigma = float(np.sqrt(10.0 ** ((thr_dbw + floor_db) / 10.0) * fs / 2.0))  # PSD per bin = 2 sigma^2 / fs
    pulses = synth.random_pulses(rng, nbuf * blen, fs, w, 8, dur_ms=(9, 30), peak_dbw=(thr_dbw + floor_db + 14, thr_dbw + floor_db + 30))
    pulses.append(synth.Pulse(blen - int(0.006 * fs), int(0.015 * fs), 0.11 * fs, synth.amp_for_peak_dbw(thr_dbw + floor_db + 24, w, fs)))  # across the boundary
    iq = synth.make_stream(synth.StreamSpec(nbuf * blen, fs, pulses, noise_sigma=sigma), 7)
    bufs = [iq[i * blen : (i + 1) * blen] for i in range(nbuf)]
    tss = [TS0 + datetime.timedelta(seconds=i * blen / fs) for i in range(nbuf)]
    return bufs, tss, dict(sample_rate=fs, fft_nperseg=nperseg)


def iq_sha256(buffers):
    return hashlib.sha256(b"".join(np.ascontiguousarray(b).tobytes() for b in buffers)).hexdigest()


def spec_sha256(spec):
    """digest of a spectrogram's values (float64, -0.0 folded into 0.0): equal digests <=> np.array_equal"""
    return hashlib.sha256(np.ascontiguousarray(np.asarray(spec, dtype=np.float64) + 0.0).tobytes()).hexdigest()


def matcher_trials():
    """Six random matcher runs -> [(devices, params, signals)], signals = [(device, ts_us, frequency, duration_us, avg)]."""
    rng = np.random.default_rng(11)
    out = []
    for trial in range(6):
        n_dev = int(rng.integers(2, 6))
        devices = [str(i) for i in range(n_dev)]
        params = dict(matching_timeout_s=float(rng.uniform(0.2, 3)), matching_time_diff_s=float(rng.uniform(0, 0.05)),
                      matching_bandwidth_hz=float(rng.uniform(0, 5000)),
                      matching_duration_diff_ms=[None, 2.0, 5.5][trial % 3])
        signals = []
        t = 1_700_000_000_000_000
        for _ in range(400):
            t += int(rng.integers(0, 200_000))
            dev = devices[int(rng.integers(0, n_dev))]
            freq = 150e6 + float(rng.integers(0, 8)) * 1500.0 + float(rng.uniform(-5, 5))
            dur = int(rng.integers(8000, 30000))
            avg = float(rng.uniform(-80, -40))
            signals.append((dev, t + int(rng.integers(-3000, 3000)), freq, dur, avg))
        out.append((devices, params, signals))
    return out


def matched_groups_arrays(groups, n_dev, ts_to_us):
    """[(ts, frequency, duration, avgs)] of `n_dev` devices -> dict of arrays (avgs: NaN where a device is absent, with a
    presence mask)"""
    avgs = np.full((len(groups), n_dev), np.nan)
    present = np.zeros((len(groups), n_dev), dtype=bool)
    for i, g in enumerate(groups):
        for j, a in enumerate(g[3]):
            if a is not None:
                avgs[i, j], present[i, j] = a, True
    return dict(ts_us=np.array([ts_to_us(g[0]) for g in groups], dtype=np.int64),
                frequency=np.array([g[1] for g in groups], dtype=np.float64),
                duration_us=np.array([us(g[2]) for g in groups], dtype=np.int64),
                avgs=avgs, present=present)


def reference_cases():
    return _npz("reference_cases.npz")
