"""Per-record band spectrum reduced on the device (rt_fetch_record_spectrum) on the GPU.  Against the frames of the same analyzer
(``fetch_record_band(k, w)``) the means, the peaks, ``total``, ``n_inside`` and ``peak_col`` are the bytes of the NumPy restatement of
the kernel's order (tests/record_spectrum_cases.py; a NaN equals a NaN), and every field lies within the derived round-off bounds
of ``record_band_rows``, which defines the result, with the same NaN pattern.  The bytes are held to themselves across handle
kinds, fetches and orders of calls.

A record at bin 0 does not exist -- every segment's mean is removed -- so the bands that wrap are those of the records at the
bins 1 ... 8 and N - 8 ... N - 1 of tests/record_band_cases.py's twin call around bin N - 1.

Worst |row - model| / bound per case as seen on an MI355X: profiles/record_spectrum_worst_ratio.txt (``RT_WRITE_PROFILES=1``
rewrites its gpu half)."""
import ctypes as C
import datetime
import os

import numpy as np
import pytest

from pyradiotracking_amd import _native
from pyradiotracking_amd.analyze import BatchSignalAnalyzer, SignalAnalyzer, record_band_rows, spectrum_hz
from tests import record_band_cases as bc
from tests import record_estimates_cases as ec
from tests import record_spectrum_cases as sc
from tests import record_stft_cases as rs
from tests import sequence_cases as sq

pytestmark = pytest.mark.gpu

SCHED = rs.GPU_SCHEDULE
S = rs.GPU_S
N_CALLS = len(SCHED.T)
WORST = {}
WIDTHS = (0, 1, 2, 3, 8)


@pytest.fixture(autouse=True)
def _need_gpu():
    if _native.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")


def _handle(nperseg, fmt, margin, n_streams=S, **extra):
    if fmt == "c128":
        extra["precision"] = "float64"
    kw = sq.case_settings(nperseg, fmt)
    kw.update(extra)
    if margin is not None:
        kw.update(record_iq=True, record_iq_margin=margin)
    return BatchSignalAnalyzer([str(i) for i in range(n_streams)], sdr_callback_length=sq.max_samples(SCHED, nperseg), **kw)


def _run(nperseg, fmt, margin, after, feed=None, calls=N_CALLS, **extra):
    b = _handle(nperseg, fmt, margin, **extra)
    try:
        for c in range(calls):
            sq.enqueue(b, rs.gpu_feed(nperseg, c, fmt) if feed is None else feed(c), fmt)
            after(b, c, b.fetch_records())
    finally:
        b.close()


def _held(name, b, rec, N, k, w):
    """the entry's triple for (k, w) against the restatement (bytes) and the model (bounds) on the same handle's band"""
    off, first, values = b.fetch_record_band(k, w)
    got = b.fetch_record_spectrum(k, w)
    rows, mean, peak = got
    assert rows.dtype == _native.SPECTRUM_DTYPE and rows.shape == (len(rec),) and mean.shape == peak.shape == (len(rec), 2 * w + 1)
    assert mean.dtype == peak.dtype == np.float64
    want = sc.restate(off, first, values, rec["start"], rec["end"], N, k)
    assert sc.same_bytes(got, want) == [], (name, k, w, sc.same_bytes(got, want))
    for f in sc.SCALARS:  # the other scalars: the restatement's NaN pattern
        assert np.array_equal(np.isnan(rows[f]), np.isnan(want[0][f])), (name, k, w, f)
    worst, left_out, bad = sc.compare(got, sc.model(off, first, values, rec["start"], rec["end"], N, k))
    assert not bad, (name, k, w, bad[:3])
    acc = WORST.setdefault(name, dict.fromkeys(worst, 0.0))
    for f, v in worst.items():
        acc[f] = max(acc[f], v)
    return got, (off, first, values), left_out


# ---- 1: every row against the restatement and the model --------------------------------------------------------------------------------
SHAPES = [(32, "c64"), (256, "u8"), (256, "i16"), (64, "i8"), (300, "c64"), (256, "c128")]


@pytest.mark.parametrize("margin", [0, 2])
@pytest.mark.parametrize("nperseg,fmt", SHAPES, ids=lambda v: str(v))
def test_every_row_against_the_restatement_and_the_model(nperseg, fmt, margin):
    """k in {1, 4} crossed with every w of WIDTHS, on every call of the GPU suite's schedule"""
    seen = dict(records=0, inside=0, two_parts=0, left_out=0, peak_bins=0)

    def after(b, c, rec):
        for k in (1, 4):
            for w in WIDTHS:
                (rows, mean, peak), (off, first, values), out = _held(f"{nperseg} {fmt} margin {margin}", b, rec, nperseg, k, w)
                seen["records"] += len(rows)
                seen["inside"] += int(rows["n_inside"].sum())
                seen["left_out"] += out
                seen["peak_bins"] += int(np.isfinite(rows["peak_bins"]).sum())
                runs = sc.plan_of(off, first, rec["start"], rec["end"], nperseg, k)
                seen["two_parts"] += int(((runs[:, 1] > runs[:, 0]) & (runs[:, 3] > runs[:, 2])).sum())
                if w == 0 and len(rows):
                    has = rows["n_inside"] > 0
                    assert np.isnan(rows["peak_bins"]).all() and (rows["peak_col"][has] == 0).all()

    _run(nperseg, fmt, margin, after)
    print(f"record_spectrum nperseg {nperseg} {fmt} margin {margin}: {seen}")
    assert seen["records"] > 100 and seen["inside"] > seen["records"] and seen["two_parts"] > 0 and seen["peak_bins"] > 0, seen
    assert seen["left_out"] <= seen["records"] // 4, seen


@pytest.mark.parametrize("N,k,w", [(8, 1, 3), (8, 4, 3), (32, 16, 2), (32, 16, 8)])
def test_the_smallest_nperseg_and_the_finest_hop(N, k, w):
    pulses = [(3, 10, 5), (N - 1, 20, 9), (1, 0, 3), (N // 2, 30, SMALL_LONG)]
    b = BatchSignalAnalyzer([str(i) for i in range(len(pulses))], sdr_callback_length=sc.SMALL_T * N, lanes=1, record_iq=True, record_iq_margin=2,
                            **sc.small_settings(N))
    try:
        for c in range(2):
            b.enqueue(sc.small_feed(N, pulses, seed=c))
            rec = b.fetch_records()
            assert len(rec) >= len(pulses)
            (rows, mean, peak), _, _ = _held(f"small N={N}", b, rec, N, k, w)
            assert (rows["n_inside"] > 0).all() and (rows["peak_col"] == w).all()  # bin-centred tones under a boxcar
            if k == 1:  # every inside frame is all tone or all noise: the neighbours hold noise alone (a frame at a finer hop straddles the switch)
                assert (rows["centre_share"] > 0.99).all()
    finally:
        b.close()


SMALL_LONG = 12


# ---- 2: size edges -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("margin", [0, 2])
def test_size_edges(margin):
    """tests/record_estimates_cases.py's boxcar pulses at nperseg 32: 1, 2, 3, 63, 64, 65, 127, 128, 129 inside frames at k = 1 -- the
    lane count and the one- and two-round limits of the partials -- and the record of 1 105 frames at k = 16; call 2 holds a record
    that began in the previous buffer, whose inside frames come from both parts"""
    b = BatchSignalAnalyzer([str(i) for i in range(ec.EDGE_S)], sdr_callback_length=ec.EDGE_T * ec.EDGE_N, lanes=1, record_iq=True, record_iq_margin=margin,
                            **ec.edge_settings())
    N = ec.EDGE_N
    try:
        for c in range(ec.EDGE_CALLS):
            b.enqueue(ec.edge_feed(c))
            rec = b.fetch_records()
            for w in (0, 2, 8):
                (rows, mean, peak), (off, first, values), _ = _held(f"size edges margin {margin}", b, rec, N, 1, w)
                if c == 0:
                    assert rows["n_inside"].tolist() == list(ec.EDGE_INSIDE) + [ec.EDGE_LONG]
                else:
                    i = len(rec) - 1
                    assert (int(rec["start"][i]), int(rec["end"][i])) == (-6, 4) and first[i] <= -6 and rows["n_inside"][i] == 10
                    runs = sc.plan_of(off, first, rec["start"], rec["end"], N, 1)[i]
                    assert runs[1] - runs[0] == 6 and runs[3] - runs[2] == 4  # both parts
            if c == 0:
                (rows, _, _), (off, _, _), _ = _held(f"size edges margin {margin}", b, rec, N, 16, 2)
                assert rows["n_inside"][-1] == 1105 and (np.diff(off)[-1] == 1105) == (margin == 0)
    finally:
        b.close()


# ---- 3: bands that wrap --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,fmt", [(32, "u8"), (256, "c64")], ids=lambda v: str(v))
def test_bands_that_wrap_round_the_circle(N, fmt):
    """the twin call around bin N - 1: records at the bins N - 8 ... N - 1 and 1 ... 7 of one stream, all of one span"""
    T, _, _ = bc.twin_layout(N)
    fi = N - 1
    b = BatchSignalAnalyzer([str(i) for i in range(S)], sdr_callback_length=T * N, record_iq=True, record_iq_margin=1, **bc.twin_settings(N))
    try:
        sq.enqueue(b, bc.twin_feed(N, fi, fmt), fmt)
        rec = b.fetch_records()
        bins = set(rec["fi"][rec["stream"] == bc.TWIN_STREAM].tolist())
        assert {1, N - 1} <= bins and 0 not in bins
        for k, w in ((1, 1), (4, 2), (1, 8)):
            (rows, mean, peak), _, _ = _held(f"wrap N={N} {fmt}", b, rec, N, k, w)
            mine = np.flatnonzero(rec["stream"] == bc.TWIN_STREAM)
            at = {int(rec["fi"][i]): i for i in mine}
            # a column d bins off is the centre column of the record d bins away: the same frames, the same means and peaks
            n = 0
            for fa, ia in at.items():
                for d in range(-w, w + 1):
                    ib = at.get((fa + d) % N)
                    if ib is not None:
                        assert mean[ia, w + d].tobytes() == mean[ib, w].tobytes() and peak[ia, w + d].tobytes() == peak[ib, w].tobytes(), (N, k, w, fa, d)
                        n += 1
            assert n > 2 * w * len(at) * 0.8
    finally:
        b.close()


# ---- 4: handle kinds and orders of calls ---------------------------------------------------------------------------------------------
def _by_record(b, rec, k, w):
    got = b.fetch_record_spectrum(k, w)
    again = b.fetch_record_spectrum(k, w)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again))  # a second fetch of the same call copies
    first = b.fetch_record_band(k, w)[1]
    return {(int(r["stream"]), int(r["fi"]), int(r["start"]), int(r["end"]), int(first[i])): got[0][i].tobytes() + got[1][i].tobytes() + got[2][i].tobytes()
            for i, r in enumerate(rec)}


def _hold_common(runs, plain):
    for name in runs:
        if name == plain:
            continue
        common = 0
        for c in range(N_CALLS):
            for key, v in runs[plain][c].items():
                if key in runs[name][c]:
                    assert runs[name][c][key] == v, (name, c, key)
                    common += 1
        assert common >= 0.9 * sum(len(c) for c in runs[plain]) > 20, (name, common)


def test_the_same_samples_give_the_same_bytes_on_every_handle_kind():
    nperseg, margin, k, w = 256, 2, 4, 2
    runs = {}
    for name, extra in (("sparse", dict(mode="sparse")), ("dense", dict(mode="dense")), ("lanes", dict(mode="sparse", lanes=3))):
        got = []
        _run(nperseg, "c64", margin, lambda b, c, rec, got=got: got.append(_by_record(b, rec, k, w)), **extra)
        runs[name] = got
    _hold_common(runs, "sparse")
    runs = {}
    for name, extra in (("dense64", dict()), ("mapfree64", dict(f64_sparse=True))):
        got = []
        _run(nperseg, "c128", margin, lambda b, c, rec, got=got: got.append(_by_record(b, rec, k, w)), **extra)
        runs[name] = got
    _hold_common(runs, "dense64")


def test_a_chained_handle_gives_the_bytes_of_sequential_calls():
    """One recording of four buffers: through a ``chain=4`` handle in one call, and through a plain handle in four."""
    nperseg, margin, links, T, k, w = 256, 2, 4, 24, 4, 2
    half = T // 2 * nperseg
    bufs = []
    for c in range(links):
        x = rs.gpu_buffer(nperseg, c)[rs.NEG_STREAM][:SCHED.T[c] * nperseg]
        bufs.append(np.ascontiguousarray(np.concatenate([x[:half], x[len(x) - half:]])))
    kw = dict(sq.settings(nperseg), mode="sparse", record_iq=True, record_iq_margin=margin)
    seq = {}
    b = BatchSignalAnalyzer(["0"], sdr_callback_length=T * nperseg, **kw)
    try:
        for c, x in enumerate(bufs):
            b.enqueue(x[None, :])
            for key, v in _by_record(b, b.fetch_records(), k, w).items():
                seq[(c,) + key[1:]] = v
    finally:
        b.close()
    ch = BatchSignalAnalyzer(["0"], sdr_callback_length=T * nperseg, chain=links, **kw)
    try:
        ch.enqueue(np.concatenate(bufs)[None, :], links=links)
        chained = _by_record(ch, ch.fetch_records(), k, w)
    finally:
        ch.close()
    common = [key for key in chained if key in seq]
    assert len(common) >= 0.9 * len(seq) > 8 and any(key[4] < 0 for key in common), (len(common), len(seq))
    for key in common:
        assert chained[key] == seq[key], key


def test_the_order_of_calls_does_not_change_the_bytes_and_another_pair_rebuilds():
    nperseg, fmt, margin = 256, "c64", 2
    first_run, n = [], [0]

    def flat(got):
        return b"".join(a.tobytes() for a in got)

    def early(b, c, rec):  # the entry in front of every other record entry
        first_run.append((flat(b.fetch_record_spectrum(4, 2)), b.fetch_record_band(4, 2)[2].tobytes()))

    def late(b, c, rec):  # ... and behind them, twice, and after other pairs and back
        b.fetch_record_stft()
        b.fetch_record_stft(hop_div=4)
        b.fetch_record_estimates(hop_div=4)
        band = b.fetch_record_band(4, 2)[2]
        assert band.tobytes() == first_run[c][1]
        assert flat(b.fetch_record_spectrum(4, 2)) == first_run[c][0] == flat(b.fetch_record_spectrum(4, 2))
        wide = b.fetch_record_spectrum(4, 8)       # another pair builds again ...
        b.fetch_record_band(2, 1)                  # ... the band pool goes to a third pair ...
        other = b.fetch_record_spectrum(1, 2)
        assert flat(b.fetch_record_spectrum(4, 2)) == first_run[c][0]  # ... and the first pair is built once more
        assert b.fetch_record_band(4, 2)[2].tobytes() == first_run[c][1]
        # the columns the pairs share are the same bytes
        narrow = b.fetch_record_spectrum(4, 2)
        assert np.ascontiguousarray(wide[1][:, 6:11]).tobytes() == narrow[1].tobytes() and np.ascontiguousarray(wide[2][:, 6:11]).tobytes() == narrow[2].tobytes()
        assert wide[0]["n_inside"].tolist() == narrow[0]["n_inside"].tolist()
        assert (other[0]["n_inside"] <= narrow[0]["n_inside"]).all()
        n[0] += len(narrow[0])

    _run(nperseg, fmt, margin, early)
    _run(nperseg, fmt, margin, late)
    assert n[0] > 20


def test_products_that_grow_between_two_calls_of_a_slot_give_a_fresh_handles_bytes():
    """A call slot's hop and band pools start at 65536 bytes.  A small call leaves all five entries' products in the slot, at
    different keys for the hop and the band entry; a later call through the same slot (two calls on: a handle has two slots) needs
    more than that floor, so both pools are freed and made again under products that still carry the small call's sizes.  Every
    entry, asked in another order, gives the bytes of a handle that has only ever seen the large call."""
    from tests import detect_order_cases as doc

    N, T, margin, n_streams = 32, 400, 2, 12
    small = [[(3, 10, 5)], [(N - 1, 20, 9)], [(1, 30, 3)], [(N // 2, 40, 12)]] + [[]] * 8  # per stream: (bin, first segment, segments)
    # (clear of the buffer's start: no look-back; an eighth of the buffer: the row means stay the noise's)
    large = [[(3 + s, 5 + s, 48)] for s in range(n_streams)]

    def feed(pulses, seed):
        return np.stack([doc.plant(N, T, [(f, t0, r, doc.TONE_DBW) for f, t0, r in p], seed=1000 * seed + s) for s, p in enumerate(pulses)])

    def handle():
        return BatchSignalAnalyzer([str(i) for i in range(n_streams)], sdr_callback_length=T * N, lanes=1, record_iq=True, record_iq_margin=margin,
                                   **sc.small_settings(N))

    def flat(got):
        return b"".join(np.ascontiguousarray(a).tobytes() for a in (got if isinstance(got, tuple) else (got,)))

    entries = dict(stft=lambda b: b.fetch_record_stft(), hop=lambda b: b.fetch_record_stft(hop_div=16), band=lambda b: b.fetch_record_band(4, 2),
                   est=lambda b: b.fetch_record_estimates(hop_div=16), spec=lambda b: b.fetch_record_spectrum(4, 2))
    key = ("stream", "fi", "start", "end")
    b, twin = handle(), handle()
    try:
        b.enqueue(feed(small, 0))
        assert len(b.fetch_records()) >= 4
        got ={name: entries[name](b) for name in ("stft", "hop", "band", "est", "spec")}
        assert 0 < got["hop"][2].nbytes <= 65536 and 0 < got["band"][2].nbytes <= 65536, (got["hop"][2].shape, got["band"][2].shape)
        b.enqueue(feed(small, 1))  # the handle's other slot
        b.fetch_records()
        b.enqueue(feed(large, 2))  # ... and the first one again
        rec = b.fetch_records()
        got = {name: entries[name](b) for name in ("spec", "est", "band", "hop", "stft")}
        twin.enqueue(feed(large, 2))
        rec_twin = twin.fetch_records()
        want = {name: entries[name](twin) for name in ("stft", "hop", "band", "est", "spec")}
        assert len(rec) >= n_streams and all(rec[f].tolist() == rec_twin[f].tolist() for f in key)
        # frames x 8 bytes (complex64) of the hop entry, x 5 columns of the band entry: past the floor, so both pools grew
        assert want["hop"][2].dtype == want["band"][2].dtype == np.complex64
        assert want["hop"][2].nbytes > 65536 and want["band"][2].nbytes > 65536 and want["band"][2].shape[1] == 5
        for name in want:
            assert flat(got[name]) == flat(want[name]), name
        assert len(got["est"]) == len(got["spec"][0]) == len(rec)
    finally:
        b.close()
        twin.close()


# ---- 5: a constant segment, a NaN sample ---------------------------------------------------------------------------------------------
CONST_VALUE = np.complex64(complex(np.float32(0.3), np.float32(-0.7)))  # a full-mantissa constant


def test_a_constant_segment_inside_a_record_is_exactly_zero_in_every_column():
    """A record's cells are its pulse's and the cold cell before it.  With that cell's segment made one value, the record of one
    pulse segment has two inside frames at k = 1, one of them exactly 0 in every column: every mean is exactly half the peak.
    NOT COVERED, because it cannot occur: a record whose inside frames are ALL constant.  A constant segment has no power, the
    detection puts no record on it, and every record holds a cell over the threshold; the row of total == 0 with its NaN quotients
    is held on the restatement and the model (tests/test_record_spectrum_contract.py: zero frames)."""
    N = ec.EDGE_N
    b = BatchSignalAnalyzer([str(i) for i in range(ec.EDGE_S)], sdr_callback_length=ec.EDGE_T * N, lanes=1, record_iq=True, record_iq_margin=0,
                            **ec.edge_settings())
    try:
        x = ec.edge_feed(0).copy()
        x[1, 9 * N:10 * N] = CONST_VALUE  # stream 1: the pulse is segment 10, the cold cell before it segment 9
        b.enqueue(x)
        rec = b.fetch_records()
        i = int(np.flatnonzero(rec["stream"] == 1)[0])
        assert (int(rec["start"][i]), int(rec["end"][i])) == (9, 11)
        for w in (0, 2, 8):
            off, first, values = b.fetch_record_band(1, w)
            frames = values[off[i]:off[i + 1]]
            assert len(frames) == 2 and (frames[0] == 0).all() and (np.abs(frames[1][w]) > 0)
            (rows, mean, peak), _, _ = _held("constant segment", b, rec, N, 1, w)
            assert rows["n_inside"][i] == 2 and np.array_equal(mean[i], peak[i] / 2.0) and rows["peak_col"][i] == w
    finally:
        b.close()


def test_a_nan_sample_inside_a_record_and_its_clean_twin():
    nperseg, fmt, margin, k, w = 256, "c64", 2, 4, 2
    t_nan = 10  # inside call 1's planted pulse (segments 6 ... 16) of the stream with the negative-frequency bin
    seen = dict(nan=0, same=0)
    sides = {}
    for dirty in (False, True):
        got = []

        def feed(c, dirty=dirty):
            x = rs.gpu_feed(nperseg, c, fmt).copy()
            if dirty and c == 1:
                x[rs.NEG_STREAM, t_nan * nperseg + 5] = np.nan
            return x

        def after(b, c, rec, got=got):
            (rows, mean, peak), (off, first, values), _ = _held(f"NaN sample dirty={dirty}", b, rec, nperseg, k, w)
            per = {}
            for i, r in enumerate(rec):
                hit = bool(np.isnan(mean[i]).any() and rows["n_inside"][i] > 0)
                if hit:  # ... then every column, every scalar
                    assert np.isnan(mean[i]).all() and np.isnan(peak[i]).all() and rows["peak_col"][i] == -1 and all(np.isnan(rows[f][i]) for f in sc.SCALARS)
                    assert int(r["stream"]) == rs.NEG_STREAM and dirty and c == 1
                per[(int(r["stream"]), int(r["fi"]), int(r["start"]), int(r["end"]), int(first[i]))] = (hit, rows[i].tobytes() + mean[i].tobytes() + peak[i].tobytes())
            got.append(per)

        _run(nperseg, fmt, margin, after, feed=feed)
        sides[dirty] = got
    for c in range(N_CALLS):
        for key, (hit, data) in sides[True][c].items():
            seen["nan"] += int(hit)
            if not hit and key in sides[False][c]:  # every other record is the clean twin's, byte for byte
                assert data == sides[False][c][key][1], (c, key)
                seen["same"] += 1
    assert seen["nan"] >= 1 and seen["same"] > 20, seen


# ---- 6: refusals, the size query ---------------------------------------------------------------------------------------------------
def _fetch_spec(b, k, w, cap=None, mean=True, peak=True):
    lib, h = b.native._lib, b.native._handle
    n = C.c_size_t(0)
    rc = lib.rt_fetch_record_spectrum(h, k, w, None, None, None, 0, C.byref(n))
    if rc != _native.RT_OK or cap is None:
        return rc, n.value, None
    B = 2 * w + 1
    rows = np.full(max(cap, 1) * 6, 7.5, np.float64)
    m = np.full(max(cap, 1) * B, 7.5, np.float64)
    p = np.full(max(cap, 1) * B, 7.5, np.float64)
    rc = lib.rt_fetch_record_spectrum(h, k, w, rows.ctypes.data, m.ctypes.data if mean else None, p.ctypes.data if peak else None, cap, C.byref(n))
    return rc, n.value, (rows, m, p)


def _err(b):
    return b.native._lib.rt_last_error(b.native._handle).decode()


def test_refusals_and_the_size_query():
    nperseg, fmt, k, w = 256, "c64", 4, 2
    B = 2 * w + 1
    name = "rt_fetch_record_spectrum"
    feeds = [rs.gpu_feed(nperseg, c, fmt) for c in range(N_CALLS)]
    off_handle = _handle(nperseg, fmt, None)
    b = _handle(nperseg, fmt, 0)
    twin = _handle(nperseg, fmt, 0)
    small = BatchSignalAnalyzer(["0"], sdr_callback_length=40 * 8, record_iq=True, **sq.settings(8))
    lib = b.native._lib

    def both(x):
        b.enqueue(x)
        twin.enqueue(x)

    def same():
        rec, want = b.fetch_records(), twin.fetch_records()
        assert rec.tobytes() == want.tobytes()  # after every refusal the handle analyses on as its twin does
        return rec

    def good(n_rec):
        """the next valid call returns the bytes it would have returned: the twin's, which was never refused"""
        got, want = b.fetch_record_spectrum(k, w), twin.fetch_record_spectrum(k, w)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, want)) and len(got[0]) == n_rec

    try:
        # feature off
        off_handle.enqueue(feeds[0])
        off_handle.fetch_records()
        with pytest.raises(_native.NativeError) as ei:
            off_handle.fetch_record_spectrum(k, w)
        assert ei.value.code == _native.RT_E_INVALID and name + ": rt_set_record_iq" in str(ei.value)
        # no delivered call yet
        assert _fetch_spec(b, k, w)[0] == _native.RT_E_INVALID and _err(b).startswith(name + ": no samples")
        both(feeds[0])
        same()
        both(feeds[1])
        rec = same()
        n_rec = len(rec)
        assert n_rec > 0
        # a null n_out
        h = b.native._handle
        assert lib.rt_fetch_record_spectrum(h, k, w, None, None, None, 0, None) == _native.RT_E_INVALID
        good(n_rec)
        # k no divisor of nperseg in 1 .. 16, w outside 0 .. 8: refused, the message names k, w and N, nothing written
        for bad_k, bad_w in ((0, 2), (17, 2), (3, 2), (-4, 2), (4, -1), (4, 9), (1, 100)):
            rc, _, _ = _fetch_spec(b, bad_k, bad_w)
            e = _err(b)
            assert rc == _native.RT_E_INVALID and f"k = {bad_k}" in e and f"w = {bad_w}" in e and f"N = {nperseg}" in e and e.startswith(name + ":"), e
            with pytest.raises(_native.NativeError):
                b.fetch_record_spectrum(bad_k, bad_w)
            good(n_rec)
        # 2 w + 1 > nperseg: N = 8 with w = 4
        small.enqueue(np.zeros((1, 40 * 8), np.complex64))
        assert len(small.fetch_records()) == 0
        assert _fetch_spec(small, 1, 4)[0] == _native.RT_E_INVALID and "w = 4" in _err(small) and "N = 8" in _err(small)
        assert _fetch_spec(small, 1, 3)[:2] == (_native.RT_OK, 0)
        # size query, then fetch; cap one short writes nothing; a larger cap leaves the rest alone; NULL mean or peak: not wanted
        rc, n, _ = _fetch_spec(b, k, w)
        assert rc == _native.RT_OK and n == n_rec
        rc, _, bufs = _fetch_spec(b, k, w, n_rec - 1)
        assert rc == _native.RT_E_CAPACITY and all(np.all(x == 7.5) for x in bufs) and _err(b).startswith(name + ":")
        good(n_rec)
        want = b.fetch_record_spectrum(k, w)
        rc, n, (rows, m, p) = _fetch_spec(b, k, w, n_rec + 3)
        assert rc == _native.RT_OK and n == n_rec
        assert rows[:6 * n_rec].tobytes() == want[0].tobytes() and m[:B * n_rec].tobytes() == want[1].tobytes() and p[:B * n_rec].tobytes() == want[2].tobytes()
        assert np.all(rows[6 * n_rec:] == 7.5) and np.all(m[B * n_rec:] == 7.5) and np.all(p[B * n_rec:] == 7.5)
        rc, n, (rows, m, p) = _fetch_spec(b, k, w, n_rec, mean=False)
        assert rc == _native.RT_OK and np.all(m == 7.5) and p.tobytes() == want[2].tobytes() and rows.tobytes() == want[0].tobytes()
        rc, n, (rows, m, p) = _fetch_spec(b, k, w, n_rec, peak=False)
        assert rc == _native.RT_OK and np.all(p == 7.5) and m.tobytes() == want[1].tobytes()
        # after the next enqueue; with two in flight: process c, process c + 1, fetch c, then the rows of c
        both(feeds[2])
        assert _fetch_spec(b, k, w)[0] == _native.RT_E_INVALID
        both(feeds[3])
        rec = same()
        assert _fetch_spec(b, k, w)[:2] == (_native.RT_OK, len(rec))
        good(len(rec))
        # a truncated delivery
        n = C.c_size_t(0)
        out = np.zeros(2, _native.RECORD_DTYPE)
        lib.rt_fetch(h, out.ctypes.data, 2, C.byref(n))
        assert n.value > 2
        assert _fetch_spec(b, k, w)[0] == _native.RT_E_INVALID and _err(b) == name + ": the call fetched last was delivered truncated"
        twin.fetch_records()
        # a call without records
        both(np.zeros((S, 4 * nperseg), np.complex64))
        assert len(same()) == 0
        assert _fetch_spec(b, k, w)[:2] == (_native.RT_OK, 0)
        got = b.fetch_record_spectrum(k, w)
        assert got[0].shape == (0,) and got[1].shape == got[2].shape == (0, B)
        # the feature turned off again
        b.native.set_record_iq(-1)
        twin.native.set_record_iq(-1)
        both(feeds[0])
        same()
        assert _fetch_spec(b, k, w)[0] == _native.RT_E_INVALID and "rt_set_record_iq" in _err(b)
    finally:
        for x in (b, twin, off_handle, small):
            x.close()


# ---- 7: the entry changes nothing else, and costs nothing where it is not called ---------------------------------------------------
def test_the_entry_changes_nothing_else():
    """With the entry never called and with it called after every fetch, in front of and between everything else: the records, the
    record cells, the record IQ, the STFT values, the estimate rows and the band are the same bytes."""
    nperseg, fmt, margin = 256, "c64", 2
    sides = {}
    for use in (False, True):
        got = []

        def after(b, c, rec, use=use, got=got):
            row = [rec.tobytes()]
            for fetch in (b.fetch_record_cells, b.fetch_record_iq, b.fetch_record_stft, lambda: b.fetch_record_stft(hop_div=4),
                          lambda: (b.fetch_record_estimates(hop_div=4),), lambda: b.fetch_record_band(4, 2), lambda: b.fetch_record_band(2, 8)):
                if use:
                    b.fetch_record_spectrum(4, 2)
                    b.fetch_record_spectrum(2, 8)
                row += [np.asarray(a).tobytes() for a in fetch()]
            got.append(row)

        _run(nperseg, fmt, margin, after, record_cells=True)
        sides[use] = got
    assert sides[False] == sides[True] and len(sides[True]) == N_CALLS


def test_a_handle_that_never_calls_the_entry_allocates_what_it_did():
    """Device memory in use once the schedule has run, read from the driver with the handle still open: a handle that never calls
    the entry uses what a second such handle uses, byte for byte; the band entry adds its pools, and the new entry's rows and plan
    come on top of those only on the handle that calls it (never less; the driver hands memory out in pieces larger than the small
    pools, so more is not required)."""
    import torch

    nperseg, fmt, margin = 256, "c64", 2
    feeds = [torch.from_numpy(rs.gpu_feed(nperseg, c, fmt)).cuda() for c in range(N_CALLS)]

    def used(call):
        torch.cuda.synchronize()
        before = torch.cuda.mem_get_info()[0]
        b = _handle(nperseg, fmt, margin)
        try:
            for x in feeds:
                b.enqueue(x)
                b.fetch_records()
                call(b)
            torch.cuda.synchronize()
            return before - torch.cuda.mem_get_info()[0]
        finally:
            b.close()

    used(lambda b: b.fetch_record_spectrum(4, 2))  # (what the process itself allocates once is allocated here)
    plain = used(lambda b: None)
    band_only = used(lambda b: b.fetch_record_band(4, 2))
    with_rows = used(lambda b: b.fetch_record_spectrum(4, 2))
    again = used(lambda b: None)
    print(f"record_spectrum device bytes: never called {plain} / {again}, band entry {band_only}, spectrum {with_rows}")
    assert plain == again > 0
    assert with_rows >= band_only >= plain


# ---- 8: the Python layers ----------------------------------------------------------------------------------------------------------
def test_signal_analyzer_and_replay_leave_the_spectrum_beside_the_band():
    nperseg, margin, k, w = 256, 2, 4, 2
    sched = sq.SCHEDULES["B"]
    n_buf = 5
    B = sched.T[0] * nperseg
    x = np.concatenate([sq.buffer(sched, nperseg, c, 1)[0] for c in range(n_buf)])
    kw = sq.settings(nperseg)
    with pytest.raises(ValueError):
        SignalAnalyzer("0", sdr_callback_length=B, record_iq=True, record_spectrum=True, **kw)
    a = SignalAnalyzer("0", sdr_callback_length=B, record_iq=True, record_iq_margin=margin, record_band=w, record_spectrum=True, stft_hop_div=k, **kw)
    ts0 = datetime.datetime(2024, 1, 1)
    kept = []
    try:
        for c in range(n_buf):
            buf = x[c * B:(c + 1) * B]
            got = a.analyze_buffer(buf, ts0 + datetime.timedelta(seconds=c * B / sq.FS))
            rows, mean, peak = a.signal_spectrum
            assert len(rows) == len(mean) == len(peak) == len(a.signal_band) == len(got)
            # what the host definition makes of each signal's own band
            for i, band in enumerate(a.signal_band):
                inside = int(rows["n_inside"][i])
                assert mean.shape[1] == band.shape[1] == 2 * w + 1 and 0 < inside <= len(band)
            if len(rows):
                assert (rows["peak_col"] == w).all()  # bin-centred tones
                hz = spectrum_hz(rows, sq.FS, nperseg)
                assert np.array_equal(hz["width"], rows["width"] * (sq.FS / nperseg))
            kept.extend(rows)
        with pytest.raises(ValueError):
            a.replay(x, ts0, chain=2, record_iq=True, record_spectrum=True)
        out = a.replay(x, ts0, chain=2, record_iq=True, stft_hop_div=k, record_band=w, record_spectrum=True)
    finally:
        a._batch.close()
        if a._replay_batch is not None:
            a._replay_batch.close()
    signals, out_iq, out_band, out_spec = out
    assert len(signals) == len(out_iq) == len(out_band) == len(out_spec) == len(kept) > 3
    for got, want, band in zip(out_spec, kept, out_band):
        assert got.tobytes() == want.tobytes()
        one = record_band_rows([0, len(band)], [0], band, [0], [0], nperseg, k)[0]  # (no cells named: nothing inside)
        assert one["n_inside"][0] == 0


def test_zz_write_the_worst_ratios():
    """(last in the file: the table of what the tests above saw on this GPU)"""
    assert WORST
    table = sc.format_worst("rt_fetch_record_spectrum on an MI355X against record_band_rows on the same handle's band (tests/test_gpu_record_spectrum.py)", WORST)
    print(table)
    assert max(max(v.values()) for v in WORST.values()) <= 1.0
    if os.environ.get("RT_WRITE_PROFILES"):
        sc.write_worst("gpu", table)

