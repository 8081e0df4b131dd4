"""Cross-call state over long call sequences on the GPU: one handle per case, every call of a schedule of
tests/sequence_cases.py through it, every call and stream held to the oracle (identity and shadow verdicts exactly, the float
fields within the precision64 model -- no tolerance of its own).  Three look-back tails rotate, so only from the fourth call on
does a scan write a tail that was written before; tests/test_sequence_contract.py shows on the CPU that the schedules see a tail
writer that drops the cell a walk stops on, or misplaces the columns of a short call, and that three calls see neither.

Case table (schedule, nperseg, mode, what varies) -- see the parametrisations below; ``-s`` prints per case the trace
``call:mode_used/fell_back/dense streams/records`` and at the end the worst |gpu - f64| / bound per family."""
import numpy as np
import pytest

from pyradiotracking_amd import _native
from pyradiotracking_amd.analyze import BatchSignalAnalyzer
from tests import precision64 as p64
from tests import sequence_cases as sq
from tests import test_gpu_record_cells as trc
from tests import test_gpu_row_means as trm
from tests.test_gpu_float64 import family, form_of
from tests.test_gpu_float64_path import DB_TOL as F64_DB_TOL, STD_TOL as F64_STD_TOL

pytestmark = pytest.mark.gpu

WORST = {}  # (family, what) -> worst ratio


@pytest.fixture(autouse=True)
def _need_gpu():
    if _native.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")


def _note(nperseg):
    fam = family(nperseg)

    def note(what, r):
        WORST[(fam, what)] = max(WORST.get((fam, what), 0.0), float(r))

    return note


def _handle(name, nperseg, mode, fmt="c64", min_hops=sq.MIN_HOPS, **extra):
    sched = sq.SCHEDULES[name]
    if fmt in ("c128", "u8f64"):
        extra["precision"] = "float64"
    return BatchSignalAnalyzer([str(i) for i in range(sq.n_streams(nperseg))], sdr_callback_length=sq.max_samples(sched, nperseg), mode=mode,
                               **sq.case_settings(nperseg, fmt, min_hops=min_hops), **extra)


def _case(name, nperseg, mode, fmt="c64", min_hops=sq.MIN_HOPS, events=(), pipelined=False, before_call=None, after_fetch=None, expect_mode=None,
          **extra):
    """One handle, the whole schedule, every call and stream against the oracle; returns the runs [(records, call_info)]."""
    sched = sq.SCHEDULES[name]
    what = f"{name} nperseg {nperseg} {mode} {fmt} {extra}"
    b = _handle(name, nperseg, mode, fmt, min_hops, **extra)
    try:
        runs = sq.run_handle(b, sched, nperseg, fmt, pipelined=pipelined, before_call=before_call and (lambda k: before_call(b, k)),
                             after_fetch=after_fetch and (lambda k, rec: after_fetch(b, k, rec)))
    finally:
        b.close()
    print(f"\n{what}: {sq.trace(runs)}")
    f64 = fmt in ("c128", "u8f64")
    form = form_of(nperseg, sq.WINDOW, extra.get("subtract_first", False), fmt == "u8")
    n_rec, n_neg = sq.hold_sequence(runs, name, nperseg, fmt, events, min_hops, form, (F64_DB_TOL, F64_STD_TOL) if f64 else None,
                                    _note(nperseg), what)
    assert n_rec > len(sched.T) and n_neg > len(sched.T) // 2, (n_rec, n_neg)
    if expect_mode is not None:
        assert all(i.mode_used == expect_mode for (r, i), t in zip(runs, sched.T) if t > 0), sq.trace(runs)
    return runs


# ----------------------------------------------------------------------------------------------------------------------------------
# every tail writer, sparse: stft_scan with lane groups of 2 / 4 / 8 lanes (32, 64, 128), direct stores (256), through the exchange
# rows (512 .. 2048, tail_any), stft_scan64 (4096), stft_wg (8192, 16384)
# ----------------------------------------------------------------------------------------------------------------------------------
SPARSE = [("A", n) for n in (32, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384)] + [("B", n) for n in (128, 256, 2048, 4096, 8192)]


@pytest.mark.parametrize("name,nperseg", SPARSE)
def test_sparse_tail_writers(name, nperseg):
    _case(name, nperseg, "sparse", expect_mode=_native.RT_MODE_SPARSE)


# dense writers: the scans' MODE 1, stft_general (8, 16), stft_bluestein (300, 4097)
DENSE = [("A", n, "dense") for n in (128, 256, 4096, 8192)] + [("A", n, "auto") for n in (8, 16, 300, 4097)]


@pytest.mark.parametrize("name,nperseg,mode", DENSE)
def test_dense_tail_writers(name, nperseg, mode):
    _case(name, nperseg, mode)


# the float64 path (stft_f64)
F64 = [("A", 256, "c128"), ("A", 300, "c128"), ("A", 256, "u8f64")]


@pytest.mark.parametrize("name,nperseg,fmt", F64)
def test_float64_path(name, nperseg, fmt):
    _case(name, nperseg, "auto", fmt)


# chunk geometry: the tail mask is kept per chunk
CHUNKS = [("A", n, L) for n in (256, 4096) for L in (4, 8, 16)]


@pytest.mark.parametrize("name,nperseg,L", CHUNKS)
def test_chunk_geometry(name, nperseg, L):
    runs = _case(name, nperseg, "sparse", segs_per_chunk=L)
    assert all(int(i.segs_per_chunk) == L for _, i in runs), [int(i.segs_per_chunk) for _, i in runs]


# input formats: the conversion is fused into the scan's load; the handle must also equal a complex64 handle fed the conversion
FORMATS = [(name, n, fmt) for name in ("A", "B") for n in (256, 4096) for fmt in ("u8", "i16", "i8")]


@pytest.mark.parametrize("name,nperseg,fmt", FORMATS)
def test_input_formats(name, nperseg, fmt):
    runs = _case(name, nperseg, "sparse", fmt)
    sched = sq.SCHEDULES[name]
    twin = _handle(name, nperseg, "sparse", "c64", signal_threshold_dbw=-90.0 + sq.WIRE_SHIFT_DB, **(dict(subtract_first=True) if fmt == "u8" else {}))
    try:
        for k in range(len(sched.T)):
            _, seen = sq.wire(sq.buffer(sched, nperseg, k, sigma=sq.case_sigma(fmt)), fmt)
            twin.enqueue(np.ascontiguousarray(seen))
            assert twin.fetch_records().tobytes() == runs[k][0].tobytes(), f"{name} {nperseg} {fmt} call {k}: differs from the complex64 handle"
    finally:
        twin.close()


# lanes and the detection form
LANES = [("A", 256, dict(lanes=2)), ("A", 256, dict(lanes=3)), ("A", 1024, dict(lanes=2)), ("A", 256, dict(group_detect=True)),
         ("A", 128, dict(group_detect=True))]


@pytest.mark.parametrize("name,nperseg,extra", LANES, ids=[f"{a}-{n}-{'-'.join(f'{k}{v}' for k, v in e.items())}" for a, n, e in LANES])
def test_lanes_and_detection_form(name, nperseg, extra):
    _case(name, nperseg, "sparse", **extra)


# pipelining: call k + 1 enqueued before call k is fetched (the two call slots alternate with both in use)
PIPELINED = [("A", 256, 1), ("A", 256, 2), ("A", 4096, 1)]


@pytest.mark.parametrize("name,nperseg,lanes", PIPELINED)
def test_pipelined_equals_serial(name, nperseg, lanes):
    serial = _case(name, nperseg, "sparse", lanes=lanes)
    piped = _case(name, nperseg, "sparse", pipelined=True, lanes=lanes)
    for k, ((a, _), (b, _)) in enumerate(zip(serial, piped)):
        assert a.tobytes() == b.tobytes(), f"call {k}"


# pre-filters on clean input (the level pinned): the chunk-bit level needs segs_per_chunk 4 and a minimum of 8 hops -- its own
# condition, min >= 2 L hops -- and runs of at least 10 segments (schedule B10: e stretched)
PREFILTER = [("B10", 256, "prefilter", 8.0, dict(segs_per_chunk=4)), ("B10", 128, "prefilter", 8.0, dict(segs_per_chunk=4)),
             ("B", 256, "runfilter", sq.MIN_HOPS, {}), ("B", 1024, "runfilter", sq.MIN_HOPS, {}), ("B", 4096, "runfilter", sq.MIN_HOPS, {})]


@pytest.mark.parametrize("name,nperseg,mode,min_hops,extra", PREFILTER, ids=[f"{a}-{n}-{m}" for a, n, m, _, _ in PREFILTER])
def test_prefilter_levels(name, nperseg, mode, min_hops, extra):
    _case(name, nperseg, mode, min_hops=min_hops, expect_mode={"prefilter": _native.RT_MODE_PREFILTER, "runfilter": _native.RT_MODE_RUNFILTER}[mode],
          **extra)


# the exact pre-filter pinned over the noise regimes of schedule C: its per-bin thresholds come from the previous call's chunk minima,
# so every change of regime meets thresholds of the regime before.  Case table: with the default hot_capacity (8192) the level
# refuses the call in which the floor jumps from 2 to 10 dB over the threshold at nperseg 1024 and 4096 (RT_E_HOT_OVERFLOW: thresholds
# 8 dB too low keep nearly every cell); the three cases run with 16384, the largest power of two whose lists fit the LDS.
@pytest.mark.parametrize("nperseg", [256, 1024, 4096])
def test_runfilter_over_noise_regimes(nperseg):
    _case("C", nperseg, "runfilter", min_hops=sq.C_MIN_HOPS, expect_mode=_native.RT_MODE_RUNFILTER, hot_capacity=16384)


# AUTO over the noise regimes: at nperseg 128 and 256 the lists are kept small enough (hot_capacity) for the floor to overflow them at
# 64 segments a call; at 4096 the default overflows
AUTO_RANK = {_native.RT_MODE_SPARSE: 0, _native.RT_MODE_PREFILTER: 1, _native.RT_MODE_RUNFILTER: 2, _native.RT_MODE_DENSE: 3}
AUTO_HOT_CAPACITY = {128: 256, 256: 512, 4096: 0}


@pytest.mark.parametrize("nperseg", [128, 256, 4096])
def test_auto_over_noise_regimes(nperseg):
    """Records equal the oracle's on every call whatever level AUTO is on; the trace holds a climb and at least one descent on which
    the handle stays -- a probe of a lower level that is followed by that level, not by the one above (more than that about the trace
    is printed, not asserted)."""
    runs = _case("C", nperseg, "auto", min_hops=sq.C_MIN_HOPS, segs_per_chunk=4, hot_capacity=AUTO_HOT_CAPACITY[nperseg])
    ranks = [AUTO_RANK[i.mode_used] for _, i in runs]
    assert any(i.fell_back for _, i in runs) and max(ranks) > ranks[0], ranks
    top = ranks.index(max(ranks))
    assert any(ranks[k] < ranks[k - 1] and ranks[k + 1] == ranks[k] for k in range(top + 1, len(ranks) - 1)), ranks


# side outputs
def _side_outputs(nperseg):
    sched = sq.SCHEDULES["A"]
    state = {"prev": None, "t_last": None}
    form = form_of(nperseg, sq.WINDOW)
    n_neg_cells = [0]

    def after_fetch(b, k, rec):
        T = sched.T[k]
        rm = b.fetch_row_means()
        off, cells = b.fetch_record_cells()
        assert rm.shape == (sq.n_streams(nperseg), nperseg) and rm.dtype == np.float32
        assert len(off) == len(rec) + 1 and np.array_equal(np.diff(off), rec["end"] - rec["start"]) and len(cells) == off[-1]
        if T == 0:
            assert np.isnan(rm).all() and len(rec) == 0
            state.update(prev=None, t_last=0)
            return
        trm._check_records_bits(rec, rm, nperseg, f"call {k}")
        L = max(1, int(b.native.call_info().segs_per_chunk))
        x = sq.buffer(sched, nperseg, k)
        refs = []
        for s in range(x.shape[0]):
            ref = p64.stft_power_f64(x[s], sq.FS, sq.WINDOW, nperseg)
            bd = p64.cell_bounds(ref, form)
            refs.append((ref, bd))
            # the row means of every bin, within the model (tests/test_gpu_row_means.py: test_every_size_family_within_the_model)
            err = np.abs(rm[s].astype(np.float64) - ref.P.mean(axis=0))
            bound = p64.row_mean_bound(ref, bd, L)
            j = int(np.argmax(err / bound))
            assert np.all(err <= bound), f"call {k} stream {s} bin {j}: row mean {rm[s][j]!r} vs {ref.P.mean(axis=0)[j]!r} (bound {bound[j]:.3g})"
        # every record's figures are the statistics of its cells (max(cells) == max_p bit for bit), the cells the plateau the walk found
        t_last = state["t_last"]
        if t_last == 0:
            # after the empty call the walk's limit is segment 1: a record may start ON a hot cell there, and at segment 0
            one = rec["start"] == 1
            for sel, tl in ((one, 0), (~one, None)):
                idx = np.flatnonzero(sel)
                sub_off = np.concatenate(([0], np.cumsum(off[idx + 1] - off[idx]))).astype(np.int64)
                sub_cells = np.concatenate([cells[off[i]:off[i + 1]] for i in idx]) if len(idx) else cells[:0]
                trc._check_own_statistics(b, rec[idx], sub_off, sub_cells, tl, f"call {k}")
        else:
            trc._check_own_statistics(b, rec, off, cells, t_last, f"call {k}")
        # ... and they are the map's: the cells of negative-start records from the previous buffer's map, within the cell bounds
        for r, o0, o1 in zip(rec, off[:-1], off[1:]):
            s, fi, a, e = int(r["stream"]), int(r["fi"]), int(r["start"]), int(r["end"])
            ref, bd = refs[s]
            pr = state["prev"][s] if a < 0 else (None, None)
            want = p64._cells(ref.P, pr[0].P if a < 0 else None, fi, a, e)
            dP = p64._cells(bd.dP, pr[1].dP if a < 0 else None, fi, a, e)
            c = cells[o0:o1].astype(np.float64)
            assert np.all(np.abs(c - want) <= dP), f"call {k} stream {s} bin {fi} [{a},{e}): cells {c} vs {want}"
            n_neg_cells[0] += int(a < 0)
        state.update(prev=refs, t_last=T)

    _case("A", nperseg, "sparse", after_fetch=after_fetch, row_means=True, record_cells=True)
    assert n_neg_cells[0] > 20


@pytest.mark.parametrize("nperseg", [256, 4096])
def test_side_outputs(nperseg):
    _side_outputs(nperseg)


# stream events in mid-sequence
EVENTS = (("reset", 5, 1), ("snr", 7, 2, 6.0))


@pytest.mark.parametrize("mode", ["sparse", "dense"])
def test_stream_events_in_mid_sequence(mode):
    """reset_stream(1) before call 5, stream 2's SNR threshold 3 -> 6 dB before call 7: the oracle of each of these streams is reset at
    that point (and stream 2's takes the new threshold), the other streams keep their look-back."""
    def before_call(b, k):
        if k == 5:
            b.reset_stream(1)
        if k == 7:
            snr = [sq.SNR_DB] * sq.n_streams(256)
            snr[2] = 6.0
            b.set_stream_settings(snr_threshold_db=snr)

    runs = _case("A", 256, mode, events=EVENTS, before_call=before_call)
    # the events took something away: without them streams 1 and 2 reach back in those calls
    plain = sq.oracle_run("A", 256)
    assert any(r.start < 0 for r in plain[5][1].records) and not (runs[5][0][runs[5][0]["stream"] == 1]["start"] < 0).any()
    with_events = sq.oracle_run("A", 256, "c64", EVENTS)
    assert not any(r.start < 0 for r in with_events[7][2].records) and any(r.start < 0 for r in with_events[8][2].records)
    assert any(sq.key(plain[k][2].records) != sq.key(with_events[k][2].records) for k in range(8, len(plain))), "6 dB changes nothing for stream 2"
    for s in (0, 3, 4):
        assert all(sq.key(plain[k][s].records) == sq.key(with_events[k][s].records) for k in range(len(plain)))


def oracle_keys():
    """Every (schedule, nperseg, format, events, minimum) the cases above ask the oracle for (tests/test_sequence_contract.py runs them
    all on the CPU)."""
    keys = [(a, n, "c64", (), sq.MIN_HOPS) for a, n in SPARSE] + [(a, n, "c64", (), sq.MIN_HOPS) for a, n, _ in DENSE]
    keys += [(a, n, f, (), sq.MIN_HOPS) for a, n, f in F64 + FORMATS]
    keys += [(a, n, "c64", (), sq.MIN_HOPS) for a, n, _ in CHUNKS + LANES + PIPELINED]
    keys += [(a, n, "c64", (), h) for a, n, _, h, _ in PREFILTER]
    keys += [("A", 256, "c64", EVENTS, sq.MIN_HOPS), ("A", 4096, "c64", (), sq.MIN_HOPS)]
    keys += [("C", n, "c64", (), sq.C_MIN_HOPS) for n in (128, 256, 1024, 4096)]
    return sorted(set(keys), key=str)


def test_zz_print_worst_ratios():
    """The worst |gpu - f64| / bound per family and field over the sequences above (``-s`` shows it)."""
    for (fam, what), v in sorted(WORST.items()):
        print(f"sequences gpu-f64 {fam:16s} {what:22s} {v:.3f}")
    assert all(v <= 1.0 for v in WORST.values())
