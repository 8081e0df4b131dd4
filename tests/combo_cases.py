"""Every pair of handle features together (tests/test_combo_contract.py on the CPU, tests/test_gpu_combos.py on the GPU).

The single-feature GPU files move one feature at a time; the defects that reached the repository were interactions of two or three.
``CASES`` is a fixed table of small cases in which every pair of values of two different axes that ``rt_create`` / ``rt_create_f64``
allow together occurs at least once, and every allowed triple (size of a fused scan, input format, sparse | dense) occurs on a
float32 handle -- the template instantiations of the float32 scans; a float64 handle's own kernels do not count towards it.  No
triple requirement had to be dropped to stay at or under ``MAX_CASES``.  The table is built at import by a greedy cover over the
enumeration of all valid cases (no randomness: the first best candidate wins).

Every case runs ONE handle through schedule P of tests/sequence_cases.py -- ten calls of at most 47 segments, schedule A's tone
tables -- and every call and stream is held to one oracle (``oracle_run``): an independent analyzer state per stream, an absent
(call, stream) pair skipped, a reset or a changed setting clearing the stream's previous map, every stream gated by its own
parameters, the wire formats seen through the kernels' conversion (float64 handles: pyrtlsdr's / the exact widening).  Nothing of
the kernels' structure is in it: no chunks, no tails, no K.

Axes (``Case``):
  size      16 (stft_general), 300 (stft_bluestein), 64 (lane groups), 256, 512 (exchange-row tail), 1024 (persistent grid),
            4096 (stft_scan64), 8192 (stft_wg)
  path      f32 | f64 (dense float64) | f64s (map-free float64, RT_FLAG_F64_SPARSE)
  fmt       cx (complex64, complex128 on float64 handles) | u8 | i16 | i8
  mode      sparse | dense | auto | runfilter
  lanes     1 | 2 | 3
  pipelined call k + 1 enqueued before call k is fetched
  presence  all | gaps (``present_cases.table("P")``, the absent rows poisoned)
  settings  uniform | perstream (``STREAM_SETTINGS`` at create) | events (per-stream, and ``EVENTS`` in mid-sequence)
  side      none | means (row_means) | cells (row_means and record_cells)
  chunk     segs_per_chunk 0 | 4 | 16
  form      default | subfirst (subtract_first) | group (group_detect)

The per-stream settings are in hops and dBW, so they serve every nperseg: the defaults (2.5 / 40 hops, -90 dBW, 2.9 dB); a minimum of
8 hops; a maximum of 25.5 hops (drops the reach-backs 31 and 33 deep, and every run of 25 cells and more: the handle is created with
the envelope, K = 42, so this stream reads a rotated tail wider than its own gate); a threshold of -69.25 dBW, a quarter of a dB
from the tones at -69 and -69.5; an SNR threshold of 8 dB.  ``EVENTS``: stream 2's SNR threshold 2.9 -> 8 dB before call 4 (under the
presence table it sits out calls 3 .. 5: the change takes effect at call 6), ``reset_stream(1)`` before call 6 (present).

SNR thresholds: a tone that is hot in h of a call's T segments has cells T / h over its row's mean, whatever its level; 2.9 dB
(1.950) and 8 dB (6.31) lie 4.6 % from the nearest T / h of schedule P, where 3 dB is 2.4 % under 47 / 23 -- inside the scatter
the noise gives a side bin's cells on the wire formats.  Wire formats: ``sequence_cases.wire`` multiplies by 20 before it
quantises, and a bin-centred tone of a given cell power has an amplitude ~ 1 / sqrt(nperseg) -- six tones at -68 dBW clip at the
rails up to nperseg 512, and the intermodulation lands at the threshold's level.  ``wire_levels`` lowers the tones (and stream 3's
threshold with them) by 6 dB up to 512 and by 12 dB up to 64, where the threshold goes down by 6 dB as well, so that the lowest
tone's side bins stay 6 dB over it and the noise 20 dB under.  ``SEEDS``: the noise seed of the five (size, format) pairs whose
maps under the schedules' own seed hold a cell within the margin of a threshold (tests/test_combo_contract.py)."""
import functools
import types
from collections import namedtuple

import numpy as np

from oracle import analyze_oracle as oracle
from tests import precision64 as p64
from tests import present_cases as pc
from tests import sequence_cases as sq

SCHEDULE = "P"
MAX_CASES = 80

Case = namedtuple("Case", "size path fmt mode lanes pipelined presence settings side chunk form")
AXES = {
    "size": (16, 300, 64, 256, 512, 1024, 4096, 8192),
    "path": ("f32", "f64", "f64s"),
    "fmt": ("cx", "u8", "i16", "i8"),
    "mode": ("sparse", "dense", "auto", "runfilter"),
    "lanes": (1, 2, 3),
    "pipelined": (False, True),
    "presence": ("all", "gaps"),
    "settings": ("uniform", "perstream", "events"),
    "side": ("none", "means", "cells"),
    "chunk": (0, 4, 16),
    "form": ("default", "subfirst", "group"),
}
TRIPLE_SIZES = (64, 256, 512, 1024, 4096, 8192)
TRIPLE_MODES = ("sparse", "dense")
F64_SPARSE_SIZES = (64, 256, 512, 1024, 4096)


def valid(c):
    """What rt_create / rt_create_f64 (and BatchSignalAnalyzer ahead of them) accept.  ``c``: a Case, or one of arrays of values."""
    size, path, mode, form = np.asarray(c.size), np.asarray(c.path), np.asarray(c.mode), np.asarray(c.form)
    f64 = path != "f32"
    bad = np.isin(size, (16, 300)) & ~np.isin(mode, ("auto", "dense"))      # the general transforms run on the dense path only
    bad |= (size == 8192) & (mode == "runfilter")                           # stft_wg: the sparse and the dense path only
    bad |= f64 & ((np.asarray(c.lanes) != 1) | ~np.isin(mode, ("auto", "dense")) | (form == "group"))  # float64: one lane, the dense path
    # the map-free path: fused sizes, no record cells, selects its path itself
    bad |= (path == "f64s") & (~np.isin(size, F64_SPARSE_SIZES) | (np.asarray(c.side) == "cells") | (mode != "auto"))
    bad |= (form == "group") & ~np.isin(size, (64, 256))                    # one wave per stream: the sparse-capable sizes up to 256
    return ~bad if bad.ndim else not bad


# ---- the table -------------------------------------------------------------------------------------------------------------------
def _generate():
    """Greedy cover: the valid case that holds most goals (pairs, triples) still open; among equals the one whose pairs have
    occurred least so far, then the first -- so the cases that are only there for a triple vary their other axes too."""
    names = list(AXES)
    sizes = [len(AXES[n]) for n in names]
    grid = np.indices(sizes).reshape(len(names), -1).T  # every combination of value indices
    grid = grid[valid(Case(*(np.array(AXES[n])[grid[:, i]] for i, n in enumerate(names))))]
    # one column of goal numbers per pair of axes, one for the triple (size, fmt, mode)
    cols, base = [], 0
    for a in range(len(names)):
        for b in range(a + 1, len(names)):
            cols.append(base + grid[:, a] * sizes[b] + grid[:, b])
            base += sizes[a] * sizes[b]
    i_size, i_fmt, i_mode = names.index("size"), names.index("fmt"), names.index("mode")
    # (on a float32 handle: a float64 handle runs its own double-precision kernels, not the instantiations the triple stands for)
    in_triple = (np.isin(np.array(AXES["size"])[grid[:, i_size]], TRIPLE_SIZES) & np.isin(np.array(AXES["mode"])[grid[:, i_mode]], TRIPLE_MODES)
                 & (np.array(AXES["path"])[grid[:, names.index("path")]] == "f32"))
    triple = base + (grid[:, i_size] * sizes[i_fmt] + grid[:, i_fmt]) * sizes[i_mode] + grid[:, i_mode]
    dummy = base + sizes[i_size] * sizes[i_fmt] * sizes[i_mode]
    cols.append(np.where(in_triple, triple, dummy))
    goals = np.stack(cols, axis=1)
    open_ = np.zeros(dummy + 1, bool)
    open_[np.unique(goals)] = True  # what some valid case holds
    open_[dummy] = False
    seen = np.zeros(dummy + 1)
    out = []
    while open_.any():
        gain = open_[goals].sum(axis=1)
        cand = np.flatnonzero(gain == gain.max())
        best = int(cand[np.argmin(seen[goals[cand]].sum(axis=1))])  # (the first of the best: deterministic)
        out.append(Case(*(AXES[n][i] for n, i in zip(names, grid[best]))))
        open_[goals[best]] = False
        seen[goals[best]] += 1
    return out


def case_id(c):
    return (f"{c.size}-{c.path}-{c.fmt}-{c.mode}-l{c.lanes}-{'pipe' if c.pipelined else 'serial'}-{c.presence}-{c.settings}-{c.side}-c{c.chunk}"
            f"-{c.form}")


def case_of(text):
    """The case of an id (of the table or not)."""
    size, path, fmt, mode, lanes, pipe, presence, settings, side, chunk, form = text.split("-")
    c = Case(int(size), path, fmt, mode, int(lanes[1:]), pipe == "pipe", presence, settings, side, int(chunk[1:]), form)
    assert case_id(c) == text and all(v in AXES[k] for k, v in c._asdict().items()) and valid(c), text
    return c


CASES = _generate()
BY_ID = {case_id(c): c for c in CASES}

# ---- a case's inputs and keywords ------------------------------------------------------------------------------------------------
MAX_HOPS_SHORT = 25.5
SNR_DB, SNR_HIGH_DB = 2.9, 8.0
THRESHOLD_BETWEEN_TONES = -69.25
STREAM_SETTINGS = ({}, dict(min_hops=8.0), dict(max_hops=MAX_HOPS_SHORT), dict(signal_threshold_dbw=THRESHOLD_BETWEEN_TONES),
                   dict(snr_threshold_db=SNR_HIGH_DB))
EVENTS = (("snr", 4, 2, SNR_HIGH_DB), ("reset", 6, 1))
PER_STREAM_KEYS = ("signal_min_duration_ms", "signal_max_duration_ms", "signal_threshold_dbw", "snr_threshold_db")


def wire_fmt(c):
    """The case's format in ``sequence_cases.wire``'s names."""
    if c.path == "f32":
        return "c64" if c.fmt == "cx" else c.fmt
    return "c128" if c.fmt == "cx" else c.fmt + "f64"


def events_of(settings):
    return EVENTS if settings == "events" else ()


def wire_levels(size, fmt):
    """(tone level, threshold) offsets in dB of a wire format at this size, see the module docstring."""
    if not sq.is_wire(fmt) or size > 512:
        return 0.0, 0.0
    return (-12.0, -6.0) if size <= 64 else (-6.0, 0.0)


def stream_kwargs(size, fmt, settings, s):
    """Analysis keywords of stream s (oracle and analyzer alike)."""
    over = dict(STREAM_SETTINGS[s]) if settings != "uniform" else {}
    min_hops = over.pop("min_hops", sq.MIN_HOPS)
    if "max_hops" in over:
        over["signal_max_duration_ms"] = 1e3 * over.pop("max_hops") * sq.hop_s(size)
    tone_db, thr_db = wire_levels(size, fmt)
    over["signal_threshold_dbw"] = over["signal_threshold_dbw"] + tone_db if "signal_threshold_dbw" in over else -90.0 + thr_db
    over.setdefault("snr_threshold_db", SNR_DB)
    return sq.case_settings(size, fmt, min_hops=min_hops, **over)


#: noise seeds per (size, format) where the schedules' own (2024) leaves a cell -- of a map, or of the tail a walk looks back into --
#: within the margin of a threshold: on the lowered levels of the small sizes a side bin's cells scatter by 5 % and some land
#: there by chance.  Searched on the CPU from 1 upwards; tests/test_combo_contract.py holds every map of the committed seeds to
#: the margin.
SEEDS = {(512, "i8"): 1, (64, "i16"): 1, (256, "i16"): 2, (256, "i8"): 3, (512, "i16"): 1}


def raw_buffer(size, fmt, k):
    """complex64 [S, n]: call k of schedule P before the format's conversion."""
    return sq.buffer(sq.SCHEDULES[SCHEDULE], size, k, sigma=sq.case_sigma(fmt), seed=SEEDS.get((size, fmt), 2024),
                     peak_dbw=sq.PEAK_DBW + wire_levels(size, fmt)[0])


def envelope_kwargs(size, fmt, settings):
    """What the handle itself is created with: the envelope of the durations, the first stream's thresholds."""
    per = [stream_kwargs(size, fmt, settings, s) for s in range(sq.n_streams(size))]
    return dict(per[0], signal_min_duration_ms=min(p["signal_min_duration_ms"] for p in per),
                signal_max_duration_ms=max(p["signal_max_duration_ms"] for p in per))


def handle_kwargs(c):
    """BatchSignalAnalyzer's keywords of the case (without ``devices`` and ``sdr_callback_length``)."""
    fmt, S = wire_fmt(c), sq.n_streams(c.size)
    per = [stream_kwargs(c.size, fmt, c.settings, s) for s in range(S)]
    kw = dict(per[0])
    if c.settings != "uniform":
        for name in PER_STREAM_KEYS:
            kw[name] = [p[name] for p in per]
    kw.update(mode=c.mode, lanes=c.lanes, segs_per_chunk=c.chunk, row_means=c.side != "none", record_cells=c.side == "cells")
    if c.form == "subfirst":
        kw["subtract_first"] = True
    if c.form == "group":
        kw["group_detect"] = True
    if c.path != "f32":
        kw["precision"] = "float64"
    if c.path == "f64s":
        kw.update(f64_sparse=True, hot_capacity=8192)  # (six tones of three bins, up to 48 segments each, and the cells before them)
    return kw


def expect_mode(c):
    from pyradiotracking_amd import _native

    if c.path == "f64s":
        return _native.RT_MODE_SPARSE
    return {"sparse": _native.RT_MODE_SPARSE, "dense": _native.RT_MODE_DENSE, "runfilter": _native.RT_MODE_RUNFILTER}.get(c.mode)


def presence_of(c_or_gaps, size):
    gaps = c_or_gaps if isinstance(c_or_gaps, bool) else c_or_gaps.presence == "gaps"
    S = sq.n_streams(size)
    return pc.table(SCHEDULE, S) if gaps else np.ones((len(sq.SCHEDULES[SCHEDULE].T), S), bool)


def seen_buffers(size, fmt, k):
    """Call k of every stream as the reference arithmetic sees it."""
    return sq.wire(raw_buffer(size, fmt, k), fmt)[1]


# ---- the oracle ------------------------------------------------------------------------------------------------------------------
MODELS = ("contract", "zeros_reset", "lockstep", "envelope", "no_restart", "drop_stop", "offset")


@functools.lru_cache(maxsize=2)
def maps(size, fmt):
    """[call][stream] -> (freqs, times, map): the reference's STFT of every buffer (what every model of one (size, format) shares)."""
    return [[oracle.stft_power(x, sq.FS, sq.WINDOW, size) for x in seen_buffers(size, fmt, k)] for k in range(len(sq.SCHEDULES[SCHEDULE].T))]


def oracle_key(c):
    """What the oracle depends on."""
    return (c.size, wire_fmt(c), c.presence == "gaps", c.settings)


def oracle_run(c, model="contract"):
    """[call][stream] -> ``sequence_cases.Call`` (None for an absent pair).  ``model``: the contract, or one of the wrong models the
    contract test holds it apart from -- ``zeros_reset`` / ``lockstep`` (an absent stream, as in tests/present_cases.py),
    ``envelope`` (every stream gated by the handle's envelope of durations and the first stream's thresholds), ``no_restart`` (a
    changed setting keeps the look-back); ``drop_stop`` / ``offset``: ``sequence_cases.tail_model_records`` under that rule, whose
    entries are record keys (the settings of ``sequence_cases.oracle_run``, complex64, chunks of 4)."""
    if model in ("drop_stop", "offset"):
        per = []
        for s in range(sq.n_streams(c.size)):
            try:
                per.append(sq.tail_model_records(SCHEDULE, c.size, s, 4, model))
            except IndexError:  # (the mutated tail sends a walk past a short call's time axis: None for that stream)
                per.append([None] * len(sq.SCHEDULES[SCHEDULE].T))
        return [list(row) for row in zip(*per)]
    return _oracle(*oracle_key(c), model)


@functools.lru_cache(maxsize=None)
def _oracle(size, fmt, gaps, settings, model):
    assert model in MODELS
    sched = sq.SCHEDULES[SCHEDULE]
    S = sq.n_streams(size)
    present = presence_of(gaps, size)
    kws = [envelope_kwargs(size, fmt, settings) if model == "envelope" else stream_kwargs(size, fmt, settings, s) for s in range(S)]
    last = [None] * S
    every = maps(size, fmt)
    out = []
    for k in range(len(sched.T)):
        for ev in events_of(settings):
            if ev[1] == k:
                if ev[0] == "snr":
                    if model != "envelope":
                        kws[ev[2]] = dict(kws[ev[2]], snr_threshold_db=ev[3])
                    if model == "no_restart":
                        continue
                last[ev[2]] = None  # (absent or not: an absent call does not touch it)
        row = []
        for s in range(S):
            if not present[k, s]:
                row.append(None)
                if model == "zeros_reset":
                    last[s] = None
                elif model == "lockstep" and last[s] is not None:
                    last[s] = np.zeros((size, sched.T[k]), last[s].dtype)
                continue
            freqs, times, spec = every[k][s]
            recs = sq.extract(times, spec, last[s], sq.params_of(kws[s]))
            row.append(sq.Call(recs, sq.shadow_flags(recs, freqs)))
            last[s] = spec
        out.append(row)
    return out


# ---- feeding a handle ------------------------------------------------------------------------------------------------------------
Run = namedtuple("Run", "records info row_means offsets cells")


def apply_event(b, c, ev):
    if ev[0] == "reset":
        b.reset_stream(ev[2])
    else:
        snr = [stream_kwargs(c.size, wire_fmt(c), c.settings, s)["snr_threshold_db"] for s in range(sq.n_streams(c.size))]
        snr[ev[2]] = ev[3]
        b.set_stream_settings(snr_threshold_db=snr)


def run_handle(b, c):
    """Every call of schedule P through handle ``b`` -> [Run].  With the presence table the mask is set ahead of every enqueue and the
    rows of absent streams hold poison; ``pipelined``: call k + 1 is enqueued before call k is fetched -- but for an event, which is a
    serial-only hook: the calls in flight are settled first.  The side outputs are fetched with their call's records."""
    sched = sq.SCHEDULES[SCHEDULE]
    fmt = wire_fmt(c)
    present = presence_of(c, c.size)
    out, in_flight = [], [0]

    def fetch():
        rec = b.fetch_records()
        info = b.native.call_info()
        rm = b.fetch_row_means() if c.side != "none" else None
        off, cells = b.fetch_record_cells() if c.side == "cells" else (None, None)
        out.append(Run(rec, info, rm, off, cells))
        in_flight[0] -= 1

    for k in range(len(sched.T)):
        due = [ev for ev in events_of(c.settings) if ev[1] == k]
        if due:
            while in_flight[0]:
                fetch()
            for ev in due:
                apply_event(b, c, ev)
        if c.presence == "gaps":
            b.set_present(present[k])
        sq.enqueue(b, pc.poisoned(raw_buffer(c.size, fmt, k), present[k], fmt), fmt)
        in_flight[0] += 1
        while in_flight[0] > (1 if c.pipelined else 0):
            fetch()
    while in_flight[0]:
        fetch()
    return out


# ---- holding a run to the oracle -------------------------------------------------------------------------------------------------
def _stream_cells(run, idx):
    """(offsets, cells) of the records ``idx`` of a call."""
    off = np.concatenate(([0], np.cumsum(run.offsets[idx + 1] - run.offsets[idx]))).astype(np.int64)
    cells = np.concatenate([run.cells[run.offsets[i]:run.offsets[i + 1]] for i in idx]) if len(idx) else run.cells[:0]
    return off, cells


def hold(c, runs, note=None):
    """After every call, per stream: an absent stream delivers nothing (NaN row means); a present one's identity (fi, start, end) and
    shadow verdicts equal the oracle's; its float fields lie within the precision64 model of the float64 transform of the same input
    (look-back cells from the reference of the stream's own last present buffer, L from call_info) -- on a float64 handle within
    DB_TOL / STD_TOL of the oracle's float64 figures; row means and record cells go through the checks of tests/test_gpu_row_means.py
    and tests/test_gpu_record_cells.py.  No tolerance of its own.  Returns (records, negative starts, negative starts across a gap)."""
    from tests import test_gpu_record_cells as trc
    from tests import test_gpu_row_means as trm
    from tests.test_gpu_float64 import form_of
    from tests.test_gpu_float64_path import DB_TOL

    sched = sq.SCHEDULES[SCHEDULE]
    size, fmt, S = c.size, wire_fmt(c), sq.n_streams(c.size)
    f64 = c.path != "f32"
    form = form_of(size, sq.WINDOW, c.form == "subfirst", fmt == "u8")
    present = presence_of(c, size)
    want = oracle_run(c)
    kws = [stream_kwargs(size, fmt, c.settings, s) for s in range(S)]
    prev = [None] * S          # float32 handles: (Ref64, Bounds) of the stream's own last present buffer; float64: (map, cell bound)
    t_last = [None] * S        # its segment count (None: no previous map)
    last_present = [None] * S
    n_rec = n_neg = n_gap = 0
    assert len(runs) == len(sched.T)
    for k, run in enumerate(runs):
        T = sched.T[k]
        L = max(1, int(run.info.segs_per_chunk))
        seen = seen_buffers(size, fmt, k)
        for ev in events_of(c.settings):
            if ev[1] == k:
                prev[ev[2]] = t_last[ev[2]] = None
                if ev[0] == "snr":
                    kws[ev[2]] = dict(kws[ev[2]], snr_threshold_db=ev[3])
        rec = run.records
        if run.row_means is not None:
            assert run.row_means.shape == (S, size) and run.row_means.dtype == (np.float64 if f64 else np.float32), f"call {k}: row means"
            if len(rec):
                trm._check_records_bits(rec, run.row_means, size, f"call {k}: a record's row_mean is not its bin's entry")
        if run.offsets is not None:
            assert len(run.offsets) == len(rec) + 1 and np.array_equal(np.diff(run.offsets), rec["end"] - rec["start"]), f"call {k}: cell offsets"
            assert len(run.cells) == run.offsets[-1], f"call {k}: cell count"
        for s in range(S):
            idx = np.flatnonzero(rec["stream"] == s)
            mine = rec[idx]
            tag = f"call {k} (T {T}) stream {s}"
            if not present[k, s]:
                assert len(mine) == 0, f"{tag}: an absent stream delivered {sq.rec_key(mine)}"
                if run.row_means is not None:
                    assert np.isnan(run.row_means[s]).all(), f"{tag}: row means of an absent stream"
                continue
            w = want[k][s]
            assert sq.rec_key(mine) == sq.key(w.records), f"{tag}: records differ from the oracle's\n got  {sq.rec_key(mine)}\n want {sq.key(w.records)}"
            assert [bool(v) for v in mine["shadowed"]] == w.shadowed, f"{tag}: shadow verdicts"
            if T == 0:
                if run.row_means is not None:
                    assert np.isnan(run.row_means[s]).all(), f"{tag}: row means of an empty call"
                prev[s], t_last[s] = None, 0
                last_present[s] = k
                continue
            pr = prev[s]
            if f64:
                try:
                    sq.check_f64(mine, w.records)
                except AssertionError as e:
                    raise AssertionError(f"{tag}: float64 fields: {e}") from None
                _, _, spec = maps(size, fmt)[k][s]
                cur = (spec, trc._f64_cell_bound(spec, size))
                if run.row_means is not None:
                    err = np.abs(oracle.to_db(run.row_means[s]) - oracle.to_db(spec.mean(axis=1)))
                    j = int(np.argmax(err))
                    assert np.all(err <= DB_TOL), f"{tag} bin {j}: row mean {run.row_means[s][j]!r} vs {spec.mean(axis=1)[j]!r}"
                    if note:
                        note("row mean dB / DB_TOL (f64)", err.max() / DB_TOL)
            else:
                ref = p64.stft_power_f64(seen[s], sq.FS, sq.WINDOW, size)
                bd = p64.cell_bounds(ref, form)
                cur = (ref, bd)
                if len(mine):
                    chk = p64.check_records(mine, ref, bd, L, pr[0] if pr else None, pr[1] if pr else None, what=tag)
                    assert not chk.failures, "\n".join(chk.failures[:8])
                    if note:
                        for f, v in chk.worst.items():
                            note(f"{f} ({form})", v)
                if run.row_means is not None:
                    err = np.abs(run.row_means[s].astype(np.float64) - ref.P.mean(axis=0))
                    bound = p64.row_mean_bound(ref, bd, L)
                    j = int(np.argmax(err / bound))
                    assert np.all(err <= bound), f"{tag} bin {j}: row mean {run.row_means[s][j]!r} vs {ref.P.mean(axis=0)[j]!r} (bound {bound[j]:.3g})"
                    if note:
                        note(f"row mean ({form})", (err / bound).max())
            if run.cells is not None and len(idx):
                # every record's figures are the statistics of its cells (max(cells) == max_p bit for bit), the cells the plateau the
                # walk found -- against the stream's own thresholds -- and the cells are the map's, within the cell bounds
                p = sq.params_of(kws[s])
                gate = types.SimpleNamespace(signal_threshold=p.signal_threshold, snr_threshold=p.snr_threshold)
                if t_last[s] == 0:  # behind an empty buffer of its own the walk's limit is segment 1: a record may start ON a hot cell there
                    one = mine["start"] == 1
                    for sel, tl in ((one, 0), (~one, None)):
                        trc._check_own_statistics(gate, mine[sel], *_stream_cells(run, idx[sel]), tl, tag)
                else:
                    trc._check_own_statistics(gate, mine, *_stream_cells(run, idx), t_last[s], tag)
                for r, i in zip(mine, idx):
                    fi, a, e = int(r["fi"]), int(r["start"]), int(r["end"])
                    got = run.cells[run.offsets[i]:run.offsets[i + 1]].astype(np.float64)
                    if f64:
                        ref_c = trc._oracle_cells(cur[0], pr[0] if a < 0 else None, r)
                        bound_c = trc._oracle_cells(cur[1], pr[1] if a < 0 else None, r)
                    else:
                        ref_c = p64._cells(cur[0].P, pr[0].P if a < 0 else None, fi, a, e)
                        bound_c = p64._cells(cur[1].dP, pr[1].dP if a < 0 else None, fi, a, e)
                    assert np.all(np.abs(got - ref_c) <= bound_c), f"{tag} bin {fi} [{a},{e}): cells {got} vs {ref_c}"
                    if note:
                        note(f"cells ({'f64' if f64 else form})", float((np.abs(got - ref_c) / bound_c).max()))
            prev[s], t_last[s] = cur, T
            neg = int((mine["start"] < 0).sum())
            n_rec += len(mine)
            n_neg += neg
            if last_present[s] is not None and k - last_present[s] > 1:
                n_gap += neg
            last_present[s] = k
    return n_rec, n_neg, n_gap
