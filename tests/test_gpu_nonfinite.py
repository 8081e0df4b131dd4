"""NaN and Inf IQ samples on the GPU: the cases of tests/nonfinite_cases.py (one poisoned sample in stream 2 of call 0, two clean
calls behind it) through ``BatchSignalAnalyzer`` in every kernel family, every handle created with ``row_means=True,
record_cells=True``.  Per call and stream:

* records: (fi, start, end) and the shadow verdicts equal the oracle's;
* float fields: NaN exactly where the float64 restatement's are, otherwise within the precision64 model (float64 handles: within
  ``DB_TOL`` / ``STD_TOL`` of tests/test_gpu_float64_path.py) -- no tolerance of its own;
* clean twin: a second handle of the same configuration is fed the same batch without the poison; the records, row means and record
  cells of streams 0, 1, 3 and 4 are byte-identical in all three calls;
* row means of stream 2: NaN in every bin in call 0, finite in calls 1 and 2, in call 2 bit-identical to the twin's;
* record cells of stream 2: NaN exactly at the poisoned segment (a negative position for call 1's reach-backs), ``max_p`` NaN exactly
  when a cell is, every other cell bit-identical to the twin's cell of the same bin and segment wherever both deliver it;
* map (``rt_spectrogram`` / ``rt_spectrogram_f64`` on call 0's batch, once on the fresh handle and once behind the three calls): the
  poisoned column NaN in all bins, every other cell of all streams bit-identical to the twin's map -- one NaN segment must not leak into the segments that share its wave, workgroup or
  row-sum fold;
* the ragged-tail position: everything byte-identical to the twin.

Stream 2's twin.  On a handle that detrends by linearity (hamming, complex64, nperseg 32 ... 4096 unless ``subtract_first``) the guard
of that form marks a stream that meets a non-finite sample, and from then on that stream -- and only that stream -- runs on the
subtract-first kernels (rt_analyze.hip: rt_fetch).  What stream 2 is compared with bit for bit is then the clean twin created
with ``subtract_first=True`` -- which of the two it ran on is read off the map's segments far from the poisoned one --; the other
streams keep the twin of the handle's own form.

``-s`` prints at the end the worst |gpu - f64| / bound per family."""
import functools

import numpy as np
import pytest

from pyradiotracking_amd import _native
from pyradiotracking_amd.analyze import BatchSignalAnalyzer
from tests import nonfinite_cases as nf
from tests import record_cells_util as rcu
from tests import sequence_cases as sq
from tests.test_gpu_record_cells import STD_TOL_DB
from tests.test_gpu_float64 import family, form_of

pytestmark = pytest.mark.gpu

WORST = {}
T = nf.T
PREFILTER_HOPS = 8.5  # the chunk-bit pre-filter needs a minimum of 2 L hops: L = 4 there, as in tests/test_gpu_sequences.py; its cases
#                       take the layout with plateaus of 10 to 12 cells (nonfinite_cases.spans_long)


@pytest.fixture(autouse=True)
def _need_gpu():
    if _native.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")


def _note(nperseg):
    fam = family(nperseg)

    def note(what, r):
        WORST[(fam, what)] = max(WORST.get((fam, what), 0.0), float(r))

    return note


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


# ---- handles ---------------------------------------------------------------------------------------------------------------------
def _handle(nperseg, hops, fmt, **extra):
    extra = dict(extra)
    extra.pop("pipelined", None)
    per_stream = extra.pop("stream_hops", None)
    if fmt == "c128":
        extra["precision"] = "float64"
    else:
        extra.setdefault("segs_per_chunk", nf.SEGS_PER_CHUNK)
    if nperseg == 4096:
        extra["record_capacity"] = 64  # thousands of NaN records in one stream: the record room grows inside the fetch
    if nperseg >= 4096 and extra.get("mode") in ("sparse", "runfilter"):
        # a pinned sparse level refuses a call whose candidate lists overflow (RT_E_HOT_OVERFLOW, by contract): the NaN column is
        # nperseg candidate cells of one segment, which land on one list -- 8192 of them beside the tones' cells are more than the
        # default 8192 entries hold (at 4096 the exact pre-filter keeps as many again).  16384 is the largest power of two whose lists
        # fit the LDS (tests/test_gpu_sequences.py); AUTO keeps the default and climbs.
        extra["hot_capacity"] = 16384
    b = BatchSignalAnalyzer([str(i) for i in range(nf.n_streams(nperseg))], sdr_callback_length=nf.n_samples(nperseg), row_means=True,
                            record_cells=True, **nf.settings(nperseg, hops), **extra)
    if per_stream is not None:
        b.set_stream_settings(signal_min_duration_ms=[1e3 * h * sq.hop_s(nperseg) for h in per_stream])
    return b


def _run(nperseg, hops, fmt, batches, extra):
    """Three calls through one handle, then the map of call 0's batch -> ([(records, call_info, row means, offsets, cells)], map)."""
    b = _handle(nperseg, hops, fmt, **extra)
    out = []
    try:
        fresh = _map(b, batches[0], nperseg, fmt)  # before any call: no stream has met the guard of the detrend by linearity yet
        piped = extra.get("pipelined", False)
        if piped:
            b.enqueue(np.ascontiguousarray(batches[0]))
        for k in range(len(batches)):
            if piped:
                if k + 1 < len(batches):
                    b.enqueue(np.ascontiguousarray(batches[k + 1]))
            else:
                b.enqueue(np.ascontiguousarray(batches[k]))
            rec = b.fetch_records()
            info = b.native.call_info()
            rm = b.fetch_row_means()
            off, cells = b.fetch_record_cells()
            out.append((rec, info, rm, off, cells))
        spec = _map(b, batches[0], nperseg, fmt)
    finally:
        b.close()
    return out, spec, fresh


def _map(b, batch, nperseg, fmt):
    import torch

    x = np.ascontiguousarray(batch)
    S, n = x.shape
    d = torch.from_numpy(x).cuda()
    m = torch.zeros((S, n // nperseg, nperseg), dtype=torch.float64 if fmt == "c128" else torch.float32, device="cuda")
    b.native.spectrogram_device(d.data_ptr(), n, n, m.data_ptr())
    return m.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _twin(nperseg, p, hops, fmt, extra_items, layout="short"):
    """The clean twin's three calls and maps, once per configuration and layout."""
    case = nf.Case(nperseg, "nan", {0: "seg0", 7: "seg7", 8: "seg8", T - 1: "last"}[p], "first", hops, fmt, layout)
    return _run(nperseg, hops, fmt, nf.buffers(case, poisoned=False), dict(extra_items))


def _freeze(extra):
    return tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in extra.items()))


def _cells_by_position(runs, s):
    """(call, bin, segment) -> the cell's bits, over every record of stream s (a look-back cell belongs to the call before)."""
    out = {}
    for k, (rec, _, _, off, cells) in enumerate(runs):
        for i in np.flatnonzero(rec["stream"] == s):
            c = cells[off[i]:off[i + 1]]
            for j in range(len(c)):
                t = int(rec["start"][i]) + j
                out[(k, int(rec["fi"][i]), t) if t >= 0 else (k - 1, int(rec["fi"][i]), T + t)] = c[j:j + 1].tobytes()
    return out


def _stream_slices(rec, off, cells, s):
    idx = np.flatnonzero(rec["stream"] == s)
    return rec[idx], [cells[off[i]:off[i + 1]] for i in idx]


# ---- one case --------------------------------------------------------------------------------------------------------------------
def _hold(case, expect_same_mode=False, **extra):
    nperseg, fmt, hops = case.nperseg, case.fmt, case.hops
    what = f"{nf.case_id(case)} {extra}"
    S = nf.n_streams(nperseg)
    p = nf.segment_of(case.pos)
    f64 = fmt == "c128"
    form = form_of(nperseg, nf.WINDOW, extra.get("subtract_first", False)) if not f64 else "sub"
    marked = form == "lin" and p is not None  # the guard of the detrend by linearity moves stream 2 to the subtract-first kernels
    stream_hops = extra.get("stream_hops")
    with np.errstate(all="ignore"):
        if stream_hops is None:
            want = nf.oracle_case(case)
        else:
            want = [nf.oracle_clean(nperseg, nf.layout_segment(case.pos), float(h), fmt, case.layout)[s] for s, h in enumerate(stream_hops)]
            want[nf.POISONED] = nf.oracle_poisoned(case._replace(hops=float(stream_hops[nf.POISONED])))
    batches = nf.buffers(case)
    runs, spec, fresh = _run(nperseg, hops, fmt, batches, extra)
    twin_runs, twin_spec, twin_fresh = _twin(nperseg, nf.layout_segment(case.pos), hops, fmt, _freeze(extra), case.layout)
    assert _bits(twin_fresh) == _bits(twin_spec), f"{what}: the clean twin's map before and behind its calls"
    twin2_runs, twin2_spec = twin_runs, twin_spec
    if marked:
        # which kernels stream 2 ran on shows in the segments two chunks and more from the poisoned one (whether a NaN sample, which
        # the form handles like the reference, moves a stream is the guard's choice; an Inf sample has to)
        far = np.abs(np.arange(T) - p) >= 2 * nf.SEGS_PER_CHUNK
        sub = _twin(nperseg, nf.layout_segment(case.pos), hops, fmt, _freeze(dict(extra, subtract_first=True)), case.layout)
        if _bits(spec[nf.POISONED][far]) == _bits(sub[1][nf.POISONED][far]):
            twin2_runs, twin2_spec = sub[0], sub[1]
        else:
            marked = False
    print(f"\n{what}: {sq.trace([(r[0], r[1]) for r in runs])}")

    # the map: the contamination check.  On the fresh handle every stream still runs the handle's own form: the poisoned column NaN in
    # all bins, every other cell of every stream the clean twin's
    if p is None:
        assert _bits(fresh) == _bits(twin_spec), f"{what}: map on the fresh handle differs from the clean twin's"
    else:
        bad = fresh[nf.POISONED][p]
        assert np.isnan(bad).all(), f"{what}: fresh handle, column {p} of stream 2 holds {bad[~np.isnan(bad)][:4]} in bins {np.flatnonzero(~np.isnan(bad))[:8]}"
        keep = np.ones(fresh.shape[:2], bool)
        keep[nf.POISONED, p] = False
        assert _bits(fresh[keep]) == _bits(twin_spec[keep]), f"{what}: fresh handle, the NaN segment leaked into (stream, segment) {np.argwhere((fresh != twin_spec).any(axis=2) & keep)[:8].tolist()}"
    for s in range(S):
        if s != nf.POISONED or p is None:
            assert _bits(spec[s]) == _bits(twin_spec[s]), f"{what}: map of stream {s} differs from the clean twin's"
        else:
            assert np.isnan(spec[s][p]).all(), f"{what}: column {p} of stream 2 has finite cells in bins {np.flatnonzero(~np.isnan(spec[s][p]))[:8]}"
            rest = np.arange(T) != p
            assert _bits(spec[s][rest]) == _bits(twin2_spec[s][rest]), f"{what}: the NaN segment leaked into segments {sorted(set(np.argwhere(spec[s][rest] != twin2_spec[s][rest])[:, 0]))[:8]} (of the other 47)"

    twin2_cells = _cells_by_position(twin2_runs, nf.POISONED)
    n_cells_compared = 0
    for k, (rec, info, rm, off, cells) in enumerate(runs):
        trec, tinfo, trm, toff, tcells = twin_runs[k]
        L = max(1, int(info.segs_per_chunk))
        assert len(off) == len(rec) + 1 and np.array_equal(np.diff(off), rec["end"] - rec["start"]) and len(cells) == off[-1], f"{what} call {k}"
        for s in range(S):
            tag = f"{what} call {k} stream {s}"
            mine, mine_cells = _stream_slices(rec, off, cells, s)
            w = want[s][k]
            assert sq.rec_key(mine) == sq.key(w.records), f"{tag}: records differ from the oracle's\n got  {sq.rec_key(mine)[:12]}\n want {sq.key(w.records)[:12]}"
            assert [bool(v) for v in mine["shadowed"]] == w.shadowed, f"{tag}: shadow verdicts"
            x = batches[k][s]
            with np.errstate(all="ignore"):
                if f64:
                    sq.check_f64(mine, w.records)
                else:
                    nf.check_fields(mine, x, batches[k - 1][s] if k else None, nperseg, "sub" if (marked and s == nf.POISONED) else form, L, tag, _note(nperseg))
            if s != nf.POISONED or p is None:
                theirs, their_cells = _stream_slices(trec, toff, tcells, s)
                assert _bits(mine) == _bits(theirs), f"{tag}: records differ from the clean twin's"
                assert _bits(rm[s]) == _bits(trm[s]), f"{tag}: row means differ from the clean twin's"
                assert all(_bits(a) == _bits(b) for a, b in zip(mine_cells, their_cells)), f"{tag}: record cells differ from the clean twin's"
                continue
            # the poisoned stream
            if k == 0:
                assert np.isnan(rm[s]).all(), f"{tag}: finite row means in bins {np.flatnonzero(~np.isnan(rm[s]))[:8]}"
            else:
                assert np.isfinite(rm[s]).all(), f"{tag}: row means"
            if k == 2:
                assert _bits(rm[s]) == _bits(twin2_runs[k][2][s]), f"{tag}: row means differ from the clean twin's"
            for r, c in zip(mine, mine_cells):
                t = int(r["start"]) + np.arange(len(c))
                nan_at = (t == p) if k == 0 else ((t == p - T) if k == 1 else np.zeros(len(c), bool))
                assert np.array_equal(np.isnan(c), nan_at), f"{tag} bin {int(r['fi'])} [{int(r['start'])},{int(r['end'])}): NaN cells at {t[np.isnan(c)]}, due at {t[nan_at]}"
                assert bool(np.isnan(r["max_p"])) == bool(nan_at.any()), f"{tag} bin {int(r['fi'])}: max_p {r['max_p']!r}"
                for j in np.flatnonzero(~nan_at):
                    pos = (k, int(r["fi"]), int(t[j])) if t[j] >= 0 else (k - 1, int(r["fi"]), T + int(t[j]))
                    if pos in twin2_cells:
                        assert c[j:j + 1].tobytes() == twin2_cells[pos], f"{tag}: cell {pos} differs from the clean twin's"
                        n_cells_compared += 1
        if expect_same_mode and k == 2:
            assert info.mode_used == tinfo.mode_used, f"{what}: call 2 ran mode {info.mode_used}, the clean twin {tinfo.mode_used}"
    assert n_cells_compared > 10 or p is None, n_cells_compared


# ----------------------------------------------------------------------------------------------------------------------------------
# transform families, complex64: stft_scan with lane groups (32, 64, 128), 256, through the exchange rows (1024), stft_scan64 (4096),
# stft_wg (8192, 16384), stft_general (16), stft_bluestein (300); both detrend forms where the linearity form exists
# ----------------------------------------------------------------------------------------------------------------------------------
FAMILIES = [(c, "sparse", False) for c in nf.every_kind_and_position(256)]
FAMILIES += [(c, "sparse", False) for n in (32, 64, 128, 1024, 4096, 8192) for c in nf.elsewhere(n)]
FAMILIES += [(c, "sparse", True) for n in (32, 64, 128, 256, 1024, 4096) for c in nf.elsewhere(n)]
FAMILIES += [(c, "auto", False) for n in (16, 300, 16384) for c in nf.elsewhere(n)]


def _ids(rows):
    return ["-".join([nf.case_id(r[0])] + [str(v) for v in r[1:]]) for r in rows]


@pytest.mark.parametrize("case,mode,subtract_first", FAMILIES, ids=_ids(FAMILIES))
def test_transform_families(case, mode, subtract_first):
    _hold(case, mode=mode, **(dict(subtract_first=True) if subtract_first else {}))


# modes at 256 and 4096 (sparse is above).  Runfilter and AUTO take call 1's bin thresholds from the poisoned call's sums: calls 1 and
# 2 equal the oracle like call 0, and call 2 runs the mode the clean twin runs.
MODES = [(c, mode) for n in (256, 4096) for mode in ("dense", "runfilter", "auto") for c in nf.elsewhere(n)]
MODES += [(c._replace(hops=PREFILTER_HOPS, layout="long"), "prefilter") for n in (256, 4096) for c in nf.elsewhere(n)]


@pytest.mark.parametrize("case,mode", MODES, ids=_ids(MODES))
def test_modes(case, mode):
    _hold(case, expect_same_mode=True, mode=mode, **(dict(segs_per_chunk=4) if mode == "prefilter" else {}))


FORMS = [(c, dict(group_detect=True)) for n in (128, 256) for c in nf.elsewhere(n)]
FORMS += [(c, dict(lanes=lanes)) for n in (256, 128) for lanes in (2, 3) for c in nf.elsewhere(n)]
FORMS += [(c, dict(lanes=lanes, pipelined=True)) for lanes in (1, 2) for c in nf.elsewhere(256)]


@pytest.mark.parametrize("case,extra", FORMS, ids=[f"{nf.case_id(c)}-{'-'.join(f'{k}{v}' for k, v in e.items())}" for c, e in FORMS])
def test_detection_forms_lanes_and_pipelining(case, extra):
    """``pipelined``: call k + 1 is enqueued before call k is fetched -- the re-run of the marked stream then analyses the call in
    flight again as well."""
    _hold(case, mode="sparse", **extra)


F64 = [c for n in (256, 300) for c in nf.four_kinds_two_positions(n, "c128")]


@pytest.mark.parametrize("case", F64, ids=nf.case_id)
def test_float64_handles(case):
    _hold(case, mode="auto")


STREAM_HOPS = (4.0, 4.0, 1.0, 4.0, 4.0)
PER_STREAM = [c._replace(hops=1.0) for c in nf.elsewhere(256)]


@pytest.mark.parametrize("case", PER_STREAM, ids=nf.case_id)
def test_per_stream_settings(case):
    """Stream 2 with a 1-hop minimum, the others with 4 hops (``set_stream_settings``), each held to an oracle of its own."""
    _hold(case, mode="sparse", stream_hops=STREAM_HOPS)


@pytest.mark.parametrize("precision", ["float32", "float64"])
def test_caller_supplied_maps(precision):
    """``rt_extract`` / ``rt_extract_f64`` on a planted map: a NaN cell inside a plateau, one in a quiet row, one in ``last`` -- one
    cell each, not a column: only that bin's row mean is NaN."""
    import torch

    f64 = precision == "float64"
    cur, last = nf.planted_maps(np.float64 if f64 else np.float32)
    with np.errstate(all="ignore"):
        want = nf.planted_oracle(cur, last)
    S, Tm, F = cur.shape
    b = BatchSignalAnalyzer([str(i) for i in range(S)], sdr_callback_length=Tm * 256, precision=precision, record_cells=True, row_means=True,
                            **nf.settings(256, nf.PLANTED_HOPS))
    try:
        d_cur, d_last = torch.from_numpy(cur).cuda(), torch.from_numpy(last).cuda()
        b.native.extract_device(d_cur.data_ptr(), Tm, F, d_last.data_ptr(), last.shape[1])
        rec = b.fetch_records()
    finally:
        b.close()
    n_nan = 0
    for s in range(S):
        mine = rec[rec["stream"] == s]
        w = want[s]
        assert sq.rec_key(mine) == sq.key(w.records), (s, sq.rec_key(mine), sq.key(w.records))
        assert [bool(v) for v in mine["shadowed"]] == w.shadowed, s
        if f64:
            with np.errstate(all="ignore"):
                sq.check_f64(mine, w.records)
        for r, x in zip(mine, w.records):
            row = cur[s][:, x.fi]
            cells = np.concatenate((last[s][x.start:, x.fi], row[:x.end])) if x.start < 0 else row[x.start:x.end]
            assert bool(np.isnan(r["max_p"])) == bool(np.isnan(r["mean_p"])) == bool(np.isnan(r["std_db"])) == bool(np.isnan(cells).any()), (s, x)
            assert bool(np.isnan(r["row_mean"])) == bool(np.isnan(row).any()), (s, x)
            # a planted cell is taken as it is: the figures are rt::run_stats of the cells (max and mean bit for bit, tests/record_cells_util.py),
            # the row mean the float64 sum of the row rounded once and divided in the map's type (rt_core.h: row_mean_of)
            with np.errstate(all="ignore"):
                mx, mean, std = rcu.run_stats(cells)
            P = cells.dtype.type
            if not np.isnan(cells).any():
                assert r["max_p"] == mx and r["mean_p"] == mean and abs(float(r["std_db"]) - float(std)) <= STD_TOL_DB, (s, x, r, mx, mean, std)
            if not f64 and not np.isnan(row).any():  # (float32 cells: the float64 sum is exact in any order; float64 rows are held by check_f64 above)
                assert r["row_mean"] == P(row.astype(np.float64).sum()) / P(len(row)), (s, x, r["row_mean"])
            n_nan += int(np.isnan(cells).any())
    assert n_nan == 3


def oracle_cases():
    """Every case above: tests/test_nonfinite_contract.py checks their claims on the CPU."""
    out = [r[0] for r in FAMILIES] + [c for c, _ in MODES] + [c for c, _ in FORMS] + F64 + PER_STREAM
    return sorted(set(out))


def test_zz_print_worst_ratios():
    """The worst |gpu - f64| / bound per family and field over the cases above (``-s`` shows it)."""
    for (fam, what), v in sorted(WORST.items()):
        print(f"nonfinite gpu-f64 {fam:16s} {what:22s} {v:.3f}")
    assert all(v <= 1.0 for v in WORST.values())
