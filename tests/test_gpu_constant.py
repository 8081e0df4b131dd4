"""Segments that cancel exactly, on the GPU: every case of tests/constant_cases.py against the oracle.

A segment whose samples are all one value is an all-zero column in the reference (``x - mean`` is exactly zero), and a record that
starts on it has ``std = NaN``.  Per case (tests/test_constant_contract.py shows on the CPU that each holds such a record, that its
decisions are clear of the thresholds and that the detrend guard is far from marking the stream):

* records equal the oracle's in (stream, fi, start, end) and in shadow verdicts; ``max``, ``avg``, ``noise``, ``snr`` within
  POWER_TOL_DB (float64 handles: the bounds of tests/test_gpu_float64_path.py); ``std`` NaN exactly where the oracle's is and within
  ``_std_tolerance`` elsewhere.  The full-mantissa complex64 control, where the reference itself leaves a residue, is held to
  DESIGN section 2, deviation 3: NaN if and only if the kernels' own cell is zero;
* with ``record_cells`` the delivered head cell of such a record is +0.0 bit for bit and ``max(cells) == max_p``; with
  ``row_means`` an all-constant stream's means are exactly 0.0 (-inf dBW) and its neighbours' are those of a handle without it;
* int16 and int8 handles equal their complex twin (synth.i16_to_complex64 ...) byte for byte, on clipped segments as elsewhere;
* a chained handle (rt_set_chain, three links) equals the plain handle fed buffer by buffer, byte for byte.

``-s`` prints per family how many records had a NaN ``std`` on both sides, here only and in the oracle only; the table of the run
is written to profiles/constant_segments_by_family.txt."""
import collections
import os

import numpy as np
import pytest

from pyradiotracking_amd import _native
from pyradiotracking_amd.analyze import BatchSignalAnalyzer
from tests import constant_cases as cc
from tests.test_gpu_parity import POWER_TOL_DB, _std_tolerance

pytestmark = pytest.mark.gpu

F64_DB_TOL = 1e-9    # tests/test_gpu_float64_path.py: DB_TOL (max / avg / noise / snr, dB)
F64_STD_TOL = 1e-5   # tests/test_gpu_float64_path.py: STD_TOL
LINKS = 3
TABLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "constant_segments_by_family.txt")
_counts = collections.OrderedDict()  # family -> [cases, records, NaN on both sides, here only, in the oracle only]


@pytest.fixture(autouse=True)
def _need_gpu():
    if _native.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    if not _counts:
        return
    lines = ["# tests/test_gpu_constant.py: records whose std is NaN (a plateau that starts on an all-zero column), per kernel family",
             f"{'family':28s} {'cases':>5s} {'records':>7s} {'NaN both':>8s} {'here only':>9s} {'oracle only':>11s}"]
    lines += [f"{fam:28s} {v[0]:5d} {v[1]:7d} {v[2]:8d} {v[3]:9d} {v[4]:11d}" for fam, v in _counts.items()]
    text = "\n".join(lines) + "\n"
    print("\n" + text)
    if len(_counts) >= 10:  # (a run of the whole file, not of a selection)
        try:
            with open(TABLE, "w") as f:
                f.write(text)
        except OSError:
            pass


def _family(c):
    if c.precision == "float64":
        return "float64 rescue" if dict(c.extra).get("f64_rescue") else "float64 map-free" if dict(c.extra).get("f64_sparse") else "float64 dense"
    if c.fmt == "u8":
        return "uint8 (subtract-first) 256"
    if c.fmt == "c64full":
        return "complex64 full mantissa 256"
    return cc.family(c.nperseg, c.window)


def _handle(c, n_streams=cc.S, chain=0, **over):
    extra = {k: v for k, v in dict(c.extra).items() if k not in cc.NOT_HANDLE_KEYWORDS}
    extra.update(over)
    lengths = cc.layout(c)[0]
    return BatchSignalAnalyzer([str(i) for i in range(n_streams)], sdr_callback_length=max(lengths), mode=c.mode, segs_per_chunk=c.spc,
                               precision=c.precision, chain=chain, **cc.settings(c), **extra)


def _enqueue(b, c, buf, twin=False, links=None):
    kw = {} if links is None else dict(links=links)
    if twin or c.fmt in ("c64", "c64full"):
        b.enqueue(cc.as_complex(c, buf) if twin else buf, **kw)
    elif c.fmt == "u8":
        b.enqueue_bytes(buf, **kw)
    elif c.fmt == "i8":
        b.enqueue_int8(buf, **kw)
    else:
        b.enqueue_int16(buf, **kw)


def _side(b, c):
    flags = dict(c.extra)
    return (b.fetch_row_means() if flags.get("row_means") else None, b.fetch_record_cells() if flags.get("record_cells") else None)


def _run(c, twin=False, rows=None, **over):
    """[buffer] -> (records, row means or None, (offsets, cells) or None); ``rows``: only these streams, as a handle of their own"""
    bufs = [np.array(buf[rows] if rows is not None else buf) for buf in cc.wire(c.name)]  # (writable copies: the table's are shared)
    b = _handle(c, n_streams=bufs[0].shape[0], **over)
    out = []
    try:
        if dict(c.extra).get("in_flight"):
            _enqueue(b, c, bufs[0], twin)
            for k in range(len(bufs)):
                if k + 1 < len(bufs):
                    _enqueue(b, c, bufs[k + 1], twin)  # two calls in flight
                out.append((b.fetch_records(), None, None))
        else:
            for buf in bufs:
                _enqueue(b, c, buf, twin)
                rec = b.fetch_records()
                out.append((rec,) + _side(b, c))
        decoder = b.decoder
    finally:
        b.close()
    return out, decoder


def _same_bytes(got, want, what):
    for k, (g, w) in enumerate(zip(got, want)):
        parts = [("records", g[0], w[0]), ("row means", g[1], w[1])]
        if g[2] is not None:
            parts += [("cell offsets", g[2][0], w[2][0]), ("cells", g[2][1], w[2][1])]
        for name, a, b in parts:
            if a is None:
                continue
            a, b = np.asarray(a), np.asarray(b)
            assert a.dtype == b.dtype and a.shape == b.shape, f"{what} buffer {k} {name}: {a.dtype}{a.shape} vs {b.dtype}{b.shape}"
            assert a.tobytes() == b.tobytes(), f"{what} buffer {k} {name} differ"


def _figures_f32(decoder, mine, s):
    sigs = decoder.signals(mine, [str(s)] * cc.S, [cc.TS0] * cc.S)
    return [(g.max, g.avg, g.noise, g.snr, g.std) for g in sigs]


def _figures_f64(mine):
    from oracle import analyze_oracle as oracle
    with np.errstate(divide="ignore", invalid="ignore"):
        return list(zip(oracle.to_db(mine["max_p"]), oracle.to_db(mine["mean_p"]), oracle.to_db(mine["row_mean"]),
                        oracle.to_db(mine["mean_p"] / mine["row_mean"]), mine["std_db"]))


def _hold_to_oracle(c, runs, decoder):
    """every buffer and stream against constant_cases.reference; returns [records, NaN both, here only, oracle only]"""
    ref = cc.reference(c.name)
    f64 = c.precision == "float64"
    tol = F64_DB_TOL if f64 else POWER_TOL_DB
    n = [0, 0, 0, 0]
    for k, (rec, _, cells) in enumerate(runs):
        at = 0
        for s in range(cc.S):
            want = ref[k][s]
            mine = rec[rec["stream"] == s]
            what = f"{c.name} buffer {k} stream {s}"
            assert [(int(r["fi"]), int(r["start"]), int(r["end"])) for r in mine] == [(r.fi, r.start, r.end) for r in want.records], what
            assert [bool(r["shadowed"]) for r in mine] == want.shadowed, f"{what}: shadow verdicts"
            figs = _figures_f64(mine) if f64 else _figures_f32(decoder, mine, s)
            prev = ref[k - 1][s].spec if k else None
            for i, (g, r) in enumerate(zip(figs, want.records)):
                for name, mine_v, want_v in zip(("max", "avg", "noise", "snr"), g, (r.max_dbw, r.avg_dbw, r.noise_dbw, r.snr_db)):
                    assert abs(float(mine_v) - float(want_v)) < tol, f"{what} ({r.fi}, {r.start}, {r.end}) {name}: {mine_v} vs {want_v}"
                here, there = bool(np.isnan(g[4])), bool(np.isnan(r.std_db))
                n[0] += 1
                n[1] += here and there
                n[2] += here and not there
                n[3] += there and not here
                own = None
                if cells is not None:
                    own = cells[1][cells[0][at + i]: cells[0][at + i + 1]]
                    assert len(own) == r.end - r.start and own.max() == mine[i]["max_p"], what
                if c.fmt == "c64full":
                    # deviation 3: NaN if and only if a cell of the record is zero in the kernels' own map
                    assert own is not None and here == bool((own == 0.0).any()), (what, r.fi, float(g[4]), own)
                    if not here and not there:
                        assert abs(float(g[4]) - float(r.std_db)) < _std_tolerance(r, want.spec, prev), (what, r.fi)
                    continue
                assert here == there, f"{what} ({r.fi}, {r.start}, {r.end}) std: {g[4]} vs {r.std_db}"
                if there:
                    if own is not None:
                        assert own[0].tobytes() == np.zeros(1, own.dtype).tobytes(), (what, r.fi, own[0])  # +0.0, bit for bit
                else:
                    std_tol = F64_STD_TOL if f64 else _std_tolerance(r, want.spec, prev)
                    assert abs(float(g[4]) - float(r.std_db)) < std_tol, f"{what} ({r.fi}, {r.start}, {r.end}) std: {g[4]} vs {r.std_db}"
            at += len(mine)
        assert at == len(rec)
    return n


def _chained(c):
    """the case's six buffers through a handle of LINKS links, re-read as the plain handle's: [buffer] -> records"""
    bufs = cc.wire(c.name)
    b = _handle(c, chain=LINKS)
    out = []
    try:
        for call in range(len(bufs) // LINKS):
            _enqueue(b, c, np.concatenate(bufs[call * LINKS: (call + 1) * LINKS], axis=1), links=LINKS)
            rec = b.fetch_records()
            for j in range(LINKS):
                mine = rec[rec["stream"] % LINKS == j].copy()
                mine["stream"] //= LINKS
                out.append(mine)
    finally:
        b.close()
    return out


@pytest.mark.parametrize("name", [c.name for c in cc.CASES])
def test_constant_segment(name):
    c = cc.BY_NAME[name]
    runs, decoder = _run(c)
    counts = _hold_to_oracle(c, runs, decoder)
    row = _counts.setdefault(_family(c), [0, 0, 0, 0, 0])
    row[0] += 1
    for i, v in enumerate(counts):
        row[1 + i] += int(v)
    expect = cc.layout(c)[3]
    if c.fmt != "c64full":
        assert counts[1] >= len(expect) and counts[2] == counts[3] == 0, counts
    if c.fmt in ("i16", "i8"):
        twin, _ = _run(c, twin=True)
        _same_bytes(runs, twin, f"{name} against its complex twin:")
    if c.placement == "c":
        assert len(cc.wire(name)) == 2 * LINKS
        for k, (mine, (want, _, _)) in enumerate(zip(_chained(c), runs)):
            assert mine.tobytes() == want.tobytes(), f"{name} buffer {k} (call {k // LINKS} link {k % LINKS}): chained against plain"
    if dict(c.extra).get("f64_rescue"):
        # the clipped stream is the rescued one: every call re-runs exactly one stream, and a handle without the target none
        for rows, n_rescued in ((None, 1), ([s for s in range(cc.S) if s != cc.TARGET], 0)):
            bufs = [np.array(buf[rows] if rows is not None else buf) for buf in cc.wire(name)]
            b = _handle(c, n_streams=bufs[0].shape[0])
            try:
                for k, buf in enumerate(bufs):
                    _enqueue(b, c, buf)
                    b.fetch_records()
                    info = b.call_info()
                    assert (int(info.n_dense_streams), bool(info.fell_back)) == (n_rescued, bool(n_rescued)), (name, k, rows, info.n_dense_streams, info.fell_back)
            finally:
                b.close()
    if c.placement in ("e_zero", "e_rail"):
        others = [s for s in range(cc.S) if s != cc.TARGET]
        alone, _ = _run(c, rows=others)
        for k, ((_, means, _), (_, means_alone, _)) in enumerate(zip(runs, alone)):
            assert means[cc.TARGET].tobytes() == np.zeros(c.nperseg, means.dtype).tobytes(), (name, k)
            assert means[others].tobytes() == means_alone.tobytes(), (name, k, "the neighbours' means depend on the constant stream")
        b = _handle(c)
        try:
            _enqueue(b, c, np.array(cc.wire(name)[0]))
            b.fetch_records()
            with np.errstate(divide="ignore"):
                dbw = b.fetch_row_means(dbw=True)
        finally:
            b.close()
        assert np.isneginf(dbw[cc.TARGET]).all() and np.isfinite(dbw[others]).all(), name
