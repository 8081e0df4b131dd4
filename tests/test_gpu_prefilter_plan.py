"""What the two run-length pre-filter levels keep, cell for cell, on the GPU: the cases of tests/prefilter_plan_cases.py (that they
are what they claim: tests/test_prefilter_plan_contract.py, on the CPU).

Per case and call:

* ``call_info()``: ``mode_used`` is the level asked for (an AUTO handle: the exact level it climbed to), ``fell_back`` is 0 -- 1 on the
  two planned overflows --, ``segs_per_chunk`` is the chunk length planned through ``hc_choose_chunk``;
* ``call_info().n_hot`` equals the planned number of emitted cells EXACTLY -- the set ``need`` bits of ``plan_runs`` on the exact
  level, the candidate cells inside needed (chunk, bin) words on the chunk-bit level.  A planner that keeps too much gives the same
  records and another count; one that keeps too little is caught here wherever the missing cell lies, not only under a record;
* the records equal the oracle's per stream -- (fi, start, end), shadow verdicts, the dB figures within 0.01 dB -- and those of a
  ``dense`` handle on the same calls byte for byte; a laned handle's equal the one-lane handle's, count and bytes.

Every case runs; none is skipped.  The counts go to profiles/prefilter_plan_counts.txt when the whole file has run."""
import collections
import os

import numpy as np
import pytest

from pyradiotracking_amd import _native
from pyradiotracking_amd.analyze import BatchSignalAnalyzer
from tests import detect_order_cases as dc
from tests import prefilter_plan_cases as pc

pytestmark = pytest.mark.gpu

TOL_DB = 0.01  # tests/test_gpu_fullsize.py: POWER_TOL_DB
#: cases that pin a defect the table's first runs found (none: every count was the planned one)
REGRESSIONS = ()
TABLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "prefilter_plan_counts.txt")
_counts = collections.OrderedDict()  # case -> [(planned, reported, share of the segments kept)]
_worst = {}                          # figure -> worst |gpu - oracle| in dB
HIP_ERROR = []                       # the case that met a HIP error: nothing more is started on that GPU

Info = collections.namedtuple("Info", "n_hot mode_used fell_back n_dense_streams segs_per_chunk")


@pytest.fixture(autouse=True)
def _need_gpu():
    if _native.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")


def _feed(b, c, k):
    x = pc.batch(c, k)
    if c.fmt == "i16":
        b.enqueue_int16(x)
    elif c.fmt == "u8":
        b.enqueue_bytes(x)
    else:
        b.enqueue(x)


def _run(c, skip=(), **over):
    """The case's calls through one handle -> {call: (records, Info)}; ``over``: keywords that differ from the case's."""
    if HIP_ERROR:
        pytest.fail(f"not run: {HIP_ERROR[0]} left a HIP error")
    kw = pc.handle_kwargs(c)
    kw.update(over)
    out = {}
    try:
        b = BatchSignalAnalyzer([str(s) for s in range(pc.n_streams(c))], sdr_callback_length=pc.max_samples(c), **kw)
        try:
            for k, call in enumerate(c.calls):
                if k in skip:
                    continue
                if call.present is not None:
                    b.set_present(call.present)
                _feed(b, c, k)
                rec = b.fetch_records()
                i = b.call_info()
                out[k] = (rec, Info(int(i.n_hot), int(i.mode_used), int(i.fell_back), int(i.n_dense_streams), int(i.segs_per_chunk)), b.decoder)
        finally:
            b.close()
    except _native.NativeError as e:
        if e.code == _native.RT_E_HIP:
            HIP_ERROR.append(c.name)
        raise AssertionError(f"{c.name} ({c.edge}): {e}") from e
    return out


def _hold_to_oracle(c, k, rec, decoder):
    for s in range(pc.n_streams(c)):
        a = pc.analyse(c.name, k, s)
        mine = rec[rec["stream"] == s]
        what = f"{c.name} call {k} stream {s}"
        assert [(int(r["fi"]), int(r["start"]), int(r["end"])) for r in mine] == dc.rec_key(a.records), f"{what}: records differ from the oracle's"
        assert [bool(r["shadowed"]) for r in mine] == a.shadowed, f"{what}: shadow verdicts"
        if not len(mine):
            continue
        _, _, _, max_dbw, avg_dbw, std_db, noise_dbw, snr_db = decoder.decode(mine)
        for name, g, w in zip(("max", "avg", "std", "noise", "snr"), (max_dbw, avg_dbw, std_db, noise_dbw, snr_db),
                              zip(*[(r.max_dbw, r.avg_dbw, r.std_db, r.noise_dbw, r.snr_db) for r in a.records])):
            err = np.abs(np.asarray(g, np.float64) - np.asarray(w, np.float64))
            i = int(np.argmax(err))
            _worst[name] = max(_worst.get(name, 0.0), float(err.max()))
            assert np.all(err < TOL_DB), f"{what} {name}: record {dc.rec_key(a.records)[i]} {float(g[i])!r} vs {float(w[i])!r}"


def _share_kept(c, k):
    """Planned share of the call's segments that the selective scan transforms again (rows that keep a cell)."""
    rows = total = 0
    for s in range(pc.n_streams(c)):
        if pc.present(c, k, s):
            rows += int(pc.planned_cells(c, k, s).any(axis=0).sum())
            total += c.calls[k].T
    return rows / max(total, 1)


def test_the_regressions_are_cases_of_the_table():
    assert all(n in pc.BY_NAME for n in REGRESSIONS)


@pytest.mark.parametrize("name", [c.name for c in pc.CASES])
def test_prefilter_plan(name):
    c = pc.BY_NAME[name]
    planned = pc.planned_counts(c)
    level = {"runfilter": _native.RT_MODE_RUNFILTER, "auto": _native.RT_MODE_RUNFILTER, "prefilter": _native.RT_MODE_PREFILTER}[c.level]
    L = pc.chunk_len(c)
    got = _run(c)
    rows = _counts[name] = []  # (kept for the table whatever the assertions below say)
    for k, call in enumerate(c.calls):
        rec, info, decoder = got[k]
        what = f"{name} call {k} ({c.edge})"
        print(f"{what}: planned {planned[k]} reported {info.n_hot} mode {info.mode_used} fell_back {info.fell_back} dense streams {info.n_dense_streams} L {info.segs_per_chunk}")
        rows.append((planned[k], info.n_hot, _share_kept(c, k)))
        assert info.mode_used == level, (what, info)
        assert info.fell_back == (1 if call.expect in ("climb", "overflow") else 0), (what, info)
        assert info.n_dense_streams == (1 if call.expect == "overflow" else 0), (what, info)
        assert info.segs_per_chunk == L, (what, info, L)
        d = info.n_hot - planned[k]
        assert d == 0, f"{what}: kept {abs(d)} {'more' if d > 0 else 'fewer'} cells than planned ({info.n_hot} reported, {planned[k]} planned)"
        _hold_to_oracle(c, k, rec, decoder)
    twin = dict(segs_per_chunk=L)
    dense = _run(c, mode="dense", **twin)
    for k in range(len(c.calls)):
        assert got[k][0].tobytes() == dense[k][0].tobytes(), f"{name} call {k}: records differ from the dense handle's"
    if dict(c.kw).get("lanes", 1) > 1:
        one = _run(c, lanes=1, **twin)
        for k in range(len(c.calls)):
            assert got[k][0].tobytes() == one[k][0].tobytes() and got[k][1].n_hot == one[k][1].n_hot, f"{name} call {k}: two lanes against one"
    if c.level == "auto":
        # the exact level asked for by name: the same count on every call that it can hold (the planned overflow it refuses)
        over = [k for k, call in enumerate(c.calls) if call.expect == "overflow"]
        pinned = _run(c, skip=over, mode="runfilter")
        for k in pinned:
            assert pinned[k][1].n_hot == got[k][1].n_hot and pinned[k][1].mode_used == level, (name, k, pinned[k][1], got[k][1])


def test_zz_write_the_counts():
    """profiles/prefilter_plan_counts.txt, once every case has run (``-s`` shows it)"""
    lines = ["# tests/test_gpu_prefilter_plan.py: per case and call the candidate cells planned from the stated rules and reported by call_info().n_hot,",
             "# and the planned share of the call's segments that the selective second scan transforms again"]
    for name, rows in _counts.items():
        for k, (want, have, share) in enumerate(rows):
            lines.append(f"{name:26s} call {k}  planned {want:6d}  reported {have:6d}  segments kept {100.0 * share:6.2f} %")
    lines.append("# worst |gpu - oracle| of the records' figures, dB: " + "  ".join(f"{k} {v:.2e}" for k, v in sorted(_worst.items())))
    text = "\n".join(lines) + "\n"
    print("\n" + text)
    if set(_counts) >= {c.name for c in pc.CASES}:  # (a run of the whole file, not of a selection)
        with open(TABLE, "w") as f:
            f.write(text)
    assert all(want == have for rows in _counts.values() for want, have, _ in rows)
