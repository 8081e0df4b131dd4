"""Every ordering routine of the sparse detection at its size edges, on the GPU: the cases of tests/detect_order_cases.py (that
they are what they claim: tests/test_detect_order_contract.py, on the CPU).

Per case:

* ``call_info().n_hot`` equals the planned number of listed cells -- which pins every list's length, and with it the routine and
  instantiation, on the device;
* the records equal the oracle's in (fi, start, end) and in shadow verdicts; their figures lie within the float64 round-off model
  (``precision64.check_records``) -- the four buffers of 2^26 samples, where a float64 map is out of proportion, within the 0.01 dB
  of tests/test_gpu_fullsize.py of the oracle's figures, float64 handles within the bounds of tests/test_gpu_float64_path.py;
* the records are byte-identical to those of a ``dense`` handle on the same input, which orders nothing (a map-free float64
  handle sums in another order than the dense one: identity and shadow verdicts there);
* a list of one cell more than it holds: ``sparse`` refuses the call with RT_E_HOT_OVERFLOW, ``auto`` falls back
  (``fell_back == 1``), ``f64_rescue`` re-runs the one stream (``n_dense_streams == 1``) -- with the oracle's records.

Every case runs; a case whose handle cannot be created fails.  The worst |gpu - reference| / bound per family and the times of
the 2^26 cases go to profiles/detect_order_worst_ratio.txt when the whole file has run."""
import collections
import os
import time

import numpy as np
import pytest

from pyradiotracking_amd import _native
from pyradiotracking_amd.analyze import BatchSignalAnalyzer
from tests import detect_order_cases as dc
from tests import precision64 as p64

pytestmark = pytest.mark.gpu

BIG_TOL_DB = 0.01  # tests/test_gpu_fullsize.py: POWER_TOL_DB
#: what the table's first run found (no ordering fault): a map-free float64 handle without RT_FLAG_F64_RESCUE reported n_hot = 0
#: for every call -- rt_fetch_f64 summed the streams' counters only on a handle with the flag
REGRESSIONS = ("f64-cap1024", "f64-cap1500", "f64-4096-top-bin")
TABLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "detect_order_worst_ratio.txt")
_worst = collections.OrderedDict()  # family -> {figure: worst ratio}
_times = collections.OrderedDict()  # 2^26 case -> (buffer s, oracle s, sparse handle s, dense handle s)
_ran = set()


@pytest.fixture(autouse=True)
def _need_gpu():
    if _native.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    if not _worst:
        return
    lines = ["# tests/test_gpu_detect_order.py: worst |gpu - reference| / bound per family (float32 handles: the float64 round-off model of",
             "# tests/precision64.py; border: 0.01 dB against the oracle's figures; f64: 1e-9 dB, std 1e-5 dB against the oracle's)"]
    for fam, w in _worst.items():
        lines.append(f"{fam:10s} " + "  ".join(f"{k} {v:.3f}" for k, v in w.items()))
    if _times:
        lines.append("# the buffers of 2^26 samples, seconds: planting the buffer, the oracle (STFT, row walk, list lengths), the sparse handle (create,")
        lines.append("# upload, analyse, fetch), the dense handle")
        for name, t in _times.items():
            lines.append(f"{name:22s} buffer {t[0]:6.1f}  oracle {t[1]:6.1f}  sparse {t[2]:6.1f}  dense {t[3]:6.1f}")
    text = "\n".join(lines) + "\n"
    print("\n" + text)
    if _ran >= {c.name for c in dc.CASES}:  # (a run of the whole file, not of a selection)
        try:
            with open(TABLE, "w") as f:
                f.write(text)
        except OSError:
            pass


def _note(family, figure, ratio):
    w = _worst.setdefault(family, collections.OrderedDict())
    w[figure] = max(w.get(figure, 0.0), float(ratio))


def _run(c, iq, **over):
    """One call of the case's handle -> (records, call info); ``over``: keywords that differ from the case's."""
    kw = dc.handle_kwargs(c)
    kw.update(over)
    b = BatchSignalAnalyzer([str(s) for s in range(len(c.streams))], sdr_callback_length=iq.shape[1], **kw)
    try:
        b.enqueue(iq)
        rec = b.fetch_records()
        return rec, b.call_info(), b.decoder
    finally:
        b.close()


def _dense_twin(c, iq):
    if dc.is_f64(c):
        return _run(c, iq, f64_sparse=False, f64_rescue=False, hot_capacity=0, mode="dense")[0]
    return _run(c, iq, mode="dense", group_detect=None)[0]


def _hold_to_oracle(c, rec, info, decoder, iq):
    from tests.test_gpu_float64 import form_of
    from tests.test_gpu_float64_path import DB_TOL, STD_TOL

    L = max(1, int(info.segs_per_chunk))
    for s in range(len(c.streams)):
        a = dc.analyse(c, s)
        mine = rec[rec["stream"] == s]
        what = f"{c.name} stream {s}"
        assert [(int(r["fi"]), int(r["start"]), int(r["end"])) for r in mine] == dc.rec_key(a.records), f"{what}: records differ from the oracle's"
        assert [bool(r["shadowed"]) for r in mine] == a.shadowed, f"{what}: shadow verdicts"
        if not len(mine):
            continue
        want = a.records
        if dc.is_f64(c):
            with np.errstate(divide="ignore"):
                got = (dc.oracle.to_db(mine["max_p"]), dc.oracle.to_db(mine["mean_p"]), dc.oracle.to_db(mine["row_mean"]),
                       dc.oracle.to_db(mine["mean_p"] / mine["row_mean"]), mine["std_db"])
            for name, g, w, tol in zip(("max", "avg", "noise", "snr", "std"), got, zip(*[(r.max_dbw, r.avg_dbw, r.noise_dbw, r.snr_db, r.std_db) for r in want]),
                                       (DB_TOL,) * 4 + (STD_TOL,)):
                err = np.abs(np.asarray(g, np.float64) - np.asarray(w, np.float64))
                _note(c.family, name, err.max() / tol)
                assert np.all(err <= tol), f"{what} {name}: {err.max()} dB"
        elif c.name in dc.BIG:
            _, _, _, max_dbw, avg_dbw, std_db, noise_dbw, snr_db = decoder.decode(mine)
            for name, g, w in zip(("max", "avg", "std", "noise", "snr"), (max_dbw, avg_dbw, std_db, noise_dbw, snr_db),
                                  zip(*[(r.max_dbw, r.avg_dbw, r.std_db, r.noise_dbw, r.snr_db) for r in want])):
                err = np.abs(np.asarray(g, np.float64) - np.asarray(w, np.float64))
                i = int(np.argmax(err))
                _note(c.family, name, err.max() / BIG_TOL_DB)
                assert np.all(err < BIG_TOL_DB), f"{what} {name}: record {dc.rec_key(want)[i]} {float(g[i])!r} vs {float(w[i])!r}"
        else:
            ref = p64.stft_power_f64(iq[s], dc.FS, dc.WINDOW, c.nperseg)
            bd = p64.cell_bounds(ref, form_of(c.nperseg, dc.WINDOW))
            chk = p64.check_records(mine, ref, bd, L, what=what)
            for k, v in chk.worst.items():
                _note(c.family, k, v)
            assert not chk.failures, "\n".join(chk.failures[:8])


def test_the_regressions_are_cases_of_the_table():
    assert all(n in dc.BY_NAME and dc.BY_NAME[n].expect == "records" and not dict(dc.BY_NAME[n].kw).get("f64_rescue") for n in REGRESSIONS)


@pytest.mark.parametrize("name", [c.name for c in dc.CASES])
def test_detect_order(name):
    c = dc.BY_NAME[name]
    t0 = time.perf_counter()
    iq = np.stack([dc.buffer(c, s) for s in range(len(c.streams))])
    if dc.is_f64(c):
        iq = iq.astype(np.complex128)
    t1 = time.perf_counter()
    planned = sum(sum(p.fills) for p in c.streams)
    for s in range(len(c.streams)):
        dc.analyse(c, s)  # (timed apart from the handles; cached for _hold_to_oracle)
    t2 = time.perf_counter()
    if c.expect == "overflow":
        with pytest.raises(_native.NativeError) as e:
            _run(c, iq)
        assert e.value.code == _native.RT_E_HOT_OVERFLOW, e.value
        _ran.add(name)  # (the same input in mode auto, or with f64_rescue, is a case of its own)
        return
    rec, info, decoder = _run(c, iq)
    t3 = time.perf_counter()
    if c.expect == "records":
        assert int(info.n_hot) == planned, f"{name}: {int(info.n_hot)} cells listed, {planned} planned"
        assert int(info.fell_back) == 0 and int(info.n_dense_streams) == 0, (name, info.fell_back, info.n_dense_streams)
        assert int(info.mode_used) == _native.RT_MODE_SPARSE, (name, info.mode_used)
    elif c.expect == "fell_back":
        assert int(info.fell_back) == 1, (name, info.fell_back, info.mode_used)
    else:
        assert c.expect == "rescued" and int(info.n_dense_streams) == 1 and int(info.fell_back) == 1, (name, info.n_dense_streams, info.fell_back)
    _hold_to_oracle(c, rec, info, decoder, iq)
    t4 = time.perf_counter()
    dense = _dense_twin(c, iq)
    t5 = time.perf_counter()
    if dc.is_f64(c):
        for f in ("stream", "fi", "start", "end", "shadowed"):
            assert np.array_equal(rec[f], dense[f]), f"{name}: {f} against the dense float64 handle"
    else:
        assert rec.tobytes() == dense.tobytes(), f"{name}: records differ from the dense handle's"
    if name in dc.BIG:
        _times[name] = (t1 - t0, t2 - t1, t3 - t2, t5 - t4)
    _ran.add(name)
