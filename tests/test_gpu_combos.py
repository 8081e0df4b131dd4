"""Every pair of handle features together on the GPU: the covering table of tests/combo_cases.py, one handle per case, the ten
calls of schedule P through it, every call and stream held to the per-stream oracle (identity and shadow verdicts exactly, the float
fields within the precision64 model -- float64 handles within the float64 path's tolerances --, row means and record cells through
the checks of their own files; no tolerance of its own).  tests/test_combo_contract.py shows on the CPU that the table covers what
it says, that every decision of every case is decidable and that the oracle differs from the wrong models of every feature.

``-s`` prints per case the trace ``call:mode_used/fell_back/dense streams/records`` and at the end the worst |gpu - f64| / bound per
family (profiles/combos_worst_ratio_by_family.txt).  A case that fails is reduced by running single ids; what remains goes into
``REGRESSIONS``."""
import pytest

from pyradiotracking_amd import _native
from pyradiotracking_amd.analyze import BatchSignalAnalyzer
from tests import combo_cases as cc
from tests import sequence_cases as sq
from tests.test_gpu_float64 import family

pytestmark = pytest.mark.gpu

WORST = {}  # (family, what) -> worst ratio

#: reduced cases of defects this table found, by id
REGRESSIONS = [
    # rt_fetch with lanes into a buffer of exactly the call's size: a last lane WITHOUT records (call 5, stream 4 alone under its
    # 8 dB) was booked as "records lost" and rt_fetch_record_cells refused the call as truncated
    "256-f32-cx-sparse-l3-serial-all-perstream-cells-c0-default",
]


@pytest.fixture(autouse=True)
def _need_gpu():
    if _native.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")


def _note(c):
    fam = family(c.size) + ("" if c.path == "f32" else " " + c.path)

    def note(what, r):
        WORST[(fam, what)] = max(WORST.get((fam, what), 0.0), float(r))

    return note


def _describe(c):
    return " ".join(f"{k}={v}" for k, v in c._asdict().items())


HIP_ERROR = []  # the case that met a HIP error: nothing more is started on that GPU


def _run_case(c):
    if HIP_ERROR:
        pytest.fail(f"not run: {HIP_ERROR[0]} left a HIP error")
    sched = sq.SCHEDULES[cc.SCHEDULE]
    try:
        b = BatchSignalAnalyzer([str(i) for i in range(sq.n_streams(c.size))], sdr_callback_length=sq.max_samples(sched, c.size), **cc.handle_kwargs(c))
        try:
            runs = cc.run_handle(b, c)
        finally:
            b.close()
    except _native.NativeError as e:
        if e.code == _native.RT_E_HIP:
            HIP_ERROR.append(cc.case_id(c))
        raise AssertionError(f"{_describe(c)}: {e}") from e
    trace = sq.trace([(r.records, r.info) for r in runs])
    print(f"\n{cc.case_id(c)}: {trace}")
    try:
        n_rec, n_neg, n_gap = cc.hold(c, runs, _note(c))
    except AssertionError as e:
        raise AssertionError(f"{_describe(c)}: {e}\n trace {trace}") from None
    assert n_rec > len(sched.T) and n_neg > len(sched.T) // 2, (_describe(c), n_rec, n_neg)
    if c.presence == "gaps":
        assert n_gap >= 3, (_describe(c), n_gap)
    want = cc.expect_mode(c)
    if want is not None:
        assert all(r.info.mode_used == want for r, t in zip(runs, sched.T) if t > 0), (_describe(c), trace)
    if c.chunk and c.path == "f32" and c.size not in (16, 300):  # (the fused scans: the chunk length asked for)
        assert all(int(r.info.segs_per_chunk) == c.chunk for r in runs), (_describe(c), [int(r.info.segs_per_chunk) for r in runs])


@pytest.mark.parametrize("c", cc.CASES, ids=[cc.case_id(c) for c in cc.CASES])
def test_case(c):
    _run_case(c)


@pytest.mark.parametrize("text", REGRESSIONS)
def test_regression(text):
    _run_case(cc.case_of(text))


def test_zz_print_worst_ratios():
    """The worst |gpu - f64| / bound per family and field over the cases above (``-s`` shows it)."""
    for (fam, what), v in sorted(WORST.items()):
        print(f"combos gpu-f64 {fam:22s} {what:28s} {v:.3f}")
    assert all(v <= 1.0 for v in WORST.values())
