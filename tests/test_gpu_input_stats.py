"""rt_set_input_stats / rt_fetch_input_stats on the GPU: every format on float32 and float64 handles at the sizes where the kernels
take another path (nothing, one sample, less than a segment, around the chunk length, several chunks and a ragged end), with a row
stride that alternates the rows' alignment and with the pointer advanced by one sample; the accumulator widths; float input with
every special value against the float64 round-off bound; the same bytes across pointer shifts, lanes, the _host entries and runs;
the presence mask, chained handles, two calls in flight, every refusal, AUTO's level-up; the analysis byte for byte with the feature
on and off; the Python layer.  The model and the rows: tests/input_stats_cases.py.

profiles/input_stats_worst_ratio.txt holds the worst |sum - fsum| / bound per format (written with RT_WRITE_PROFILES=1)."""
import ctypes as C
import datetime
import os

import numpy as np
import pytest

from pyradiotracking_amd import _native, build
from pyradiotracking_amd.analyze import BatchSignalAnalyzer, SignalAnalyzer, input_levels
from tests import input_stats_cases as isc
from tests import int16_cases as ic

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 3
WORST = {}
ENTRY = {"c64": "rt_process", "c128": "rt_process", "u8": "rt_process_u8", "i16": "rt_process_i16", "i8": "rt_process_i8"}
FED = {"c64": "c", "c128": "c", "u8": "u8", "i16": "i16", "i8": "i8"}
F32_FORMATS = ("u8", "i8", "i16", "c64")
F64_FORMATS = ("u8", "i8", "i16", "c128")


@pytest.fixture(autouse=True)
def _need_gpu():
    if _native.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")


@pytest.fixture(scope="module")
def chunk():
    lib = C.CDLL(build.build_hostcheck())
    lib.hc_input_stats_chunk.restype = C.c_int
    return int(lib.hc_input_stats_chunk())


_ROWS = {}


def _row_and_model(fmt, n, seed, chunk):
    """a random row and its model, made once for all the handle kinds that take it"""
    key = (fmt, n, seed)
    if key not in _ROWS:
        row = isc.random_row(fmt, n, seed, chunk)
        row.setflags(write=False)
        _ROWS[key] = (row, isc.model_row(fmt, row))
    return _ROWS[key]


def _handle(max_samples, n_streams=S, stats=True, **kw):
    kw.setdefault("fft_nperseg", 256)
    # (full-range random input: a threshold no cell reaches keeps the detection -- which the rows do not depend on -- out of the way;
    # the map-free float64 path would otherwise overflow its candidate lists and deliver no call at all)
    kw.setdefault("signal_threshold_dbw", 60.0)
    return BatchSignalAnalyzer([str(i) for i in range(n_streams)], sdr_callback_length=max_samples, input_stats=stats, **kw)


class Feed:
    """Rows on the device: ``rows`` [S][2 n] components, laid out with ``stride`` samples per row behind ``shift`` samples of
    padding (the block itself is 256-byte aligned, so ``shift`` decides the first row's alignment and ``stride`` the others')."""

    def __init__(self, fmt, rows, stride=None, shift=0):
        self.fmt, self.n = fmt, len(rows[0]) // 2
        self.stride = self.n if stride is None else stride
        comps = np.zeros((shift + len(rows) * self.stride + 1) * 2, dtype=isc.DTYPE[fmt])
        for s, r in enumerate(rows):
            comps[2 * (shift + s * self.stride):][:2 * self.n] = r
        self.host = comps[2 * shift:]  # (a view: the _host entries read the same layout)
        self.buf = _native.DeviceBuffer(0, max(comps.nbytes, 16))
        self.buf.upload(comps)
        self.ptr = self.buf.ptr + shift * isc.SAMPLE_BYTES[fmt]

    def enqueue(self, b, host=False):
        nat = b._native
        fn = getattr(nat._lib, ENTRY[self.fmt] + ("_host" if host else ""))
        nat._check(fn(nat._handle, self.host.ctypes.data if host else self.ptr, self.n, self.stride))
        nat._fed.append(FED[self.fmt])


def _stats(b, feed, host=False):
    feed.enqueue(b, host)
    b.fetch_records()
    return b.fetch_input_stats()


def _formats(b):
    return F64_FORMATS if b.precision == "float64" else F32_FORMATS


KINDS = {"float32": {}, "float64": dict(precision="float64"), "float64 sparse": dict(precision="float64", f64_sparse=True)}


@pytest.mark.parametrize("kind", list(KINDS))
def test_sizes_and_alignments_against_the_model(chunk, kind):
    """Every format the handle takes, n_samples nothing ... 3 C + 17, rows n + 1 samples apart (consecutive rows alternate their
    alignment), once more with the pointer one sample on: integer formats field for field, float sums within the bound, and the
    shifted run the same bytes."""
    b = _handle(3 * chunk + 18, **KINDS[kind])
    try:
        for fmt in _formats(b):
            for n in isc.sizes(chunk):
                rows, models = zip(*(_row_and_model(fmt, n, 10 + s, chunk) for s in range(S)))
                seen = []
                for shift in (0, 1):
                    got = _stats(b, Feed(fmt, rows, stride=n + 1, shift=shift))
                    for s in range(S):
                        r = isc.compare(fmt, got[s], models[s], f"{kind} {fmt} n={n} shift={shift} stream {s}")
                        WORST[fmt] = max(WORST.get(fmt, 0.0), r)
                    seen.append(got.tobytes())
                assert seen[0] == seen[1], (kind, fmt, n)
    finally:
        b.close()


def test_accumulator_widths(chunk):
    """Every component at -32768, at 255, at 0 and at -128 over 3 C + 17 samples: no thread's, wave's or chunk's partial wraps."""
    n = 3 * chunk + 17
    b = _handle(n)
    try:
        for fmt, value in (("i16", -32768), ("u8", 255), ("u8", 0), ("i8", -128)):
            rows = [isc.constant_row(fmt, n, value)] * S
            got = _stats(b, Feed(fmt, rows, stride=n + 1))
            for s in range(S):
                isc.compare(fmt, got[s], isc.model_row(fmt, rows[s]), f"{fmt} all {value}")
            assert int(got[0]["n_rail"]) == 2 * n
    finally:
        b.close()


def test_a_megasample_of_int16_rails():
    """One stream of 2^20 samples of (-32768, -32768): sum_sq = 2^51 exactly."""
    n = 1 << 20
    b = _handle(n, n_streams=1)
    try:
        got = _stats(b, Feed("i16", [isc.constant_row("i16", n, -32768)]))[0]
        assert (int(got["n_samples"]), int(got["n_rail"]), float(got["sum_i"]), float(got["sum_q"]), float(got["sum_sq"]), float(got["peak"])) == \
               (n, 2 * n, -float(2 ** 35), -float(2 ** 35), float(2 ** 51), 32768.0)
    finally:
        b.close()


@pytest.mark.parametrize("fmt", ["c64", "c128"])
def test_float_input_with_every_special_value(chunk, fmt):
    """0.3 * Gaussian with +-1.0, 1.5, -0.0, a denormal, NaN, +Inf and -Inf planted: counts and peak exact, the sums within
    (m + 1) 2^-53 fsum(|terms|) of fsum."""
    n = 3 * chunk + 17
    b = _handle(n, **(KINDS["float64"] if fmt == "c128" else {}))
    try:
        rows = [isc.random_row(fmt, n, 20 + s, chunk) for s in range(S)]
        got = _stats(b, Feed(fmt, rows, stride=n + 1))
        for s in range(S):
            m = isc.model_row(fmt, rows[s])
            assert m["n_nonfinite"] == 3 and m["n_rail"] >= 8 and m["peak"] == 1.5
            r = isc.compare(fmt, got[s], m, f"{fmt} stream {s}")
            WORST[fmt + " specials"] = max(WORST.get(fmt + " specials", 0.0), r)
        # nothing but non-finite components: counted, and nothing else
        nan_rows = [isc.constant_row(fmt, 200, v) for v in (np.nan, np.inf, -np.inf)]
        got = _stats(b, Feed(fmt, nan_rows))
        for s in range(S):
            assert (int(got[s]["n_nonfinite"]), int(got[s]["n_rail"]), float(got[s]["sum_i"]), float(got[s]["sum_sq"]), float(got[s]["peak"])) == (400, 0, 0.0, 0.0, 0.0)
    finally:
        b.close()


def test_the_same_bytes_across_lanes_entries_and_runs(chunk):
    """5 streams on 1, 2 and 3 lanes, the device entry and the _host entry, the pointer shifted, twice each: one set of bytes."""
    n, S5 = 2 * chunk + 301, 5
    for fmt in ("c64", "u8", "i16"):
        rows = [isc.random_row(fmt, n, 30 + s, chunk) for s in range(S5)]
        seen = {}
        for lanes in (1, 2, 3):
            b = _handle(n + 2, n_streams=S5, lanes=lanes)
            try:
                for shift, host in ((0, False), (1, False), (0, True), (0, False)):
                    seen[(lanes, shift, host, len(seen))] = _stats(b, Feed(fmt, rows, stride=n + 1, shift=shift), host).tobytes()
            finally:
                b.close()
        assert len(set(seen.values())) == 1, (fmt, [k for k, v in seen.items() if v != next(iter(seen.values()))])
        got = np.frombuffer(next(iter(seen.values())), dtype=_native.INPUT_STATS_DTYPE)
        for s in range(S5):
            isc.compare(fmt, got[s], isc.model_row(fmt, rows[s]), f"{fmt} lanes stream {s}")
    # a float64 handle: complex128 from the device and from the host
    rows = [isc.random_row("c128", n, 40 + s, chunk) for s in range(S)]
    b = _handle(n + 2, precision="float64")
    try:
        got = [_stats(b, Feed("c128", rows, stride=n + 1), host).tobytes() for host in (False, True, False)]
        assert got[0] == got[1] == got[2]
    finally:
        b.close()


@pytest.mark.parametrize("kind", ["float32", "float64"])
def test_presence_mask(chunk, kind):
    """An absent stream: n_samples 0, zero sums, format and unit set; the present rows as without a mask."""
    n = chunk + 100
    b = _handle(n, **KINDS[kind])
    try:
        rows = [isc.random_row("u8", n, 50 + s, chunk) for s in range(S)]
        full = _stats(b, Feed("u8", rows))
        b.set_present([True, False, True])
        got = _stats(b, Feed("u8", rows))
        assert got[0].tobytes() == full[0].tobytes() and got[2].tobytes() == full[2].tobytes()
        gone = got[1]
        assert [int(gone[f]) for f in ("n_samples", "n_rail", "n_nonfinite", "format", "unit")] == [0, 0, 0, 1, 255]
        assert [float(gone[f]) for f in ("sum_i", "sum_q", "sum_sq", "peak")] == [0.0] * 4
        assert np.isnan(input_levels(got)[1]["power_dbfs"]) and not np.isnan(input_levels(got)[0]["power_dbfs"])
        b.set_present(None)
        assert _stats(b, Feed("u8", rows)).tobytes() == full.tobytes()
    finally:
        b.close()


def test_chained_handle_every_link_is_a_stream(chunk):
    B = chunk + 256
    b = BatchSignalAnalyzer(["a", "b"], sdr_callback_length=B, chain=2, input_stats=True)
    try:
        raw = np.stack([isc.random_row("u8", 2 * B, 60 + r, chunk) for r in range(2)])
        b.enqueue_bytes(raw)
        b.fetch_records()
        got = b.fetch_input_stats()
        assert got.shape == (4,)
        for r in range(2):
            for link in range(2):
                isc.compare("u8", got[2 * r + link], isc.model_row("u8", raw[r, 2 * B * link:2 * B * (link + 1)]), f"run {r} link {link}")
    finally:
        b.close()


def _refused(b, word):
    with pytest.raises(_native.NativeError) as e:
        b.fetch_input_stats()
    assert e.value.code == _native.RT_E_INVALID and word in str(e.value), str(e.value)


def test_two_calls_in_flight_and_every_refusal(chunk):
    n = chunk + 77
    b = _handle(n)
    try:
        nat = b._native
        _refused(b, "no call delivered")
        f0, f1 = (Feed("i16", [isc.random_row("i16", n, 70 + 10 * k + s, chunk) for s in range(S)]) for k in (0, 1))
        want = [[isc.model_row("i16", f.host[2 * s * n:2 * (s + 1) * n]) for s in range(S)] for f in (f0, f1)]
        f0.enqueue(b)
        f1.enqueue(b)
        # pending calls: the switch is refused, and nothing is delivered yet
        with pytest.raises(_native.NativeError) as e:
            b.set_input_stats(False)
        assert e.value.code == _native.RT_E_INVALID and "pending" in str(e.value)
        _refused(b, "no call delivered")
        b.fetch_records()
        got = b.fetch_input_stats()  # process k, process k + 1, fetch k, stats k
        for s in range(S):
            isc.compare("i16", got[s], want[0][s], "call 0")
        assert b.fetch_input_stats().tobytes() == got.tobytes()  # (again: a copy)
        b.fetch_records()
        got = b.fetch_input_stats()
        for s in range(S):
            isc.compare("i16", got[s], want[1][s], "call 1")
        # a wrong n, a null output
        out = np.zeros(S + 1, dtype=_native.INPUT_STATS_DTYPE)
        assert nat._lib.rt_fetch_input_stats(nat._handle, out.ctypes.data, S + 1) == _native.RT_E_INVALID
        assert nat._lib.rt_fetch_input_stats(nat._handle, out.ctypes.data, S - 1) == _native.RT_E_INVALID
        assert nat._lib.rt_fetch_input_stats(nat._handle, None, S) == _native.RT_E_INVALID
        assert not out.view(np.uint8).any()
        # the next rt_process invalidates; so does rt_reset
        f0.enqueue(b)
        _refused(b, "no call delivered")
        b.fetch_records()
        b.fetch_input_stats()
        b.reset()
        _refused(b, "no call delivered")
        # off: refused; a call enqueued while it was off has none, also once the feature is on again
        b.set_input_stats(False)
        _refused(b, "off")
        f0.enqueue(b)
        b.fetch_records()
        _refused(b, "off")
        b.set_input_stats(True)
        _refused(b, "before the feature was on")  # (the delivered call was enqueued while it was off)
        f1.enqueue(b)
        b.fetch_records()
        got = b.fetch_input_stats()
        for s in range(S):
            isc.compare("i16", got[s], want[1][s], "after on again")
    finally:
        b.close()


def test_turned_on_between_calls_and_an_extract_call(chunk):
    """A handle made without the feature: call 0 is enqueued and fetched, the feature turned on, and call 0 has no rows; call 1
    has.  An rt_extract call has none either."""
    n = chunk
    b = _handle(n, stats=False)
    try:
        f = Feed("u8", [isc.random_row("u8", n, 90 + s, chunk) for s in range(S)])
        f.enqueue(b)
        b.fetch_records()
        _refused(b, "off")
        b.set_input_stats(True)
        _refused(b, "before the feature was on")
        got = _stats(b, f)
        b.set_input_stats(True)  # (again: rt_set_input_stats ends the validity of what was delivered, as rt_reset does)
        _refused(b, "before the feature was on")
        got = _stats(b, f)
        for s in range(S):
            isc.compare("u8", got[s], isc.model_row("u8", f.host[2 * s * n:2 * (s + 1) * n]), "call 1")
    finally:
        b.close()
    a = SignalAnalyzer("0", sample_rate=300000, sdr_callback_length=256 * 40, input_stats=True)
    try:
        freqs = np.fft.fftfreq(256, 1 / 300000)
        times = np.arange(40) * 256 / 300000
        a.extract_signals(freqs, times, np.full((256, 40), 1e-12, np.float32), datetime.datetime(2024, 1, 1))
        assert a.input_stats is None
        with pytest.raises(_native.NativeError) as e:
            a._batch.fetch_input_stats()
        assert e.value.code == _native.RT_E_INVALID and "rt_extract" in str(e.value)
    finally:
        a._batch.close()


def test_auto_level_up_inside_the_fetch_delivers_the_first_pass_rows():
    """int16_cases' "near" variant: the sparse lists overflow and AUTO analyses the call again inside rt_fetch; the rows are those of
    the enqueue, and the records those of a twin without the feature."""
    raw = ic.buffer_of(ic.modes_wire("near"), 0, ic.M_BLEN)
    kw = dict(sdr_callback_length=ic.M_BLEN, mode="auto", segs_per_chunk=4, record_capacity=2048, **ic.modes_kwargs("near"))
    devices = [str(i) for i in range(raw.shape[0])]
    b, twin = BatchSignalAnalyzer(devices, input_stats=True, **kw), BatchSignalAnalyzer(devices, **kw)
    try:
        b.enqueue_int16(raw)
        twin.enqueue_int16(raw)
        rec, want = b.fetch_records(), twin.fetch_records()
        assert b.call_info().fell_back == 1 and rec.tobytes() == want.tobytes() and len(rec) > 0
        got = b.fetch_input_stats()
        for s in range(raw.shape[0]):
            isc.compare("i16", got[s], isc.model_row("i16", raw[s]), f"stream {s}")
    finally:
        b.close()
        twin.close()


def _products(b):
    rec = b.fetch_records()
    means = b.fetch_row_means()
    offsets, cells = b.fetch_record_cells()
    o2, first, samples = b.fetch_record_iq()
    return [np.asarray(x).tobytes() for x in (rec, means, offsets, cells, o2, first, samples)], len(rec)


@pytest.mark.parametrize("nperseg,mode,precision", [(256, "sparse", "float32"), (256, "dense", "float32"), (256, "auto", "float32"), (4096, "sparse", "float32"),
                                                    (4096, "dense", "float32"), (4096, "auto", "float32"), (256, "auto", "float64")])
def test_the_analysis_is_untouched(nperseg, mode, precision):
    """A twin without the feature: records, row means, record cells and record IQ byte for byte, over two consecutive buffers."""
    raw_all = ic.wire(nperseg, "hamming")
    kw = dict(sdr_callback_length=ic.BLEN, mode=mode, row_means=True, record_cells=True, record_iq=True, record_iq_margin=1, precision=precision,
              **ic.kwargs(nperseg, "hamming"))
    devices = [str(i) for i in range(raw_all.shape[0])]
    b, twin = BatchSignalAnalyzer(devices, input_stats=True, **kw), BatchSignalAnalyzer(devices, **kw)
    try:
        total = 0
        for k in range(ic.N_BUF):
            raw = ic.buffer_of(raw_all, k)
            for x in (b, twin):
                x.enqueue_int16(raw)
            got, n = _products(b)
            want, _ = _products(twin)
            assert got == want, (nperseg, mode, precision, k)
            total += n
            stats = b.fetch_input_stats()
            for s in range(raw.shape[0]):
                isc.compare("i16", stats[s], isc.model_row("i16", raw[s]), f"buffer {k} stream {s}")
        assert total > 20
    finally:
        b.close()
        twin.close()


def test_the_python_layer(chunk):
    """``fetch_input_stats`` (above), ``SignalAnalyzer.input_stats`` through the four ``process_*`` methods, ``input_levels``."""
    n = 256 * 40
    rng = np.random.default_rng(7)
    ts = datetime.datetime(2024, 1, 1)
    a = SignalAnalyzer("0", sample_rate=300000, sdr_callback_length=n, input_stats=True)
    plain = SignalAnalyzer("0", sample_rate=300000, sdr_callback_length=n)
    try:
        assert a.input_stats is None and plain.input_stats is None
        x = (0.2 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
        x[5] = 1.0 + 0.0j
        a.analyze_buffer(x, ts)
        isc.compare("c64", a.input_stats, isc.model_row("c64", x.view(np.float32)), "analyze_buffer")
        lv = input_levels(a.input_stats)[0]
        assert lv["power_dbfs"] == pytest.approx(10 * np.log10(np.mean(np.abs(x.astype(np.complex128)) ** 2)), abs=1e-9)
        assert lv["rail_fraction"] == pytest.approx(1 / (2 * n)) and lv["peak"] == pytest.approx(float(np.max(np.abs(x.view(np.float32)))))
        for fmt, method in (("u8", a.process_bytes), ("i16", a.process_int16), ("i8", a.process_int8)):
            raw = isc.random_row(fmt, n, 100, chunk)
            method(raw, None)
            isc.compare(fmt, a.input_stats, isc.model_row(fmt, raw), method.__name__)
        a.process_samples(x, None)
        isc.compare("c64", a.input_stats, isc.model_row("c64", x.view(np.float32)), "process_samples")
        plain.analyze_buffer(x, ts)
        assert plain.input_stats is None
    finally:
        a._batch.close()
        plain._batch.close()


def test_zz_write_the_worst_ratios():
    """(last in the file: what the tests above saw on this GPU)"""
    assert WORST
    lines = ["rt_fetch_input_stats on the GPU against math.fsum: worst |sum - fsum| / ((m + 1) 2^-53 fsum(|terms|)) per format",
             "(integer formats are compared for equality: 0)"]
    lines += [f"{name:16s} {WORST[name]:.6f}" for name in sorted(WORST)]
    text = "\n".join(lines) + "\n"
    print(text)
    assert max(WORST.values()) <= 1.0
    if os.environ.get("RT_WRITE_PROFILES"):
        with open(os.path.join(REPO, "profiles", "input_stats_worst_ratio.txt"), "w") as f:
            f.write(text)
