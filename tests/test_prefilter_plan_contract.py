"""The cases of tests/prefilter_plan_cases.py against the oracle and the host build alone (no GPU): that the fed samples put exactly
the planned cells over the threshold, clear of it; that MODE 6's per-bin thresholds stay out of the way; that the Python rule is the
planner's (``hc_plan_runs``, word for word); that the table reaches every edge it claims, found by brute force from its tones; and
that the table is sharp: each of six planted faults changes the planned count of at least one case -- while two of them, the
over-keeping ones, leave the records untouched, which is why the records alone could not see them."""
import collections

import numpy as np
import pytest

from oracle import analyze_oracle as oracle
from tests import detect_order_cases as dc
from tests import prefilter_plan_cases as pc

NAMES = [c.name for c in pc.CASES]
RUN = [c.name for c in pc.CASES if c.level != "prefilter"]
PRE = [c.name for c in pc.CASES if c.level == "prefilter"]
TINY = ("run-64-T10-r2", "run-256-T2-r9", "run-256-T16-r17")  # buffers of a few segments: no duty rule (prefilter_plan_cases._TinyLayout)


def _streams(c, k):
    return [s for s in range(pc.n_streams(c)) if pc.present(c, k, s)]


def test_the_edges_are_the_librarys():
    """rows of threshold bits, planner instantiations and the rows a wave may hold, as the table assumes them"""
    assert [pc.lane_group(n) for n in (64, 128, 256, 1024, 2048, 4096)] == [4, 8, 16, 64, 128, 256]
    assert [(pc.words(n), pc.tiles_per_wave(n)) for n in (64, 128, 256, 1024, 2048, 4096)] == [(1, 64), (2, 32), (4, 16), (16, 4), (32, 2), (64, 1)]
    hot, need = np.zeros(300, np.uint64), np.zeros(300, np.uint64)
    assert [pc._hc().hc_plan_runs(hot.ctypes.data, need.ctypes.data, 300, 1, r, 0) for r in (2, 16, 17, 256, 257)] == [pc.planner_of(r) for r in (2, 16, 17, 256, 257)] == [4, 4, 8, 8, 16]
    for T in (pc.ROWS_PER_WAVE, pc.ROWS_PER_WAVE + 1, 20000, 25599):  # kPlanRowsPerWave: no wave holds more rows, and at r = 100 it alone asks for a second
        B, wave, _, _ = pc.borders(64, T, 100)
        assert wave <= pc.ROWS_PER_WAVE and -(-T // wave) == -(-T // pc.ROWS_PER_WAVE), (T, B, wave)
    for n in (64, 128, 256, 1024, 2048, 4096):  # every (column, bit) of a row holds one bin
        col, bit = pc.bin_slot(n)
        assert len({(int(a), int(b)) for a, b in zip(col, bit)}) == n and col.max() == pc.words(n) - 1 and bit.max() == 63


@pytest.mark.parametrize("name", NAMES)
def test_the_fed_samples_hold_the_planned_bits_clear_of_every_threshold(name):
    c = pc.BY_NAME[name]
    thr_db = pc.FORMATS[c.fmt][0]
    thr = oracle.db_to_linear(thr_db)
    snr = oracle.db_to_linear(pc.SNR_DB)
    clear_db = 40.0 if c.fmt == "c64" else 6.0  # (quantised input: half a step of dither lies 20 .. 30 dB under the threshold)
    L = pc.chunk_len(c)
    assert L == (c.L or L) and (c.level != "prefilter" or pc.prefilter_ok(c)), (name, L)
    if c.level == "auto":
        assert not pc.prefilter_ok(c), "the exact level must be the next one up"
    for k, call in enumerate(c.calls):
        for s in _streams(c, k):
            _, _, spec = pc.spec(name, k, s)
            hot = pc.plan_bits(c, k, s)
            what = f"{name} call {k} stream {s}"
            assert spec.shape == hot.shape, (what, spec.shape)  # (a ragged tail makes no segment)
            assert np.array_equal(spec >= thr, hot), f"{what}: the threshold bits are not the planned ones"
            with np.errstate(divide="ignore"):
                quiet = float(oracle.to_db(spec[hot].min())) if hot.any() else np.inf
                loud = float(oracle.to_db(spec[~hot].max()))
            assert quiet >= thr_db + clear_db and loud <= thr_db - clear_db, (what, quiet, loud)
            means = spec.mean(axis=1, dtype=np.float64)
            if hot.any():
                ratio_db = oracle.to_db(spec[hot] / np.broadcast_to(means[:, None], spec.shape)[hot])
                # (a buffer of two segments: a bin hot in one of them stands 3.01 dB over its row's mean, one hot in both 0 dB: 2 dB and
                # 1 dB from the threshold of 1 dB, and no buffer of two can do better)
                assert float(np.abs(ratio_db - pc.SNR_DB).min()) >= (0.99 if name in TINY else 3.0), (what, "a hot cell near the SNR threshold")
                assert name in TINY or float(ratio_db.min()) > pc.SNR_DB, what
            if name not in TINY:
                assert hot.sum(axis=1).max() * pc.DUTY <= call.T, (what, "a bin hot in more than an eighth of the segments")
            # one tone at a time, the cell before it included
            on = np.zeros(call.T + 1, int)
            for f, t0, n, _ in call.streams[s]:
                on[max(t0 - 1, 0):t0 + n] += 1
            assert on.max() <= 1 or name in TINY, (what, "two tones at a time")
            if c.level == "prefilter":
                continue
            # MODE 6's per-bin thresholds: far under every hot cell, and under snr x this buffer's row mean (after_bit_scan's check)
            theta, src = pc.theta_table(c, k, s, lambda kk, ss: pc.spec(name, kk, ss)[2])
            if hot.any():
                floor = np.where(hot, spec, np.inf).min(axis=1)
                assert (theta * 10.0 ** 0.6 <= floor).all(), (what, src, "theta within 6 dB of a hot cell")
            # 0.1 dB (2.3 %): the kernels' float32 sums over up to 2^15 cells differ from these float64 ones by 2^15 x 2^-24 = 2e-3 at the very most
            assert (theta[1:] * 10.0 ** 0.01 <= snr * means[1:]).all(), (what, src, float((theta[1:] / (snr * means[1:])).max()), "theta over snr x row mean: the call would be re-analysed")
            # bin 0 is round-off (prefilter_plan_cases.theta_table): from the buffer itself a minimum under the mean, from the buffer before
            # held against a row mean that a tone's segments raise
            assert theta[0] * (100.0 if src != k else 10.0 ** 0.01) <= snr * means[0], (what, src, theta[0], means[0])


@pytest.mark.parametrize("name", NAMES)
def test_every_list_fits_where_it_should(name):
    c = pc.BY_NAME[name]
    cap = pc.hot_cap(c)
    for k, call in enumerate(c.calls):
        fill, s = pc.bucket_fill(c, k)
        if call.expect == "overflow":
            streams = [x for x in range(pc.n_streams(c)) if max(int(pc.planned_cells(c, k, x)[b::16].sum()) for b in range(16)) > cap]
            assert streams == [s] and 4 * len(streams) <= pc.n_streams(c), (name, k, streams)  # one stream, a quarter of the batch: it alone is analysed again
        else:
            assert fill <= cap, (name, k, fill, cap)
        if call.expect == "climb":
            assert pc.sparse_fill(c, k) > cap, (name, k)
        elif c.level == "auto":
            assert call.expect == "overflow" or pc.sparse_fill(c, k) <= 16 * cap  # (AUTO stays on its level for sixteen calls, whatever the sparse level could hold)
    assert c.level != "auto" or [k.expect for k in c.calls][:2] == ["climb", "count"]


def _words(c, hot):
    """bool [nperseg, T] -> the planner's rows, uint64 [T, w]."""
    col, bit = pc.bin_slot(c.nperseg)
    out = np.zeros((hot.shape[1], pc.words(c.nperseg)), np.uint64)
    for f in np.flatnonzero(hot.any(axis=1)):
        out[hot[f], col[f]] |= np.uint64(1) << np.uint64(bit[f])
    return out


@pytest.mark.parametrize("name", RUN)
def test_the_rule_is_the_host_planners(name):
    """need = C[t] | C[t + 1] as stated, the tile walk restated in Python and hc_plan_runs (plan_tile_column at the call's own w, r
    and tile rows) agree word for word"""
    c = pc.BY_NAME[name]
    counts = pc.planned_counts(c)
    for k, call in enumerate(c.calls):
        total = 0
        for s in _streams(c, k):
            hot = pc.plan_bits(c, k, s)
            r, B = pc.run_cells(c, call.T), pc.tile_rows(c, call.T)
            need = pc.runfilter_need(hot, r)
            assert np.array_equal(pc.tile_walk(hot, r, B), need), (name, k, s, "the restated tile walk")
            rows = _words(c, hot)
            got = np.zeros_like(rows)
            planes = pc._hc().hc_plan_runs(rows.ctypes.data, got.ctypes.data, call.T, pc.words(c.nperseg), c.r, 0)
            assert planes == pc.planner_of(r)
            assert np.array_equal(got, _words(c, need)), (name, k, s, "hc_plan_runs")
            total += int(sum(bin(int(v)).count("1") for v in got.ravel() if v))
        assert total == counts[k], (name, k, total, counts[k])


def _edges_of(c):
    """The run-length edges a RUNFILTER case holds, by brute force from its tones and the library's tiling:
    {(kind, tile | wave)} and {(r, split)}."""
    kinds, splits = set(), set()
    for k, call in enumerate(c.calls):
        r = pc.run_cells(c, call.T)
        B, wave, tile_b, wave_b = pc.borders(c.nperseg, call.T, r)
        for s in _streams(c, k):
            for f, t0, n, _ in call.streams[s]:
                end = t0 + n  # first row after the run
                for b, where in [(b, "tile") for b in tile_b] + [(b, "wave") for b in wave_b]:
                    if n == r and end == b:
                        kinds.add(("end-last", where))
                    if n == r and t0 == b:
                        kinds.add(("start-first", where))
                    if n == r and t0 < b < end:
                        kinds.add(("split", where))
                        splits.add((r, b - t0))
                    if t0 < b and end - 1 == b + r - 1:
                        kinds.add(("halo-last", where))
                    if t0 < b and end - 1 == b + r:
                        kinds.add(("halo-past", where))
    return kinds, splits


def test_the_table_reaches_every_edge():
    run = [pc.BY_NAME[n] for n in RUN]
    # every (family, planner instantiation) pair: rows of 1 .. 64 words under counters of 4, 8 and 16 planes
    pairs = {(c.nperseg, pc.planner_of(pc.run_cells(c, k.T))) for c in run for k in c.calls}
    missing = [(n, p) for n in (64, 128, 256, 1024, 2048, 4096) for p in (4, 8, 16) if (n, p) not in pairs]
    assert not missing, missing
    assert {pc.planner_of(r) for r in (2, 9, 16)} == {4} and {pc.planner_of(r) for r in (17, 256)} == {8} and pc.planner_of(257) == 16
    assert {2, 9, 16, 17, 256, 257} <= {c.r for c in run}
    cols, bits = collections.defaultdict(set), set()
    for c in run:
        col, bit = pc.bin_slot(c.nperseg)
        for k, call in enumerate(c.calls):
            for s in _streams(c, k):
                for f, _, _, _ in call.streams[s]:
                    cols[c.nperseg].add(int(col[f]))
                    bits.add(int(bit[f]))
                    if c.nperseg == 4096:
                        cols["lanes"].add(f % 64)
    for n in (64, 128, 256, 1024, 2048, 4096):
        assert cols[n] == set(range(pc.words(n))), (n, sorted(set(range(pc.words(n))) - cols[n]))
    assert bits == set(range(64)), sorted(set(range(64)) - bits)
    assert cols["lanes"] == set(range(64))  # nperseg 4096: an edge in bins of every lane of stft_scan64
    # every border edge at a tile border and at a wave border
    kinds, splits = set(), set()
    for c in run:
        a, b = _edges_of(c)
        kinds |= a
        splits |= b
    missing = [(kind, where) for kind in ("end-last", "start-first", "split", "halo-last", "halo-past") for where in ("tile", "wave") if (kind, where) not in kinds]
    assert not missing, missing
    for r in (2, 9, 16, 17, 256, 257):  # a run of r split over a border at every split
        assert {(r, k) for k in range(1, r)} <= splits, (r, sorted(set(range(1, r)) - {k for rr, k in splits if rr == r}))
    # per geometry case: its own tile and wave borders both carry the edges (4096: one tile a wave, every border a wave's)
    for n in (64, 128, 256, 1024, 2048, 4096):
        c = next(c for c in run if c.name.startswith(f"run-{n}-") and c.r == 9 and len(_edges_of(c)[0]) >= 5)
        have, _ = _edges_of(c)
        for where in ("tile", "wave") if n != 4096 else ("wave",):
            assert {(kind, where) for kind in ("end-last", "start-first", "split", "halo-last", "halo-past")} <= have, (c.name, where, sorted(have))
        assert {(9, k) for k in range(1, 9)} <= _edges_of(c)[1], c.name
    # the buffer's ends, r > T, the tiling's ends
    tones = {(c.name, k, s, t.t0, t.r) for c in run for k, call in enumerate(c.calls) for s in _streams(c, k) for t in call.streams[s]}
    e = pc.BY_NAME["ends-256-r9"]
    assert {("ends-256-r9", 0, 0, 0, 1), ("ends-256-r9", 0, 1, 0, 8), ("ends-256-r9", 0, 2, 1, 8), ("ends-256-r9", 0, 0, 691, 9), ("ends-256-r9", 0, 1, 692, 8)} <= tones
    assert pc.BY_NAME["ends-256-r9-ragged"].calls[0].tail % 256 and e.calls[0].tail == 0
    assert pc.run_cells(pc.BY_NAME["run-256-T2-r9"], 2) == 3 and pc.run_cells(pc.BY_NAME["run-256-T16-r17"], 16) == 17
    B, wave, tile_b, _ = pc.borders(64, 10, 2)
    assert B == 1 and wave == 64  # ten of the wave's 64 one-row tiles lie inside the buffer
    seq = pc.BY_NAME["sequence-256"]
    Ts = [k.T for k in seq.calls]
    assert len(Ts) >= 6 and any(a < b for a, b in zip(Ts, Ts[1:])) and any(a > b for a, b in zip(Ts, Ts[1:])) and 0 in pc.planned_counts(seq)
    col = pc.bin_slot(256)[0]
    kept = [[(s, t.bin) for s, ts in enumerate(k.streams) for t in ts if t.r >= 9 or t.t0 == 0] for k in seq.calls]  # the kept runs of every call
    for a, b in zip(kept, kept[1:]):  # the bins move: no (stream, bin) serves two calls in a row, and the runs' word columns come in another order
        assert not set(a) & set(b) and (not a or not b or [int(col[f]) for _, f in a] != [int(col[f]) for _, f in b])
    assert {int(col[f]) for ks in kept for _, f in ks} == {0, 1, 2, 3}
    # PREFILTER: a needed chunk at 255, 256 and 257, a partial last chunk, nperseg 256 / 1024 / 4096
    big = pc.BY_NAME["pre-256-L4-chunks300"]
    full = {t.t0 // 4 for s in big.calls[0].streams for t in s if t.t0 % 4 == 0 and t.r >= 4}
    assert {255, 256, 257} <= full and big.calls[0].T // 4 > 256
    assert {c.nperseg for c in pc.CASES if c.level == "prefilter"} == {256, 1024, 4096}
    assert all(c.calls[0].T % pc.chunk_len(c) for c in pc.CASES if c.name in ("pre-256-L4", "pre-1024-L4", "pre-4096-L4", "pre-256-L32"))
    assert pc.chunk_len(pc.BY_NAME["pre-256-L32"]) == 32 and pc.BY_NAME["pre-256-L32"].L == 0  # the library's own choice


@pytest.mark.parametrize("name", PRE)
def test_the_chunk_rule_tells_the_two_border_conventions_apart(name):
    """the cold cell under a chunk's lowest segment: planned for the upper chunk (what stft_scan and stft_scan64 do); the other
    convention would count differently in every PREFILTER case that plants it"""
    c = pc.BY_NAME[name]
    if name == "pre-256-L4-chunks300":
        return
    L = pc.chunk_len(c)
    for k in range(len(c.calls)):
        mine = sum(int(pc.prefilter_emit(pc.plan_bits(c, k, s), L).sum()) for s in _streams(c, k))
        other = sum(int(pc.prefilter_emit(pc.plan_bits(c, k, s), L, lower_emits=True).sum()) for s in _streams(c, k))
        assert mine == pc.planned_counts(c)[k] and mine != other, (name, k, mine, other)
        # a run of 2 L - 2 cells that covers no aligned chunk emits nothing: why the level asks for 2 L - 1
        for s in _streams(c, k):
            for t in c.calls[k].streams[s]:
                if t.r == 2 * L - 2 and t.t0 % L == 1:
                    assert not pc.planned_cells(c, k, s)[t.bin].any(), (name, k, s)


def _record_keys(c, k, s):
    return sorted(dc.rec_key(pc.analyse(c.name, k, s).records))


@pytest.mark.parametrize("name", NAMES)
def test_the_oracles_records_are_the_planned_plateaus(name):
    """... found again from the planned cells alone; no shadow verdict hangs on two maxima, and every record's first cell is noise"""
    c = pc.BY_NAME[name]
    n = 0
    for k, call in enumerate(c.calls):
        for s in _streams(c, k):
            a = pc.analyse(name, k, s)
            assert _record_keys(c, k, s) == pc.records_from_cells(c, k, s, pc.planned_cells(c, k, s)), (name, k, s)
            mx = np.array([r.max_dbw for r in a.records], np.float64)  # (records that touch in time differ by 1e-3 dB and more)
            lo, hi = np.array([r.start for r in a.records]), np.array([r.end for r in a.records])
            near = (np.abs(mx[:, None] - mx[None, :]) < 1e-3) & (lo[:, None] <= hi[None, :] + 1) & (lo[None, :] <= hi[:, None] + 1)
            np.fill_diagonal(near, False)
            assert not near.any(), (name, k, s)
            n += len(a.records)
    assert n > 0 or name in TINY, name


@pytest.mark.parametrize("fault", pc.FAULTS)
def test_the_table_is_sharp(fault):
    """each planted fault changes the planned count of at least one case"""
    caught = []
    for c in pc.CASES:
        if (fault == "spread_two") != (c.level == "prefilter"):
            continue
        if fault == "stale_need" and len(c.calls) < 2:
            continue
        want, got = pc.planned_counts(c), pc.planned_counts(c, fault)
        if want != got:
            caught.append((c.name, [b - a for a, b in zip(want, got)]))
    assert caught, fault
    print(f"{fault}: caught by {len(caught)} cases, first {caught[:3]}")
    if fault in ("halo_short", "before_clear", "drop_at_tile_end"):
        assert any(d < 0 for _, ds in caught for d in ds), (fault, "an under-keeping fault")
    else:
        assert all(d >= 0 for _, ds in caught for d in ds), (fault, "an over-keeping fault")


@pytest.mark.parametrize("fault", ("stale_need", "keep_all"))
def test_records_cannot_see_a_planner_that_keeps_too_much(fault):
    """the gap this table closes: a need word left over from the call before, or a planner that keeps every threshold cell, gives
    the oracle's records in every case -- and a different count (test_the_table_is_sharp)"""
    seen = 0
    for c in pc.CASES:
        if c.level == "prefilter" or (fault == "stale_need" and len(c.calls) < 2):
            continue
        carried = [None] * pc.n_streams(c)
        for k in range(len(c.calls)):
            for s in _streams(c, k):
                cells = pc.planned_cells(c, k, s, fault, carried[s])
                carried[s] = cells
                seen += int(cells.sum()) - int(pc.planned_cells(c, k, s).sum())
                assert pc.records_from_cells(c, k, s, cells) == _record_keys(c, k, s), (fault, c.name, k, s)
    assert seen > 0, fault
