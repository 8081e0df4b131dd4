"""The cases of tests/detect_order_cases.py against the oracle alone (no GPU): that every list has the planned length, that the
restated switches send it to the intended routine, that the table reaches every routine and instantiation, that no decision is
near a threshold -- and that the table is sharp: a walker over the ordered lists reproduces the oracle's records, and under each
of three planted faults it does not.

The buffers of 2^26 samples (``BIG``) are the slow ones: about ten seconds each on a desktop CPU for the buffer, the oracle's map
and its row walk, so each is analysed once and its checks share that."""
import numpy as np
import pytest

from tests import detect_order_cases as dc

K = dc.constants()
NAMES = [c.name for c in dc.CASES]
WALKED = [c.name for c in dc.CASES if c.expect == "records" and c.name not in dc.BIG]


def test_the_edges_are_the_librarys():
    """the constants the restated switches use are rt_core.h's (hc_detect_order_constants), not copies"""
    assert K == dc.Consts(buckets=16, small_bucket=1024, group_cells=896, group_bins=256, quarters=4, cand_cap_max=64)
    assert (K.small_bucket - K.group_cells) * 8 // 4 == K.group_bins  # the group's row means lie behind its cells
    assert [dc.key_tbits(n) for n in (2048, 2049, 16384, 16385, 1 << 18, (1 << 18) + 1)] == [11, 12, 14, 15, 18, 19]


@pytest.mark.parametrize("name", NAMES)
def test_lists_are_as_planned_and_clear_of_the_thresholds(name):
    c = dc.BY_NAME[name]
    for s, plan in enumerate(c.streams):
        a = dc.analyse(c, s)
        assert a.fills == plan.fills, f"{name} stream {s}: cells per bucket"
        assert a.runs == plan.plateaus, f"{name} stream {s}: records per bucket"
        assert len(a.records) == sum(plan.plateaus)
        # every planted cell and every other cell at least 40 dB from the threshold, every SNR decision 3 dB from its own
        assert a.quietest_hot_db >= dc.THRESHOLD_DBW + 40.0 and a.loudest_cold_db <= dc.THRESHOLD_DBW - 40.0, (name, s, a.quietest_hot_db, a.loudest_cold_db)
        assert a.snr_margin_db >= 3.0, (name, s, a.snr_margin_db)
        # no shadow verdict hangs on the last bits of two maxima: records that overlap in time differ by 1e-3 dB and more
        mx = np.array([r.max_dbw for r in a.records], np.float64)
        lo = np.array([r.start for r in a.records])
        hi = np.array([r.end for r in a.records])
        near = (np.abs(mx[:, None] - mx[None, :]) < 1e-3) & (lo[:, None] <= hi[None, :] + 1) & (lo[None, :] <= hi[:, None] + 1)
        np.fill_diagonal(near, False)
        assert not near.any(), (name, s, np.argwhere(near)[:4])
        if name in dc.BIG:  # (the walker's check here, while the buffer's analysis is at hand)
            assert dc.walk(c, s) == sorted(dc.rec_key(a.records)), f"{name} stream {s}: the walker's records"


def _intended(c):
    """family -> the routines its cases are there for"""
    return {"bitmap": {"bitmap", "packed"}, "packed": {"packed"}, "border": {"packed", "regs", "large"}, "large": {"large", "packed", "bitmap", "overflow"},
            "group": {"group_packed", "packed", "bitmap", "overflow"}, "plateaus": {"bitmap", "packed", "large"}, "f64": {"f64_lds", "overflow"}}[c.family]


@pytest.mark.parametrize("name", NAMES)
def test_the_restated_switch_names_the_intended_routine(name):
    c = dc.BY_NAME[name]
    per = dc.routines(c, [p.fills for p in c.streams])
    flat = [r for rs in per for r in rs]
    assert flat and {r[0] for r in flat} <= _intended(c), (name, flat)
    hb = dc._bits(c.nperseg // K.buckets)
    tbits = dc.key_tbits(c.T)
    got = set(flat)
    if name == "bitmap-256-T2048":
        assert hb + tbits == 15 and got == {("packed", 1)} | {("bitmap", m) for m in (2, 4, 8, 16)}
        assert any(t.bin == 255 and t.t0 + t.r == c.T for t in c.streams[0].tones)  # bin 255, segment 2047: every key bit set
    if name == "bitmap-256-T2049":
        assert hb + tbits == 16 and got == {("packed", m) for m in (1, 2, 4, 8, 16)}
    if c.family == "packed":
        assert 15 < hb + tbits and hb + tbits + 10 <= 32 and c.T & (c.T - 1) and got == {("packed", m) for m in (1, 2, 4, 8, 16)}
    if c.family == "border":
        full = c.T * c.nperseg == 1 << 26
        assert (hb + tbits + 10 == 32) if full else (hb + tbits + 10 == 33 and (c.T - 1) * c.nperseg == 1 << 26)
        assert got == {("packed" if full else "regs", m) for m in (1, 2, 4, 8, 16)} | {("large", 2048)}
        assert any(t.bin == c.nperseg - 1 and t.t0 + t.r == c.T - 1 for t in c.streams[0].tones)  # the top bin through segment T - 2
    if c.family == "group":
        totals = [sum(p.fills) for p in c.streams]
        for t, rs, p in zip(totals, per, c.streams):
            grouped = dc.group_can(c.nperseg, c.T) and t <= K.group_cells and max(p.fills) <= dc.hot_cap(c)
            assert (rs == [("group_packed", max(64, dc.next_pow2(t)) // 64)]) == grouped, (name, t, rs)
        if name == "group-256-T16384":
            assert dc._bits(c.nperseg) + tbits + 10 == 32
        if name == "group-256-T16385":
            assert not dc.group_can(c.nperseg, c.T)
    if c.expect in ("overflow", "fell_back", "rescued"):
        assert ("overflow", 0) in got, name
        over = [max(p.fills) if not dc.is_f64(c) else sum(p.fills) for p in c.streams]
        assert max(over) == dc.hot_cap(c) + 1  # one cell more than a list holds
    else:
        assert ("overflow", 0) not in got, name


def test_every_routine_and_instantiation_is_reached():
    reached = set()
    for c in dc.CASES:
        for rs in dc.routines(c, [p.fills for p in c.streams]):
            reached.update(rs)
    missing = [r for r in dc.ALL_ROUTINES if r not in reached]
    assert not missing, missing
    # ... and at its edges: a list of exactly 64 M cells (no padding: the 0xFFFFFFFF sentinel's neighbours are real words) and of one more
    fills = {}
    for c in dc.CASES:
        for p, rs in zip(c.streams, dc.routines(c, [p.fills for p in c.streams])):
            if dc.is_f64(c) or (rs and rs[0][0] == "group_packed"):
                fills.setdefault(rs[0], set()).add(sum(p.fills))
            else:
                for n in p.fills:
                    if n:
                        fills.setdefault(dc.bucket_routine(c.nperseg, c.T, n, dc.hot_cap(c)), set()).add(n)
    for routine in ("bitmap", "packed", "regs", "group_packed"):
        for m in (1, 2, 4, 8, 16):
            if (routine, m) not in dc.ALL_ROUTINES:
                continue
            full = 64 * m if (routine, m) != ("group_packed", 16) else K.group_cells
            have = fills[(routine, m)]
            assert full in have, (routine, m, sorted(have))
            if m > 1:
                assert 64 * (m // 2) + 1 in have, (routine, m, sorted(have))  # the shortest list of this instantiation
    assert {1025, 1500, 2048, 2049, 4096, 4097, 8192} <= set().union(*(fills[("large", n2)] for n2 in (2048, 4096, 8192)))
    assert {1023, 1024} <= fills[("f64_lds", 1024)] and {1025, 1500} <= fills[("f64_lds", 2048)]
    # plateaus per bucket around the staging area (cand_cap 32 up to 32 bins a bucket, kCandCapMax beyond)
    for c in (dc.BY_NAME["plateaus-256"], dc.BY_NAME["plateaus-1024"]):
        cap = 32 if c.nperseg // K.buckets <= 32 else K.cand_cap_max
        counts = set(c.streams[0].plateaus)
        assert {cap, cap + 1} <= counts and 2 * K.cand_cap_max + 1 in counts, (c.name, cap, counts)


@pytest.mark.parametrize("name", WALKED)
def test_a_walker_over_the_ordered_lists_finds_the_oracles_records(name):
    c = dc.BY_NAME[name]
    for s in range(len(c.streams)):
        assert dc.walk(c, s) == sorted(dc.rec_key(dc.analyse(c, s).records)), f"{name} stream {s}"


@pytest.mark.parametrize("fault", [f for f in dc.FAULTS if f])
def test_the_table_is_sharp(fault):
    """a routine that drops the last cell of a list of exactly 64 M, compares its words as signed integers, or builds its keys
    with one time bit too few changes the records of at least one case (the slow 2^26 buffers are not needed for any of the three)"""
    caught = []
    for c in dc.CASES:
        if c.expect != "records" or c.name in dc.BIG:
            continue
        for s in range(len(c.streams)):
            if dc.walk(c, s, fault) != sorted(dc.rec_key(dc.analyse(c, s).records)):
                caught.append((c.name, s))
    assert caught, fault
    print(f"{fault}: caught by {len(caught)} (case, stream) pairs, first {caught[:3]}")
