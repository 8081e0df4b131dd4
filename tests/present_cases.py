"""Streams that sit out a call (``rt_set_present``): schedules with a presence table, on top of tests/sequence_cases.py.

The schedules, buffers and tones are those of ``sequence_cases``; a pattern adds ``present[k][s]``.  In the reference every SDR is
a ``SignalAnalyzer`` of its own, called when its radio delivers: the oracle side is ``sequence_cases.oracle_run`` restated so that
an absent (call, stream) pair is skipped -- no ``stft_power``, ``last[s]`` untouched (``oracle_run``).  The schedule's tones make
that visible without anything new: tone i of stream s is hot on the last ``d`` segments of buffer j - 1 and on the first ``e`` of
buffer j, for every j -- so a stream present at call a and next at call b > a + 1 holds the tail of boundary a + 1 in its last
present buffer and the head of boundary b in its next one, in the same bin: ONE reach-back record of ``d + e`` cells across the
gap (``gap_records``).

Two wrong models of an absent stream are restated as well, and tests/test_present_contract.py holds every pattern apart from both:

* ``zeros_reset``  today's runner: the absent row is analysed as zeros and the stream's next buffer starts without look-back;
* ``lockstep``     the handle's one rotation and one segment count: the stream's next buffer looks back into the BATCH's previous
                   call -- the stream's own row of it, which the scan did not write, modelled as the cold map of an absent call
                   with that call's segment count.

The rows of absent streams hold poison (``poisoned``): NaN samples on complex input, a full-scale tone on the wire formats."""
import functools

import numpy as np

from oracle import analyze_oracle as oracle
from tests import sequence_cases as sq

# ---- presence tables -------------------------------------------------------------------------------------------------------------
# Schedule A: 13 calls of T = 96 70 96 33 96 9 64 2 96 0 40 96 70 segments, five streams.  A gap must end on a call whose time axis
# holds the walk's stop cell: the reference reads ``times[d + 1]`` of the CURRENT buffer (sequence_cases: reach), and a schedule's
# tones reach back up to 33 segments out of a long buffer.  So no gap may end on the calls of 33, 9 or 2 segments unless the buffer
# before the gap is short itself -- which moves the patterns a little from the plainest ones:
#   stream 0  always present (but for the call every stream sits out);
#   stream 1  absent on single calls: 1, 5, 7 (and 11);
#   stream 2  absent two calls running (2, 3), then three (5, 6, 7), then three again (9, 10, 11): four running, closed by a
#             present call, do not fit thirteen calls beside that rule (the stream would have to be present at calls 3 and 7) --
#             schedule C's table has them;
#   stream 3  absent on the first call, on the empty call (9) and on the call after it;
#   stream 4  absent whenever (k + 1) % 3 == 0, and at call 3 as well: present there, its gap would end on the 33-segment call;
#   call 11   every stream absent; call 12 closes every stream's gap.
# test_present_contract.py runs the oracle over every pattern and would show the IndexError.
ALL_ABSENT_CALL = 11


def _table_a():
    n, S = len(sq.A_T), 5
    p = np.ones((n, S), bool)
    p[[1, 5, 7], 1] = False
    p[[2, 3], 2] = False
    p[[5, 6, 7], 2] = False
    p[[9, 10, 11], 2] = False
    p[[0, 9, 10], 3] = False
    for k in range(n):
        if (k + 1) % 3 == 0:
            p[k, 4] = False
    p[3, 4] = False
    p[ALL_ABSENT_CALL, :] = False
    return p


# Schedule P: 10 calls of T = 47 47 47 33 35 9 47 0 41 47 segments (tests/combo_cases.py).  Every gap ends on call 2, 4, 6, 8 or 9:
# 41 or 47 segments hold the stop cell of the deepest reach-back (33) whatever buffer lies before the gap, and the 35 of call 4
# that of a gap from call 1 or 2 (at most 33 cells deep: times[34]):
#   stream 0  always present (but for the call every stream sits out);
#   stream 1  absent on single calls: 1, (3,) 7 -- the empty call;
#   stream 2  absent three calls running (3, 4, 5), then two (7, 8);
#   stream 3  absent on the first call and on the call of 9 segments (5);
#   stream 4  absent whenever (k + 1) % 3 == 0 (2, 5, 8): its last gap looks back into its own empty buffer of call 7;
#   call 3    every stream absent.
# combo_cases.EVENTS: stream 2's SNR threshold changes before call 4, which it sits out; stream 1 is reset before call 6, present.
P_ALL_ABSENT_CALL = 3


def _table_p():
    p = np.ones((len(sq.SCHEDULES["P"].T), 5), bool)
    p[[1, 7], 1] = False
    p[[3, 4, 5, 7, 8], 2] = False
    p[[0, 5], 3] = False
    p[[2, 5, 8], 4] = False
    p[P_ALL_ABSENT_CALL, :] = False
    return p


def _table_regular(n, S):
    """Schedules of equal lengths (B, B10): stream 0 always present, 1 absent on single calls, 2 two / three / four running,
    3 on the first call and two in the middle, 4 whenever (k + 1) % 3 == 0; the last call but one with every stream absent."""
    p = np.ones((n, S), bool)
    p[[2, 6], 1] = False
    p[[1, 2], 2] = False
    p[[4, 5, 6], 2] = False
    if n > 12:
        p[[8, 9, 10, 11], 2] = False
    p[[0, 4, 5], 3] = False
    for k in range(n):
        if (k + 1) % 3 == 0:
            p[k, 4] = False
    p[n - 2, :] = False
    return p


def _table_c():
    """Schedule C (72 calls of 64 segments; the floor rises in calls 2 .. 5, stream 1 alone is noisy in calls 9 and 10): stream 1
    absent through the noisy calls 2 .. 5, so that it meets the raised floor -- and thresholds of the exact pre-filter made from an
    older buffer of its own -- never; streams 2 .. 4 as in the regular table, stretched over the quiet tail."""
    n, S = sq.C_CALLS, 5
    p = np.ones((n, S), bool)
    p[[2, 3, 4, 5], 1] = False
    p[[7, 8], 2] = False
    p[[20, 21, 22], 2] = False
    p[[40, 41, 42, 43], 2] = False
    p[[0, 12, 13], 3] = False
    for k in range(n):
        if (k + 1) % 3 == 0:
            p[k, 4] = False
    p[30, :] = False
    return p


@functools.lru_cache(maxsize=None)
def table(name, S=5):
    """present[k][s] of a schedule (bool array); streams beyond the schedule's (nperseg >= 8192 runs three) are cut off."""
    if name == "A":
        t = _table_a()
    elif name == "C":
        t = _table_c()
    elif name == "P":
        t = _table_p()
    else:
        t = _table_regular(len(sq.SCHEDULES[name].T), 5)
    t = t[:, :S].copy()
    t.setflags(write=False)
    return t


def gaps(present, s):
    """[(a, b)] calls a < b with stream s present at both and absent at every call between (b - a - 1 >= 1 absent calls)."""
    out, last = [], None
    for k in range(present.shape[0]):
        if present[k, s]:
            if last is not None and k - last > 1:
                out.append((last, k))
            last = k
    return out


# ---- poison ----------------------------------------------------------------------------------------------------------------------
def poisoned(x, present_k, fmt):
    """Call k's buffers ``x`` (``sequence_cases.buffer``: complex64 [S, n]) in the form the handle is fed (``sequence_cases.wire``),
    the rows of absent streams replaced by poison: NaN on complex input, a full-scale tone (a quarter of the sample rate, every
    component at the rails) on the wire formats.  A handle that reads such a row finds records, climbs AUTO's levels or marks the
    detrend guard."""
    feed, _ = sq.wire(x, fmt)
    feed = np.array(feed)
    n = x.shape[1]
    for s in np.flatnonzero(~np.asarray(present_k)):
        if fmt in ("c64", "c128"):
            feed[s] = np.nan + 1j * np.nan
        else:
            q = np.arange(n) % 4
            re, im = np.array([1, 0, -1, 0])[q], np.array([0, 1, 0, -1])[q]
            if fmt in ("u8", "u8f64"):
                feed[s, 0::2] = np.where(re > 0, 255, np.where(re < 0, 0, 128))
                feed[s, 1::2] = np.where(im > 0, 255, np.where(im < 0, 0, 128))
            elif fmt in ("i8", "i8f64"):
                feed[s, 0::2] = np.where(re > 0, 127, np.where(re < 0, -128, 0))
                feed[s, 1::2] = np.where(im > 0, 127, np.where(im < 0, -128, 0))
            else:
                feed[s, 0::2] = np.where(re > 0, 32767, np.where(re < 0, -32768, 0))
                feed[s, 1::2] = np.where(im > 0, 32767, np.where(im < 0, -32768, 0))
    return feed


# ---- the oracle over a schedule with gaps ----------------------------------------------------------------------------------------
MODELS = ("gapped", "zeros_reset", "lockstep")


@functools.lru_cache(maxsize=None)
def oracle_run(name, nperseg, fmt="c64", events=(), min_hops=sq.MIN_HOPS, S=None, model="gapped"):
    """[call][stream] -> ``sequence_cases.Call`` (None for an absent pair): ``sequence_cases.oracle_run`` with the (call, stream)
    pairs of ``table(name)`` that are absent skipped -- no ``stft_power``, ``last[s]`` untouched.  An event (reset, SNR change)
    issued while its stream is absent takes effect at the stream's next present call, as the state it changes is only read there.
    ``model``: the contract (``gapped``) or one of the two wrong models of the module docstring."""
    assert model in MODELS
    sched = sq.SCHEDULES[name]
    S = sq.n_streams(nperseg) if S is None else S
    present = table(name, S)
    kws = [sq.case_settings(nperseg, fmt, min_hops=min_hops) for _ in range(S)]
    last = [None] * S
    out = []
    for k in range(len(sched.T)):
        for ev in events:
            if ev[1] == k:
                last[ev[2]] = None
                if ev[0] == "snr":
                    kws[ev[2]] = dict(kws[ev[2]], snr_threshold_db=ev[3])
        _, seen = sq.wire(sq.buffer(sched, nperseg, k, S, sigma=sq.case_sigma(fmt)), fmt)
        row = []
        for s in range(S):
            if not present[k, s]:
                row.append(None)
                if model == "zeros_reset":
                    last[s] = None
                elif model == "lockstep" and last[s] is not None:
                    last[s] = np.zeros((nperseg, sched.T[k]), last[s].dtype)
                continue
            freqs, times, spec = oracle.stft_power(seen[s], sq.FS, sq.WINDOW, nperseg)
            recs = sq.extract(times, spec, last[s], sq.params_of(kws[s]))
            row.append(sq.Call(recs, sq.shadow_flags(recs, freqs)))
            last[s] = spec
        out.append(row)
    return out


def gap_records(name, nperseg, fmt="c64", min_hops=sq.MIN_HOPS, S=None):
    """{absent calls in the gap: [(call, stream, record)]}: the oracle's records that start in the previous buffer of a stream whose
    previous buffer lies across a gap."""
    S = sq.n_streams(nperseg) if S is None else S
    present = table(name, S)
    want = oracle_run(name, nperseg, fmt, (), min_hops, S)
    out = {}
    for s in range(S):
        for a, b in gaps(present, s):
            for r in want[b][s].records:
                if r.start < 0:
                    out.setdefault(b - a - 1, []).append((b, s, r))
    return out


# ---- feeding a handle ------------------------------------------------------------------------------------------------------------
def run_handle(b, name, nperseg, fmt="c64", pipelined=False, before_call=None, after_fetch=None, S=None, masked=True):
    """Every call of the schedule through handle ``b`` (poisoned rows for the absent streams) -> [(records, call_info)], like
    ``sequence_cases.run_handle``.  ``masked``: ``b.set_present(table[k])`` ahead of call k's enqueue -- with ``pipelined`` call
    k + 1 is enqueued, under ITS mask, before call k is fetched.  ``masked=False`` is the twin on which the entry is never called."""
    sched = sq.SCHEDULES[name]
    S = sq.n_streams(nperseg) if S is None else S
    present = table(name, S)
    n = len(sched.T)

    def enqueue(k):
        if before_call:
            before_call(k)
        if masked:
            b.set_present(present[k])
        sq.enqueue(b, poisoned(sq.buffer(sched, nperseg, k, S, sigma=sq.case_sigma(fmt)), present[k], fmt), fmt)

    out = []
    if pipelined:
        enqueue(0)
    for k in range(n):
        if pipelined:
            if k + 1 < n:
                enqueue(k + 1)
        else:
            enqueue(k)
        rec = b.fetch_records()
        out.append((rec, b.native.call_info()))
        if after_fetch:
            after_fetch(k, rec)
    return out


def hold_sequence(runs, name, nperseg, fmt="c64", events=(), min_hops=sq.MIN_HOPS, form="lin", f64_tol=None, note=None, what="", S=None):
    """``sequence_cases.hold_sequence`` with gaps, its comparison rules unchanged: after every call, per PRESENT stream, identity and
    shadow verdicts equal the gapped oracle's and the float fields lie within the precision64 model (look-back cells from the
    reference of the stream's own last present buffer); an ABSENT stream delivers nothing.  Returns (records, negative starts,
    negative starts across a gap)."""
    from tests import precision64 as p64

    sched = sq.SCHEDULES[name]
    S = sq.n_streams(nperseg) if S is None else S
    present = table(name, S)
    want = oracle_run(name, nperseg, fmt, events, min_hops, S)
    prev = [None] * S
    last_present = [None] * S
    n_rec = n_neg = n_gap = 0
    for k, (rec, info) in enumerate(runs):
        L = max(1, int(info.segs_per_chunk))
        _, seen = sq.wire(sq.buffer(sched, nperseg, k, S, sigma=sq.case_sigma(fmt)), fmt)
        for ev in events:
            if ev[1] == k:
                prev[ev[2]] = None
        for s in range(S):
            mine = rec[rec["stream"] == s]
            tag = f"{what} call {k} (T {sched.T[k]}) stream {s}"
            if not present[k, s]:
                assert len(mine) == 0, f"{tag}: an absent stream delivered {sq.rec_key(mine)}"
                continue
            w = want[k][s]
            assert sq.rec_key(mine) == sq.key(w.records), f"{tag}: records differ from the gapped oracle's\n got  {sq.rec_key(mine)}\n want {sq.key(w.records)}"
            assert [bool(v) for v in mine["shadowed"]] == w.shadowed, f"{tag}: shadow verdicts"
            if f64_tol is not None:
                sq.check_f64(mine, w.records)
            elif sched.T[k] > 0:
                ref = p64.stft_power_f64(seen[s], sq.FS, sq.WINDOW, nperseg)
                bd = p64.cell_bounds(ref, form)
                if len(mine):
                    pr = prev[s]
                    chk = p64.check_records(mine, ref, bd, L, pr[0] if pr else None, pr[1] if pr else None, what=tag)
                    assert not chk.failures, "\n".join(chk.failures[:8])
                    if note:
                        for f, v in chk.worst.items():
                            note(f"{f} ({form})", v)
                prev[s] = (ref, bd)
            else:
                prev[s] = None
            neg = int((mine["start"] < 0).sum())
            n_rec += len(mine)
            n_neg += neg
            if last_present[s] is not None and k - last_present[s] > 1:
                n_gap += neg
            last_present[s] = k
    return n_rec, n_neg, n_gap
