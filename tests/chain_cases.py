"""Consecutive buffers of a recording as the streams of one call (``rt_set_chain``): the cases of tests/test_chain_contract.py (CPU)
and tests/test_gpu_chain.py (GPU).

A chain schedule is a schedule of tests/sequence_cases.py read as RECORDINGS: stream r of the schedule is recording r, call k of
the schedule is buffer k of every recording.  A chained handle of ``links`` links analyses buffers ``c * links ... c * links +
links - 1`` in its call c, buffer k at link ``k % links`` of run r (stream ``r * links + k % links``); all links of a call have one
length, so the schedule's lengths are per-call lengths of schedule A (or P) repeated ``links`` times.  The generator of
sequence_cases puts tones across EVERY boundary between consecutive buffers -- hot on the last d segments of buffer k - 1 and the
first e of buffer k --, so they cross link boundaries inside a call and call boundaries (last link -> first link) alike, and where
E_TAB gives e = 1 the tone's last hot segment is segment 0 of a link.

The yardstick is a plain handle of R streams that is fed the same buffers one call after another (``run_plain``); the chained
handle's records must equal its records byte for byte after mapping (call, stream) -> (recording, buffer) (``by_buffer``).

A mask ``present[k][r]`` says which buffers a recording HAS: an absent buffer is never analysed -- the reference's analyzer of that
recording is not called --, on the chained handle by ``set_present`` over the streams, on the yardstick by ``set_present`` over the
recordings (what tests/test_gpu_present.py holds to the gapped oracle).

Also here: the NumPy model of the host-only book (rt_core.h: ChainBook on a PresenceBook)."""
import numpy as np

from tests import present_cases as pc
from tests import sequence_cases as sq

R = 2  # recordings per handle in the GPU cases

# per-call lengths and ragged tails: schedule A's calls 0, 1, 3, 7, 8 (a call of other T, one of 33 < K, one of T = 2) and schedule
# P's calls 0, 3, 4, 5, 8 (all shorter than K + 6; one of 9 segments); "P7": two more calls, for a run that sits out four;
# "Pn": P with schedule C's raised noise floors in calls 2 and 3 (and C's thinned tones and runs of at least 10 segments)
CALLS = {
    "A": ((96, 70, 33, 2, 96), (5, 0, 7, 1, 0)),
    "P": ((47, 33, 35, 9, 41), (5, 7, 0, 3, 0)),
    "P7": ((47, 33, 35, 9, 41, 47, 33), (5, 7, 0, 3, 0, 0, 9)),
    "Pn": ((47, 33, 35, 9, 41), (5, 7, 0, 3, 0)),
}
NOISY_SIGMAS = (sq.ssc.SIGMA_QUIET, sq.ssc.SIGMA_QUIET, sq.SIGMA_FLOOR, sq.SIGMA_HIGH, sq.ssc.SIGMA_QUIET)


def schedule(base, links):
    """The chain schedule of ``base`` for ``links`` links, registered with sequence_cases under its name."""
    name = f"chain{base}{links}"
    if name not in sq.SCHEDULES:
        T, rag = CALLS[base]
        over = lambda v: tuple(x for x in v for _ in range(links))
        if base == "Pn":
            sq.SCHEDULES[name] = sq.Schedule(name, over(T), over(rag), False, 10, over(NOISY_SIGMAS), None, sq.C_D_MAX, sq.C_TONES)
        else:
            sq.SCHEDULES[name] = sq.Schedule(name, over(T), over(rag), False, 0, None, None)
    return name


def n_calls(base):
    return len(CALLS[base][0])


def boundary_kinds(name, nperseg, links, fmt="c64", min_hops=sq.MIN_HOPS):
    """{kind: oracle records with a negative start}: "link" -- the buffer is a later link of its call; "call" -- it is a call's first
    link (it looks into the last link of the call before); "t0" -- such a record of either kind that ends with segment 0 of its
    buffer (``end == 1``: the plateau's last hot cell is t = 0 of the link)."""
    want = sq.oracle_run(name, nperseg, fmt, (), min_hops, R)
    out = {"link": [], "call": [], "t0": []}
    for k, row in enumerate(want):
        for r, call in enumerate(row):
            for x in call.records:
                if x.start < 0:
                    out["link" if k % links else "call"].append((k, r, x))
                    if x.end == 1:
                        out["t0"].append((k, r, x))
    return out


# ---- the book ---------------------------------------------------------------------------------------------------------------------
NONE, WRITTEN, READ = 0, 1, 2  # rt_core.h: kChainNone / kChainWritten / kChainRead


class Model:
    """"A run is one reference analyzer; its buffers of a call are the present links in index order."

    Per run: the number of the buffer the analyzer saw last (a global counter, -1: none) and its segment count.  Beside it the
    rotation of three tail buffers, each holding per stream the number of the buffer whose columns it holds (written by a present
    stream, carried from the buffer read to the buffer written for an absent one, as the presence model of
    tests/test_present_contract.py).  ``call`` asserts that every present stream's source holds the columns of its predecessor
    buffer.  ``wrong``: "own_index" -- a run's first link looks into its OWN index of the call before; "call_T" -- a run's first
    link takes ``start_min`` from the call's own T."""

    def __init__(self, S, links, wrong=None):
        self.S, self.L, self.wrong = S, links, wrong
        self.present = np.ones(S, bool)
        self.reset = np.zeros(S, bool)
        self.cur = 0
        self.n_buffers = 0
        self.tails = np.full((3, S), -1, np.int64)
        self.last_buffer = np.full(S // links, -1, np.int64)  # per run: the analyzer's previous buffer
        self.last_T = np.full(S // links, -1, np.int64)
        self.last_T_idx = np.full(S, -1, np.int64)  # per stream index: its own previous length (the wrong model "own_index")
        self.undo = None

    def forget(self):
        self.reset[:] = False
        self.last_buffer[:] = -1
        self.last_T[:] = -1
        self.last_T_idx[:] = -1

    def call(self, T):
        self.undo = (self.reset.copy(), self.cur, self.n_buffers, self.tails.copy(), self.last_buffer.copy(), self.last_T.copy(), self.last_T_idx.copy())
        rd, wr = self.cur, (self.cur + 1) % 3
        S, L = self.S, self.L
        absent = ~self.present
        src_buf, src_idx, nsl = np.zeros(S, np.int32), np.full(S, -1, np.int32), np.full(S, -1, np.int32)
        took = self.reset & self.present
        new_tail = self.tails[rd].copy()  # absent streams: carried
        for r in range(S // L):
            prev_buffer, prev_T, prev_at = self.last_buffer[r], self.last_T[r], None  # the analyzer's `_spectrogram_last`
            for s in range(r * L, (r + 1) * L):
                if absent[s]:
                    continue
                me = self.n_buffers
                self.n_buffers += 1
                if took[s]:
                    pass  # a fresh analyzer: no previous map
                elif prev_at is not None:  # the link before, of this call: its columns are in the buffer the call writes
                    src_buf[s], src_idx[s], nsl[s] = WRITTEN, prev_at, prev_T
                    assert new_tail[prev_at] == prev_buffer, (s, prev_at)
                elif prev_buffer >= 0:  # the run's last buffer of an earlier call: in the buffer the call reads
                    if self.wrong == "own_index":
                        src_buf[s], src_idx[s], nsl[s] = READ, s, self.last_T_idx[s]
                    else:
                        at = int(np.flatnonzero(self.tails[rd, r * L:(r + 1) * L] == prev_buffer)[-1]) + r * L
                        src_buf[s], src_idx[s], nsl[s] = READ, at, (T if self.wrong == "call_T" else prev_T)
                        assert self.tails[rd, at] == prev_buffer, (s, at, self.tails[:, at], prev_buffer)
                new_tail[s] = me
                prev_buffer, prev_T, prev_at = me, T, s
                self.last_T_idx[s] = T
            if prev_at is not None:
                self.last_buffer[r], self.last_T[r] = prev_buffer, prev_T
        self.tails[wr] = new_tail
        self.reset &= absent
        self.cur = wr
        return absent.astype(np.uint8), nsl, (rd, wr), src_buf, src_idx, took.astype(np.uint8)

    def rollback(self):
        took = self.undo[0] & ~self.reset
        _, self.cur, self.n_buffers, self.tails, self.last_buffer, self.last_T, self.last_T_idx = self.undo
        self.reset = self.reset | took


def run_tables(name, links):
    """The presence table of present_cases for schedule ``name`` re-read as two runs of ``links`` streams: stream s takes the
    table's column (3 s + s // links) % 5, so that holes, absent suffixes and whole absent runs all occur (the table's call that
    every stream sits out among them).  -> bool [calls][2 * links]."""
    t = pc.table(name)
    S = 2 * links
    return np.stack([t[:, (s * 3 + s // links) % t.shape[1]] for s in range(S)], axis=1)


# ---- feeding handles (GPU) --------------------------------------------------------------------------------------------------------
def feed_of(name, nperseg, k, fmt, present_k=None):
    """buffer k of every recording in the form a handle is fed ([R, ...]); the rows of absent recordings poisoned."""
    x = sq.buffer(sq.SCHEDULES[name], nperseg, k, R, sigma=sq.case_sigma(fmt))
    return pc.poisoned(x, np.ones(R, bool) if present_k is None else present_k, fmt)


def run_plain(b, name, nperseg, fmt="c64", present=None, before_buffer=None):
    """The yardstick: every buffer of the schedule through the plain R-stream handle ``b``, one call each -> [(records, info)] by
    buffer.  ``present[k][r]``; ``before_buffer(b, k)`` runs ahead of buffer k's enqueue."""
    out = []
    for k in range(len(sq.SCHEDULES[name].T)):
        if before_buffer:
            before_buffer(b, k)
        if present is not None:
            b.set_present(present[k])
        sq.enqueue(b, feed_of(name, nperseg, k, fmt, None if present is None else present[k]), fmt)
        out.append((b.fetch_records(), b.native.call_info()))
    return out


def chained_feed(name, nperseg, c, links, fmt, present=None):
    """call c of the chained handle: [R * links, ...] rows, run r's link j = buffer c * links + j of recording r."""
    per = [feed_of(name, nperseg, c * links + j, fmt, None if present is None else present[c * links + j]) for j in range(links)]
    return np.ascontiguousarray(np.stack(per, axis=1).reshape(R * links, -1))


def run_chained(b, name, nperseg, links, fmt="c64", present=None, pipelined=False, before_call=None, after_fetch=None):
    """Every call of the chained handle ``b`` (a BatchSignalAnalyzer of R * links streams on which ``native.set_chain(links)`` was
    called) -> [(records, info)] by call.  The rows go in as the handle's own [S, B] layout, masks through ``native.set_present``."""
    n = len(sq.SCHEDULES[name].T) // links

    def enqueue(c):
        if before_call:
            before_call(b, c)
        if present is not None:
            m = np.array([present[c * links + j][r] for r in range(R) for j in range(links)], bool)
            b.native.set_present(m)
        feed = chained_feed(name, nperseg, c, links, fmt, present)
        if fmt == "u8":
            b.native.process_host_u8(feed)
        elif fmt == "i16":
            b.native.process_host_i16(feed)
        elif fmt == "i8":
            b.native.process_host_i8(feed)
        else:
            b.native.process_host(feed)

    out = []
    if pipelined:
        enqueue(0)
    for c in range(n):
        if pipelined:
            if c + 1 < n:
                enqueue(c + 1)
        else:
            enqueue(c)
        rec = b.fetch_records()
        out.append((rec, b.native.call_info()))
        if after_fetch:
            after_fetch(b, c, rec)
    return out


def by_buffer(chained_runs, links):
    """The chained handle's records re-read as the yardstick's: [buffer k] -> records with ``stream`` = the recording."""
    out = []
    for c, (rec, _) in enumerate(chained_runs):
        for j in range(links):
            mine = rec[rec["stream"] % links == j].copy()
            mine["stream"] //= links
            out.append(mine)
    return out
