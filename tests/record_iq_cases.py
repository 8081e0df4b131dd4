"""The samples behind every record (``rt_set_record_iq`` / ``rt_fetch_record_iq``): the NumPy model both suites hold the library to
(tests/test_record_iq_contract.py on the CPU through ``rt_hostcheck``, tests/test_gpu_record_iq.py on the GPU), and the cases.

``KeepEverything`` is the model the header states: keep every buffer that was fed, know for every stream which buffer its detection
looks back into, and slice whole segments with the clip rule

    first_seg = max(start - m, -D(s))   ...   min(end + m, T) - 1,      D(s) = min(T_pred, K + m) or 0

It knows nothing of tail rows, rotation or call slots.  ``TailRows`` is a model of the MECHANISM on a plain handle (three rows per
stream, written at enqueue, read at fetch) with the three mistakes such a mechanism invites, each of which the schedules must tell
from the truth:

* ``ragged``  the tail taken from the buffer's last ``D * N`` samples: the ragged remainder included;
* ``offset``  the tail written at a column offset that ignores ``T < K + m``;
* ``reuse``   two rows per stream in alternation: the row a pending call still reads is written by the next enqueue.
"""
import copy

import numpy as np

from tests import sequence_cases as sq

#: format -> (dtype of the fed array, its elements per sample, bytes per sample)
FORMATS = {"c64": (np.complex64, 1, 8), "c128": (np.complex128, 1, 16), "u8": (np.uint8, 2, 2), "i8": (np.int8, 2, 2), "i16": (np.int16, 2, 4)}
WRONG = ("ragged", "offset", "reuse")
#: schedule P on the GPU: (nperseg, format, margin, pipelined, device tensors) -- every nperseg, format and margin, serial and
#: pipelined, host arrays and device tensors, each at least twice; nperseg 8 in uint8 makes a segment 16 bytes
GPU_SEQUENCES = (
    (8, "u8", 0, False, False), (8, "c64", 3, True, True), (32, "c64", 0, True, False), (32, "i8", 3, False, True),
    (256, "i16", 3, True, False), (256, "u8", 0, False, True), (4096, "i8", 0, True, True), (4096, "i16", 3, False, False),
)
GPU_SEQUENCE_CASES = tuple(sorted({c[:3] for c in GPU_SEQUENCES}))


def base_format(fmt):
    """sequence_cases' format names -> the fed format: ``u8f64`` feeds uint8, ``c128`` complex128 ..."""
    return fmt[:-3] if fmt.endswith("f64") else fmt


def samples_of(feed, fmt):
    """The fed array ``[S, n * per]`` with one entry per SAMPLE: ``[S, n]`` complex, ``[S, n, 2]`` for the wire formats."""
    dt, per, _ = FORMATS[fmt]
    a = np.asarray(feed)
    assert a.dtype == dt, (a.dtype, fmt)
    if a.ndim == 1:
        a = a[None, :]
    return a if per == 1 else a.reshape(a.shape[0], -1, 2)


def raw(x):
    """any sample array -> its bytes"""
    return np.ascontiguousarray(x).view(np.uint8).reshape(-1)


class _Held:
    """A buffer a later detection looks back into."""

    def __init__(self, row, T, fmt, held):
        self.row, self.T, self.fmt, self.held = row, T, fmt, held


class ModelCall:
    def __init__(self, T, N, margin, fmt, rows, lead):
        self.T, self.N, self.margin, self.fmt, self.rows, self.lead = T, N, margin, fmt, rows, lead  # lead[s] = (_Held or None, D)

    def D(self, s):
        return self.lead[s][1]

    def expect(self, rec):
        """``rec``: the delivered records (``stream``, ``start``, ``end``) -> (offsets, first_seg, [samples of record i])."""
        N, m = self.N, self.margin
        offsets, first_seg, out = [0], [], []
        for s, start, end in zip(rec["stream"].tolist(), rec["start"].tolist(), rec["end"].tolist()):
            pred, D = self.lead[s]
            first = max(start - m, -D)
            last = max(first, min(end + m, self.T))
            parts = []
            if first < 0:
                parts.append(pred.row[(pred.T + first) * N:(pred.T + min(last, 0)) * N])
            if last > 0:
                parts.append(self.rows[s][max(first, 0) * N:last * N])
            got = np.concatenate(parts) if parts else self.rows[s][:0]
            assert len(got) == (last - first) * N
            out.append(got)
            first_seg.append(first)
            offsets.append(offsets[-1] + len(got))
        return np.array(offsets, np.int64), np.array(first_seg, np.int32), out


class KeepEverything:
    """The model: every buffer kept; ``links >= 2``: the streams are runs of consecutive buffers (rt_set_chain)."""

    def __init__(self, S, N, K, margin=None, links=0):
        self.S, self.N, self.K, self.links = S, N, K, links if links >= 2 else 0
        self.margin = None  # None: the feature is off
        self.present = np.ones(S, bool)
        self.reset()
        if margin is not None:
            self.set_margin(margin)
        self._undo = None

    def reset(self):
        self.last = [None] * self.S
        self.last_run = [None] * (self.S // self.links if self.links else 0)
        self.pending_reset = np.zeros(self.S, bool)

    def reset_stream(self, s):
        self.pending_reset[s] = True

    def set_present(self, mask):
        self.present = np.ones(self.S, bool) if mask is None else np.asarray(mask, bool).copy()

    def set_margin(self, m):
        m = None if m is None or m < 0 else m
        if m != self.margin:
            for h in self.last + self.last_run:
                if h is not None:
                    h.held = False
        self.margin = m

    def set_chain(self, links):
        self.links = links if links >= 2 else 0
        self.reset()

    def _lead(self, h, fmt):
        if h is None or self.margin is None or not h.held or h.fmt != fmt:
            return (h, 0)
        return (h, min(h.T, self.K + self.margin))

    def call(self, feed, fmt):
        self._undo = (copy.copy(self.last), copy.copy(self.last_run), self.pending_reset.copy(),
                      [None if h is None else h.held for h in self.last + self.last_run])
        rows = samples_of(feed, fmt)
        T = rows.shape[1] // self.N
        on = self.margin is not None
        lead = [(None, 0)] * self.S
        if not self.links:
            for s in np.flatnonzero(self.present):
                h = None if self.pending_reset[s] else self.last[s]
                self.pending_reset[s] = False
                lead[s] = self._lead(h, fmt)
                self.last[s] = _Held(rows[s], T, fmt, on)
        else:
            for r in range(self.S // self.links):
                pred = None
                for s in range(r * self.links, (r + 1) * self.links):
                    if not self.present[s]:
                        continue
                    h = pred if pred is not None else self.last_run[r]
                    if self.pending_reset[s]:
                        h = None
                    self.pending_reset[s] = False
                    lead[s] = self._lead(h, fmt)
                    pred = _Held(rows[s], T, fmt, on)
                if pred is not None:
                    self.last_run[r] = pred
        return ModelCall(T, self.N, self.margin or 0, fmt, rows, lead)

    def rollback(self):
        self.last, self.last_run, self.pending_reset, held = self._undo
        for h, was in zip(self.last + self.last_run, held):
            if h is not None:
                h.held = was


class TailRows:
    """The mechanism on a plain handle without masks: ``rows`` tail rows per stream of ``K + m`` segments, written by ``enqueue``,
    read by ``fetch`` -- in the caller's order, so that two calls may be in flight.  ``rule``: "correct" or one of ``WRONG``."""

    def __init__(self, S, N, K, margin, rule="correct"):
        assert rule == "correct" or rule in WRONG
        self.S, self.N, self.cols, self.margin, self.rule = S, N, K + margin, margin, rule
        self.n_rows = 2 if rule == "reuse" else 3
        self.tails = [[None] * self.n_rows for _ in range(S)]
        self.cur = [-1] * S       # the row holding each stream's latest tail
        self.held = [0] * S       # segments in it
        self.calls = {}           # k -> what fetch k needs
        self.pending = []

    def enqueue(self, k, feed, fmt):
        rows = samples_of(feed, fmt)
        n = rows.shape[1]
        T, N = n // self.N, self.N
        D = min(T, self.cols)
        lead = []
        for s in range(self.S):
            lead.append((self.cur[s], min(self.held[s], self.cols) if self.cur[s] >= 0 else 0))
        for s in range(self.S):
            busy = {self.cur[s]} | {self.calls[j]["lead"][s][0] for j in self.pending}
            if self.rule == "reuse":
                w = 1 - self.cur[s] if self.cur[s] >= 0 else 0
            else:
                w = min(i for i in range(self.n_rows) if i not in busy)
            row = np.zeros((self.cols * N,) + rows.shape[2:], rows.dtype)
            src = rows[s][n - D * N:n] if self.rule == "ragged" else rows[s][(T - D) * N:T * N]
            row[:D * N] = src  # (a tail of D segments lies at the start of its row)
            self.tails[s][w] = row
            self.cur[s], self.held[s] = w, D
        self.calls[k] = dict(T=T, rows=rows, lead=lead)
        self.pending.append(k)

    def fetch(self, k, rec, first_lookback):
        """``first_lookback[s]``: whether the detection had look-back for s (the schedules here: every call but the first)."""
        c = self.calls[k]
        self.pending.remove(k)
        N, m = self.N, self.margin
        out = []
        for s, start, end in zip(rec["stream"].tolist(), rec["start"].tolist(), rec["end"].tolist()):
            buf, D = c["lead"][s]
            if not first_lookback[s]:
                D = 0
            first = max(start - m, -D)
            last = max(first, min(end + m, c["T"]))
            parts = []
            if first < 0:
                row = self.tails[s][buf]
                # "offset": the reader takes segment -d from column K + m - d, as if every tail were K + m segments deep
                base = self.cols if self.rule == "offset" else D
                parts.append(row[(base + first) * N:(base + min(last, 0)) * N])
            if last > 0:
                parts.append(c["rows"][s][max(first, 0) * N:last * N])
            out.append(np.concatenate(parts) if parts else c["rows"][s][:0])
        return out


# ---- the schedules' own records (the CPU oracle) and synthetic ones ----------------------------------------------------------------
def oracle_records(name, nperseg, k, S=None):
    """The oracle's records of call k of a schedule, all streams, as a structured array in delivery order."""
    calls = sq.oracle_run(name, nperseg, S=S)
    keys = [(s, int(r.fi), int(r.start), int(r.end)) for s, c in enumerate(calls[k]) for r in c.records]
    return np.array(keys, dtype=[("stream", "<i4"), ("fi", "<i4"), ("start", "<i4"), ("end", "<i4")])


def random_records(rng, call, lookback_T, K, n_per_stream=4):
    """Records a detection could deliver for ``call``: per present stream a few (start, end) with start >= -min(T_pred, K) where
    the stream has look-back (``lookback_T[s]``: T_pred or -1), in (stream, fi, start) order.  Always one at the deepest start."""
    keys = []
    for s, T_pred in enumerate(lookback_T):
        if T_pred is None or call.T < 2:
            continue
        lo = -min(T_pred, K) if T_pred > 0 else 0
        starts = sorted({lo, 0} | {int(rng.integers(lo, call.T - 1)) for _ in range(n_per_stream)})
        for fi, a in enumerate(starts):
            e = int(rng.integers(max(a, 0) + 1, call.T + 1))
            keys.append((s, fi, a, e))
    return np.array(keys, dtype=[("stream", "<i4"), ("fi", "<i4"), ("start", "<i4"), ("end", "<i4")])


def feed(name, nperseg, k, fmt, S=None):
    """What call k of a schedule feeds the handle in format ``fmt`` (sequence_cases' names)."""
    sched = sq.SCHEDULES[name]
    return np.ascontiguousarray(sq.wire(sq.buffer(sched, nperseg, k, S, sigma=sq.case_sigma(fmt)), fmt)[0])


def model_run(name, nperseg, fmt, margin, S=None, events=()):
    """[call] -> ModelCall for a whole schedule on a plain handle; ``events``: ("reset", k, s) / ("snr", k, s, dB) as
    ``sequence_cases.oracle_run`` takes them -- both start stream s's call k without look-back."""
    sched = sq.SCHEDULES[name]
    S = sq.n_streams(nperseg) if S is None else S
    m = KeepEverything(S, nperseg, sq.tail_cols(nperseg), margin)
    out = []
    for k in range(len(sched.T)):
        for ev in events:
            if ev[1] == k:
                m.reset_stream(ev[2])
        out.append(m.call(feed(name, nperseg, k, fmt, S), base_format(fmt)))
    return out


# ---- a stream whose threshold lies under its noise ---------------------------------------------------------------------------------
# Schedule P's first calls at nperseg 256 on three streams; stream 1 is given a threshold of -170 dBW (the noise is at -152 dBW a
# cell) and an SNR threshold of 0 dB, so every run of three cells over their row's mean is a record: hundreds of short records per
# call anywhere in the buffer, the last segments included -- what clips the margin at the END, which the schedule's own records never
# do (their `end` is at most 6 and no call of 9 or more segments is shorter than 6 + 3) -- and a payload several times the 1 MiB a
# slot's pool starts with, so that the pool has to grow inside the fetch.  Beside it streams 0 and 2 keep the schedule's records, 4 to
# 38 segments long.
NOISY_NPERSEG, NOISY_S, NOISY_STREAM, NOISY_CALLS, NOISY_MARGIN = 256, 3, 1, 6, 3
NOISY_THRESHOLD_DBW, NOISY_SNR_DB = -170.0, 0.0


def noisy_settings():
    """[stream] -> analysis keywords"""
    out = [sq.settings(NOISY_NPERSEG) for _ in range(NOISY_S)]
    out[NOISY_STREAM] = dict(out[NOISY_STREAM], signal_threshold_dbw=NOISY_THRESHOLD_DBW, snr_threshold_db=NOISY_SNR_DB)
    return out


def noisy_oracle_records():
    """[call] -> the oracle's records of the case, all streams, in delivery order"""
    kws = noisy_settings()
    last = [None] * NOISY_S
    out = []
    for k in range(NOISY_CALLS):
        x = sq.buffer(sq.SCHEDULES["P"], NOISY_NPERSEG, k, NOISY_S)
        keys = []
        for s in range(NOISY_S):
            _, times, spec = sq.oracle.stft_power(x[s], sq.FS, sq.WINDOW, NOISY_NPERSEG)
            keys += [(s, int(r.fi), int(r.start), int(r.end)) for r in sq.extract(times, spec, last[s], sq.params_of(kws[s]))]
            last[s] = spec
        out.append(np.array(keys, dtype=[("stream", "<i4"), ("fi", "<i4"), ("start", "<i4"), ("end", "<i4")]))
    return out


def noisy_model():
    m = KeepEverything(NOISY_S, NOISY_NPERSEG, sq.tail_cols(NOISY_NPERSEG), NOISY_MARGIN)
    return [m.call(feed("P", NOISY_NPERSEG, k, "c64", NOISY_S), "c64") for k in range(NOISY_CALLS)]


def coverage(calls, records, margin):
    """What a case must hold to be worth running: counts of records that reach back, start at segment 0, and are clipped by the
    margin at the front (the lead or segment 0 stops it) and at the end (T stops it)."""
    back = zero = front = tail = 0
    for c, rec in zip(calls, records):
        for s, start, end in zip(rec["stream"].tolist(), rec["start"].tolist(), rec["end"].tolist()):
            back += start < 0 and c.D(s) > 0
            zero += start == 0
            front += margin > 0 and start - margin < -c.D(s)
            tail += margin > 0 and end + margin > c.T
    return dict(back=back, zero=zero, front=front, tail=tail)


def check_delivery(call, rec, got, what=""):
    """``got`` = (offsets, first_seg, samples) as ``BatchSignalAnalyzer.fetch_record_iq`` returns them, against the model."""
    offsets, first_seg, samples = got
    w_off, w_first, w_parts = call.expect(rec)
    assert np.array_equal(offsets, w_off), f"{what}: offsets"
    assert np.array_equal(first_seg, w_first), f"{what}: first segments\n got  {first_seg.tolist()}\n want {w_first.tolist()}"
    assert samples.dtype == FORMATS[call.fmt][0], (what, samples.dtype)
    for i, w in enumerate(w_parts):
        g = samples[offsets[i]:offsets[i + 1]]
        assert np.array_equal(raw(g), raw(w)), f"{what}: record {i} {rec[i]}: the samples are not the fed bytes"
    return len(w_parts)
