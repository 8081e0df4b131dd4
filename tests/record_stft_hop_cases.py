"""Record STFT at a sub-segment hop (``rt_fetch_record_stft_hop``): the NumPy restatement of the frame plan, the frames of a
record's snippet, the lane-group restatement of the kernel's order and the synthetic pulses of the estimator tests -- shared by
tests/test_record_stft_hop_contract.py (CPU) and tests/test_gpu_record_stft_hop.py (GPU).  The model of a value, its bound and the
GPU suite's buffers are tests/record_stft_cases.py's: a frame is a segment that starts elsewhere, with the same summation depth.

Frame plan.  Record i delivers L_i = (offsets[i + 1] - offsets[i]) / N whole segments first_seg[i] ...; the Lp = clamp(-first_seg,
0, L) below 0 are its predecessor part, the rest its own.  A part of L >= 1 segments has (L - 1) k + 1 frames every h = N / k
samples, a part of none has none, and no frame straddles the parts.
"""
import math

import numpy as np

from tests import record_stft_cases as rs


def part_frames(L, k):
    L = np.asarray(L, dtype=np.int64)
    return np.where(L > 0, (L - 1) * k + 1, 0)


def frame_plan(offsets, first_seg, N, k):
    """``offsets`` [n + 1] in SAMPLES (``fetch_record_iq``'s), ``first_seg`` [n] -> dict: ``frame_first`` [n + 1], ``pool_seg`` [n],
    ``lp`` [n], and per frame ``record``, ``part`` (0 the predecessor's, 1 the record's own), ``sample`` (the frame's first sample
    in the pool / in ``fetch_record_iq``'s samples) and ``position`` (relative to sample 0 of the call's buffer)."""
    offsets = np.asarray(offsets, dtype=np.int64)
    first = np.asarray(first_seg, dtype=np.int64)
    h = N // k
    L = np.diff(offsets) // N
    lp = np.clip(-first, 0, L)
    fp, fc = part_frames(lp, k), part_frames(L - lp, k)
    frame_first = np.concatenate([[0], np.cumsum(fp + fc)]).astype(np.int64)
    record, part, sample, position = [], [], [], []
    for i in range(len(first)):
        for p, (n_f, seg0, at) in enumerate(((fp[i], offsets[i], first[i] * N), (fc[i], offsets[i] + lp[i] * N, max(first[i], 0) * N))):
            j = np.arange(n_f, dtype=np.int64)
            record.append(np.full(n_f, i))
            part.append(np.full(n_f, p))
            sample.append(seg0 + j * h)
            position.append(at + j * h)
    cat = lambda a: np.concatenate(a).astype(np.int64) if a else np.zeros(0, np.int64)  # noqa: E731
    return dict(frame_first=frame_first, pool_seg=offsets[:-1] // N, lp=lp, record=cat(record), part=cat(part), sample=cat(sample),
                position=cat(position))


def frames_of(x, sample, N):
    """[n_frames, N]: the frames that start at ``sample`` of the flat complex samples ``x``"""
    x = np.asarray(x).reshape(-1)
    return x[np.asarray(sample, dtype=np.int64)[:, None] + np.arange(N)[None, :]]


# ---- the kernel's order with a group of G lanes a frame ----------------------------------------------------------------------------
def _group_butterfly(v, G):
    lanes = np.arange(G)
    m = G // 2
    while m >= 1:
        v = v + v[:, lanes ^ m]
        m //= 2
    return v[:, 0]


def restate_groups(x, fi, w, root, nperseg, spp, G, ft=np.float32):
    """record_stft_hop's arithmetic for the frames ``x`` [n, N] at one bin with ``G`` lanes a frame (csrc/rt_record_stft_hop.h):
    lane l walks the pieces l, l + G, ... of ``spp`` samples; the mean about the first sample; four fmas a sample; a butterfly
    over the G lanes (xor G / 2 ... 1).  ``G = 64`` is ``rs.restate``'s order."""
    N = int(nperseg)
    ct = np.complex64 if ft == np.float32 else np.complex128
    x = np.asarray(x).reshape(-1, N).astype(ct)
    xr, xi = np.ascontiguousarray(x.real), np.ascontiguousarray(x.imag)
    w = np.asarray(w).astype(ft)
    tr, ti = rs.twiddles(N, ft)
    lanes = np.arange(G)
    rounds = math.ceil(math.ceil(N / spp) / G)
    order = [(j * G + lanes) * spp + e for j in range(rounds) for e in range(spp)]  # [step][lane] -> sample
    x0r, x0i = xr[:, :1], xi[:, :1]
    sr = np.zeros((x.shape[0], G), ft)
    si = np.zeros((x.shape[0], G), ft)
    for n in order:
        ok = (n < N)[None, :]
        nn = np.minimum(n, N - 1)
        sr = np.where(ok, sr + (xr[:, nn] - x0r), sr)
        si = np.where(ok, si + (xi[:, nn] - x0i), si)
    mr = x0r[:, 0] + _group_butterfly(sr, G) / ft(N)
    mi = x0i[:, 0] + _group_butterfly(si, G) / ft(N)
    ar = np.zeros((x.shape[0], G), ft)
    ai = np.zeros((x.shape[0], G), ft)
    for n in order:
        ok = (n < N)[None, :]
        nn = np.minimum(n, N - 1)
        k = (int(fi) * nn) % N
        vr = w[nn][None, :] * (xr[:, nn] - mr[:, None])
        vi = w[nn][None, :] * (xi[:, nn] - mi[:, None])
        t_r, t_i = tr[k][None, :], ti[k][None, :]
        nr = rs._fma(-vi, t_i, rs._fma(vr, t_r, ar, ft), ft)
        ni = rs._fma(vi, t_r, rs._fma(vr, t_i, ai, ft), ft)
        ar, ai = np.where(ok, nr, ar), np.where(ok, ni, ai)
    root = ft(root)
    return (root * _group_butterfly(ar, G) + 1j * (root * _group_butterfly(ai, G))).astype(ct)


def group_of(nperseg, bytes_per_sample):
    """the lane group the kernel gives a frame: the smallest of 8, 16, 32 that holds its 16-byte pieces, else 64"""
    pieces = -(-nperseg * bytes_per_sample // 16)
    return 8 if pieces <= 8 else 16 if pieces <= 16 else 32 if pieces <= 32 else 64


# ---- synthetic pulses for the estimators -------------------------------------------------------------------------------------------
def one_part_record(x, fi, w, scale, N, k, first_segment=0):
    """A single record over the whole segments of ``x`` (all of one part): ``(offsets, first_segment, values)`` as
    ``fetch_record_stft(hop_div=k)`` would return them, the values from the float64 model."""
    L = len(x) // N
    n_f = (L - 1) * k + 1
    frames = frames_of(x, np.arange(n_f) * (N // k), N)
    q = rs.model_values(frames, fi, w, scale, N)
    return np.array([0, n_f], np.int64), np.array([first_segment], np.int32), q.values


def tone_record(delta_bins, fi, N, k, w, scale, n_seg=12, noise_db=-40.0, seed=0):
    """A tone ``delta_bins`` off bin ``fi``'s centre over ``n_seg`` segments under noise ``noise_db`` below it: one record, all of
    one part, whose own cells are all of them."""
    rng = np.random.default_rng([seed, int(round(delta_bins * 1000)) % 100003, k])
    n = np.arange(n_seg * N)
    sigma = 10.0 ** (noise_db / 20.0) / math.sqrt(2.0)
    x = np.exp(2j * np.pi * (fi + delta_bins) * n / N) + sigma * (rng.standard_normal(n.size) + 1j * rng.standard_normal(n.size))
    return one_part_record(x, fi, w, scale, N, k)


#: the rows of the edge sweep: (window, nperseg)
EDGE_ROWS = (("hamming", 256), ("hamming", 4096), ("hann", 1024), ("boxcar", 256))
EDGE_T, EDGE_ON, EDGE_OFF = 10, 2, 6  # segments of a trial; the pulse switches on inside segment 2 and off inside segment 6
EDGE_BIN = 50


def edge_trial(N, rng):
    """A bin-centred pulse switched on and off at random SAMPLES: ``(x, rise, fall, start, end)`` -- the record's own cells are the
    segments wholly inside the pulse, the segments around them are its delivered margin."""
    rise = int(rng.integers(EDGE_ON * N, (EDGE_ON + 1) * N))
    fall = int(rng.integers(EDGE_OFF * N, (EDGE_OFF + 1) * N))
    n = np.arange(EDGE_T * N)
    x = np.exp(2j * np.pi * EDGE_BIN * n / N)
    x[:rise] = 0
    x[fall:] = 0
    return x, rise, fall, EDGE_ON + 1, EDGE_OFF


def edge_errors(window, N, k, trials=40, seed=5):
    """worst |edge - switch sample| in samples over ``trials`` pulses, (rise, fall), of ``record_edges`` on the model's values"""
    from oracle import analyze_oracle as oracle
    from pyradiotracking_amd.analyze import record_edges

    w = oracle.window_coefficients(window, N)
    scale = 1.0 / (rs.sq.FS * float((w ** 2).sum()))
    rng = np.random.default_rng([seed, N, k])
    worst = np.zeros(2)
    for _ in range(trials):
        x, rise, fall, start, end = edge_trial(N, rng)
        off, first, values = one_part_record(x, EDGE_BIN, w, scale, N, k)
        got = record_edges(off, first, values, [start], [end], N, k)[0]
        worst = np.maximum(worst, np.abs(got - (rise, fall)))  # (a NaN edge would poison the maximum: none may occur)
    return worst


PROFILE = rs.os.path.join(rs.os.path.dirname(rs.PROFILE), "record_stft_hop_estimators.txt")


def write_estimators(path=PROFILE):
    from oracle import analyze_oracle as oracle
    from pyradiotracking_amd.analyze import record_fine

    lines = ["record_stft_hop: the estimators on the float64 model's values (tests/record_stft_hop_cases.py), no GPU involved.", "",
             "record_edges: worst |edge - switch sample| over 40 bin-centred pulses switched at random samples, in hops (h = nperseg / k)",
             "and in nperseg; the suite's cap is a quarter of a hop at k >= 2.",
             f"{'window':>8} {'nperseg':>8} {'k':>3} {'rise/h':>8} {'fall/h':>8} {'worst/N':>8}"]
    for window, N in EDGE_ROWS:
        for k in (1, 2, 4, 8):
            e = edge_errors(window, N, k)
            lines.append(f"{window:>8} {N:>8} {k:>3} {e[0] / (N // k):8.3f} {e[1] / (N // k):8.3f} {e.max() / N:8.4f}")
    lines += ["", "record_fine: tones delta bins off bin 50's centre, nperseg 256, hamming, noise 40 dB down, 12 segments: the estimate in bins",
              f"{'delta':>8} {'k=1':>8} {'k=4':>8} {'k=8':>8}"]
    N, fi = 256, 50
    w = oracle.window_coefficients("hamming", N)
    scale = 1.0 / (rs.sq.FS * float((w ** 2).sum()))
    for delta in (0.3, 0.7, 1.3, -1.6):
        row = []
        for k in (1, 4, 8):
            off, first, values = tone_record(delta, fi, N, k, w, scale)
            row.append(record_fine(off, first, values, [0], [12], rs.sq.FS, N, k, [fi])["offset_hz"][0] / (rs.sq.FS / N))
        lines.append(f"{delta:8.3f} " + " ".join(f"{v:8.4f}" for v in row))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    write_estimators()
    print(open(PROFILE).read())
