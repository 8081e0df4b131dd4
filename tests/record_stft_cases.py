"""One complex STFT value per delivered segment (``rt_fetch_record_stft``): the float64 model of a value, its round-off bound, the
NumPy restatement of the kernel's summation order the bound's constant was fixed from, and the inputs of both suites
(tests/test_record_stft_contract.py on the CPU, tests/test_gpu_record_stft.py on the GPU).

Model (``model_values``).  For a delivered segment with samples x[0 .. N) -- the snippet ``fetch_record_iq`` returns, converted as
the kernels convert the call's format -- window w (the float32 coefficients SciPy multiplies with; float64 on a float64 handle),
``scale`` as the handle carries it and the record's bin fi,

    value = sqrt(scale) * sum_n w[n] (x[n] - mean(x)) exp(-2 pi i fi n / N)

evaluated in float64 for float32 handles and in ``numpy.longdouble`` for float64 ones (the model must be finer than what it
judges), as a single-bin sum with the twiddle's exponent reduced in integers.  It is SciPy's ``mode='complex'`` spectrogram at that
bin and segment (tests/test_record_stft_contract.py holds it to that).

Bound (the form of tests/precision64.py, per value):

    e = sqrt(scale) * u * ( C * G * ||w y||_2  +  C_DC * mean|x| * |W_fi| )  +  C_ABS * u * |value|

u = 2**-24 (2**-53 for a float64 handle), y = x - mean(x), W = DFT(w).  G is the depth of record_stft's summation order
(csrc/rt_record_stft.h), not an FFT's: a lane adds its own samples one after the other -- ceil(N / (64 SPP)) pieces of SPP samples,
SPP = 16 bytes / bytes per sample -- and six butterfly steps combine the 64 lanes: G = samples a lane + 6.  C_DC is precision64's;
C_ABS covers the multiplication by sqrt(scale), its own rounding and the store.

The constant C is fixed from float32 arithmetic on the CPU only: ``restate`` walks the kernel's order in NumPy float32 (each fma as
one rounding of the float64 product-sum), ``sweep`` runs it over every size, window, bin and input kind below.  Where no tone and no
window lobe is in the bin the C term stands alone, and C is about 4 x the worst |restatement - model| there in units of
sqrt(scale) u G ||w y||; C_ABS is about 4 x what the tones' rows need; with all three the restatement stays under a third of the
bound everywhere (``python -m tests.record_stft_cases`` writes the sweep to profiles/record_stft_worst_ratio.txt).  The GPU's figures
are appended to that file and never go into a constant.
"""
import math
import os
from collections import namedtuple

import numpy as np

from oracle import analyze_oracle as oracle
from pyradiotracking_amd import synth
from tests import precision64 as p64
from tests import sequence_cases as sq

U32, U64 = 2.0 ** -24, 2.0 ** -53
#: profiles/record_stft_worst_ratio.txt: the float32 noise rows reach 0.575 in units of the C term alone: about 4 x
C_SUM = 2.5
C_DC = p64.C_DC
#: a tone at its bin has |value| ~ sqrt(N) ||w y||: the roundings of the last butterfly steps, of sqrt(scale) and of the product are
#: relative to |value| and reach about 2 u |value| in the sweep
C_ABS = 8.0

#: samples of a 16-byte piece, by fed format
SPP = {"c64": 2, "c128": 1, "u8": 8, "i8": 8, "i16": 4}
PI_LD = np.longdouble("3.14159265358979323846264338327950288")

Quantities = namedtuple("Quantities", "values norm abs_m absW root")


def depth(nperseg, spp):
    """G: the samples one lane adds in turn, and the six butterfly steps over the wave."""
    return math.ceil(nperseg / (64 * spp)) * spp + 6


def u8_to_complex128_like_handle(raw):
    """What a float64 handle makes of wire bytes (include/rt_analyze.h, csrc/rt_f64.h: load_f64): ``(double)b / 127.5 - 1.0`` per
    component, a real division.  NumPy's complex ``iq /= 127.5`` (``synth.u8_to_complex128_like_pyrtlsdr``) multiplies by a rounded
    reciprocal instead: for 20 of the 256 byte values the last bit differs, an absolute 1e-16 a sample that a segment of noise under
    a DC offset shows at once against a float64 bound."""
    v = np.asarray(raw, dtype=np.float64) / 127.5 - 1.0
    return v[..., 0::2] + 1j * v[..., 1::2]


def converted(samples, fmt, f64=False):
    """``fetch_record_iq``'s samples in the fed format -> what the kernels compute with (complex64, complex128 on a float64 handle)"""
    if fmt in ("c64", "c128"):
        return np.asarray(samples)
    flat = np.ascontiguousarray(samples).reshape(-1)
    return {"u8": u8_to_complex128_like_handle if f64 else synth.u8_to_complex64_like_kernel,
            "i8": synth.i8_to_complex128 if f64 else synth.i8_to_complex64,
            "i16": synth.i16_to_complex128 if f64 else synth.i16_to_complex64}[fmt](flat)


def model_values(x, fi, w, scale, nperseg, wide=False):
    """``x``: the complex samples of whole segments (any number), ``fi`` one bin for all or one per segment -> ``Quantities`` per
    segment.  ``wide``: longdouble arithmetic (a float64 handle's model), else float64."""
    ft = np.longdouble if wide else np.float64
    ct = np.clongdouble if wide else np.complex128
    N = int(nperseg)
    x = np.asarray(x).reshape(-1, N)
    n_seg = x.shape[0]
    fi = np.broadcast_to(np.asarray(fi, dtype=np.int64), (n_seg,))
    xr, xi = x.real.astype(ft), x.imag.astype(ft)
    yr, yi = xr - xr.mean(axis=1)[:, None], xi - xi.mean(axis=1)[:, None]
    k = (fi[:, None] * np.arange(N, dtype=np.int64)[None, :]) % N  # the exponent, reduced in integers
    ang = (ft(-2) * (PI_LD if wide else ft(np.pi))) * k.astype(ft) / ft(N)
    c, s = np.cos(ang), np.sin(ang)
    wr = np.asarray(w).astype(ft)[None, :]
    vr, vi = wr * yr, wr * yi
    root = np.sqrt(ft(scale))
    X = ((vr * c - vi * s).sum(axis=1) + 1j * (vr * s + vi * c).sum(axis=1)).astype(ct)
    norm = np.sqrt((vr * vr + vi * vi).sum(axis=1)).astype(np.float64)
    abs_m = np.hypot(xr, xi).mean(axis=1).astype(np.float64)
    absW = np.abs(((wr * c).sum(axis=1) + 1j * (wr * s).sum(axis=1)).astype(np.complex128))
    return Quantities(X * root, norm, abs_m, absW, float(root))


def bound(q, nperseg, spp, u=U32, c_sum=C_SUM):
    """[n_seg] the amplitude bound of every value"""
    with np.errstate(invalid="ignore"):
        return q.root * u * (c_sum * depth(nperseg, spp) * q.norm + C_DC * q.abs_m * q.absW) + C_ABS * u * np.abs(q.values).astype(np.float64)


def ratios(got, q, nperseg, spp, u=U32):
    """|got - model| / bound per value; a value that must be NaN and is: 0, one that is NaN and must not be (or the reverse): inf"""
    got = np.asarray(got)
    want_nan = ~np.isfinite(np.abs(q.values).astype(np.float64))
    got_nan = ~np.isfinite(got)
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.abs(got.astype(q.values.dtype) - q.values).astype(np.float64)
        b = bound(q, nperseg, spp, u)
        r = np.where(b > 0, d / b, np.where(d == 0, 0.0, np.inf))
    r = np.where(want_nan | got_nan, np.where(want_nan & got_nan, 0.0, np.inf), r)
    return r


# ---- the kernel's order in NumPy ---------------------------------------------------------------------------------------------------
def twiddles(nperseg, ft=np.float32):
    """rt_tables.h: record_stft_twiddles -- exp(-2 pi i j / N) in the wider type, rounded once (cos, sin)"""
    wide = np.float64 if ft == np.float32 else np.longdouble
    pi = wide(np.pi) if ft == np.float32 else PI_LD
    ang = wide(-2) * pi * np.arange(nperseg).astype(wide) / wide(nperseg)
    return np.cos(ang).astype(ft), np.sin(ang).astype(ft)


def _fma(a, b, c, ft):
    wide = np.float64 if ft == np.float32 else np.longdouble
    return (a.astype(wide) * b.astype(wide) + c.astype(wide)).astype(ft)


def _butterfly(v):
    lanes = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lanes ^ m]
    return v[:, 0]


def restate(x, fi, w, root, nperseg, spp, ft=np.float32, fault=None):
    """record_stft's arithmetic, operation by operation, for the segments ``x`` [n_seg, N] at one bin: lane l walks the pieces l,
    l + 64, ... of ``spp`` samples; the mean about the first sample; four fmas a sample; butterflies over the 64 lanes.
    ``fault``: one of the planted mistakes of tests/test_record_stft_contract.py."""
    N = int(nperseg)
    ct = np.complex64 if ft == np.float32 else np.complex128
    x = np.asarray(x).reshape(-1, N).astype(ct)
    xr, xi = np.ascontiguousarray(x.real), np.ascontiguousarray(x.imag)
    w = np.asarray(w).astype(ft)
    tr, ti = twiddles(N, ft)
    if fault == "conjugate":
        ti = -ti
    if fault == "fi_off_by_one":
        fi = (fi + 1) % N
    lanes = np.arange(64)
    rounds = math.ceil(math.ceil(N / spp) / 64)
    order = [(j * 64 + lanes) * spp + e for j in range(rounds) for e in range(spp)]  # [step][lane] -> sample
    x0r, x0i = xr[:, :1], xi[:, :1]
    sr = np.zeros((x.shape[0], 64), ft)
    si = np.zeros((x.shape[0], 64), ft)
    for n in order:
        ok = (n < N)[None, :]
        nn = np.minimum(n, N - 1)
        sr = np.where(ok, sr + (xr[:, nn] - x0r), sr)
        si = np.where(ok, si + (xi[:, nn] - x0i), si)
    mr = x0r[:, 0] + _butterfly(sr) / ft(N)
    mi = x0i[:, 0] + _butterfly(si) / ft(N)
    if fault == "no_detrend":
        mr, mi = np.zeros_like(mr), np.zeros_like(mi)
    ar = np.zeros((x.shape[0], 64), ft)
    ai = np.zeros((x.shape[0], 64), ft)
    for n in order:
        ok = (n < N)[None, :]
        nn = np.minimum(n, N - 1)
        k = (int(fi) * nn) % N
        vr = w[nn][None, :] * (xr[:, nn] - mr[:, None])
        vi = w[nn][None, :] * (xi[:, nn] - mi[:, None])
        t_r, t_i = tr[k][None, :], ti[k][None, :]
        nr = _fma(-vi, t_i, _fma(vr, t_r, ar, ft), ft)
        ni = _fma(vi, t_r, _fma(vr, t_i, ai, ft), ft)
        ar, ai = np.where(ok, nr, ar), np.where(ok, ni, ai)
    root = ft(root) if fault != "scale_not_root" else ft(float(root) ** 2)
    return (root * _butterfly(ar) + 1j * (root * _butterfly(ai))).astype(ct)


# ---- the sweep that fixes C --------------------------------------------------------------------------------------------------------
SWEEP_SIZES = (32, 256, 300, 1024, 4096)
SWEEP_WINDOWS = ("hamming", "hann", ("kaiser", 8.0))
KINDS = ("noise", "tone", "tone_dc", "u8", "i16")


def sweep_bins(N):
    return (0, 1, N - 1, N // 2, N - N // 3)


def window32(window, nperseg):
    return oracle.window_coefficients(window, nperseg).astype(np.float32)


def sweep_input(kind, N, fi, n_seg, rng):
    """complex64 [n_seg, N] and the samples of a piece its format would have"""
    x = (rng.standard_normal((n_seg, N)) + 1j * rng.standard_normal((n_seg, N))) * 0.012
    n = np.arange(N)
    if kind != "noise":
        x = x + 0.25 * np.exp(2j * np.pi * ((fi + 0.3) * n) / N)[None, :] * np.exp(2j * np.pi * 0.3 * np.arange(n_seg))[:, None]
    if kind == "tone_dc":
        x = x + (0.4 - 0.3j)
    if kind == "u8":
        return synth.u8_to_complex64_like_kernel(synth.quantize_u8(x.astype(np.complex64).reshape(-1))).reshape(n_seg, N), SPP["u8"]
    if kind == "i16":
        return synth.i16_to_complex64(synth.quantize_i16(x.astype(np.complex64).reshape(-1))).reshape(n_seg, N), SPP["i16"]
    return x.astype(np.complex64), SPP["c64"]


def sweep(n_seg=24, seed=7, f64=False):
    """{(nperseg, window, kind): (c, full)}.  ``c``: the worst |restatement - model| / (sqrt(scale) u G ||w y||) at the two bins
    outside every window's main lobe (N / 2 and N - N / 3), where the C term stands alone for an input without a tone -- C_SUM
    comes from the ``noise`` rows of this column.  ``full``: the worst |restatement - model| / bound over all five bins with the
    constants as they stand."""
    ft, u = (np.float64, U64) if f64 else (np.float32, U32)
    out = {}
    for N in SWEEP_SIZES:
        for window in SWEEP_WINDOWS:
            w = oracle.window_coefficients(window, N) if f64 else window32(window, N)
            scale = float(1.0 / (sq.FS * (w.astype(np.float64) ** 2).sum())) if f64 else p64.scale_f32(window, N, sq.FS)
            root = math.sqrt(scale) if f64 else float(np.float32(math.sqrt(scale)))
            for kind in KINDS:
                rng = np.random.default_rng([seed, N, KINDS.index(kind)])
                c_only = full = 0.0
                for fi in sweep_bins(N):
                    x, spp = sweep_input(kind, N, fi, n_seg, rng)
                    if f64:
                        x = x.astype(np.complex128)
                    q = model_values(x, fi, w, scale, N, wide=f64)
                    got = restate(x, fi, w, root, N, spp, ft)
                    d = np.abs(got.astype(q.values.dtype) - q.values).astype(np.float64)
                    if fi in (N // 2, N - N // 3):
                        c_only = max(c_only, float((d / (q.root * u * depth(N, spp) * q.norm)).max()))
                    full = max(full, float(ratios(got, q, N, spp, u).max()))
                out[(N, window if isinstance(window, str) else "kaiser8", kind)] = (c_only, full)
    return out


PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "record_stft_worst_ratio.txt")


def write_sweep(path=PROFILE):
    lines = ["record_stft: the NumPy restatement of the kernel's summation order against the float64 (longdouble) model",
             "(tests/record_stft_cases.py: restate, sweep), 24 segments a row at the bins 0, 1, N - 1, N / 2 and N - N / 3.",
             "  c     worst |d| / (sqrt(scale) u G ||w y||_2) at the bins N / 2 and N - N / 3 (outside every window's main lobe)",
             "  full  worst |d| / bound over all five bins, bound = sqrt(scale) u (C_SUM G ||w y|| + C_DC mean|x| |W_fi|) + C_ABS u |value|",
             f"C_SUM = {C_SUM} (4 x the worst `c` of the float32 noise rows), C_DC = {C_DC}, C_ABS = {C_ABS}; G = samples a lane + 6.", "",
             f"{'nperseg':>8} {'window':>8} {'input':>8} {'c f32':>8} {'full f32':>9} {'c f64':>8} {'full f64':>9}"]
    a, b = sweep(), sweep(f64=True)
    for key in a:
        lines.append(f"{key[0]:>8} {key[1]:>8} {key[2]:>8} {a[key][0]:8.3f} {a[key][1]:9.3f} {b[key][0]:8.3f} {b[key][1]:9.3f}")
    noise = max(v[0] for k, v in a.items() if k[2] == "noise")
    worst = (max(v[1] for v in a.values()), max(v[1] for v in b.values()))
    lines.append(f"CPU restatement: worst c of the float32 noise rows {noise:.3f}; worst full ratio float32 {worst[0]:.3f}, float64 {worst[1]:.3f}")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return noise, worst


# ---- pulse-pair estimate -----------------------------------------------------------------------------------------------------------
def fine_allowance(c, e):
    """What ``offset`` (in bins) of one record may differ from the model's: (1 / 2 pi) sum_pairs(|c_t| e_{t+1} + |c_{t+1}| e_t +
    e_t e_{t+1}) / |R_model| -- ``c`` the model's values of the pairs' cells in order, ``e`` their bounds."""
    a = np.abs(np.asarray(c).astype(np.complex128))
    R = np.abs((c[1:] * np.conj(c[:-1])).sum())
    return float((a[:-1] * e[1:] + a[1:] * e[:-1] + e[:-1] * e[1:]).sum() / R / (2 * np.pi))


# ---- the GPU suite's buffers -------------------------------------------------------------------------------------------------------
#: schedule P's tables (tests/sequence_cases.py) on four calls of 24 .. 40 segments and four streams: the first call has no
#: look-back (D = 0), the later ones hold records that reach back into the held tails
GPU_S = 4
GPU_SCHEDULE = sq.SCHEDULES["P"]._replace(name="P4", T=(40, 33, 35, 24), rag_base=sq.SCHEDULES["P"].rag_base[:4])
DC_STREAM, DC_OFFSET, DC_BIN = 0, complex(0.02, -0.015), 1
NEG_STREAM = 1
FINE_OFFSET_BINS = 0.2  # the two planted pulses sit this far over their bin's centre
PLANT_SEGS = (6, 16)    # ... and last over these whole segments of calls 1 and 2


def neg_bin(nperseg):
    """The negative-frequency bin (upper half of the fftfreq order) furthest from the schedule's tones of that stream"""
    N = nperseg
    tones = sq.tone_bins(N, NEG_STREAM) + sq.extra_bins(N, NEG_STREAM)
    return max(range(N // 2 + 1, N), key=lambda b: (min(min((b - t) % N, (t - b) % N) for t in tones), b))


def gpu_buffer(nperseg, k, sigma=synth.NOISE_SIGMA):
    """complex64 [GPU_S, n]: call k as schedule P plants it, plus in calls 1 and 2 a pulse at bin 1 of a stream under a DC offset
    (every sample of that stream, every call) and one at a negative-frequency bin of another stream."""
    x = sq.buffer(GPU_SCHEDULE, nperseg, k, GPU_S, sigma=sigma).astype(np.complex128)
    w = oracle.window_coefficients(sq.WINDOW, nperseg)
    amp = synth.amp_for_peak_dbw(sq.PEAK_DBW - 4.0, w, sq.FS)
    x[DC_STREAM] += DC_OFFSET
    if k in (1, 2):
        a, e = PLANT_SEGS[0] * nperseg, PLANT_SEGS[1] * nperseg
        n = np.arange(a, e)
        for s, b in ((DC_STREAM, DC_BIN), (NEG_STREAM, neg_bin(nperseg))):
            x[s, a:e] += amp * np.exp(2j * np.pi * (b + FINE_OFFSET_BINS) * n / nperseg)
    return x.astype(np.complex64)


def gpu_feed(nperseg, k, fmt):
    """what call k feeds a handle in format ``fmt`` (sequence_cases' names; the wire formats with its gain and noise level: the DC
    offset becomes 0.4 + 0.3 of full scale, nothing clips)"""
    return np.ascontiguousarray(sq.wire(gpu_buffer(nperseg, k, sq.case_sigma(fmt)), fmt)[0])


if __name__ == "__main__":
    print(write_sweep())
