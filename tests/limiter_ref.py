"""NumPy restatements of taco_wave_limit (include/taco_hip.h) -- TEST INFRASTRUCTURE for csrc/limiter.hip.

limit(): steps 1 to 6 in float32, every operation one rounded fp32 operation in the stated order -- vectorised over n, looping over
the taps j and the window k, which keeps the order of both sums.  The entry point has no recursion, so this is not an approximation
of it: the kernel must give these bits.
true_peak64(): the meter in fp64 with the same taps, for what the interpolator reads on tones.
The tables are formed here from the formulas, on their own."""
from __future__ import annotations

import numpy as np
from scipy.signal import lfilter

F32 = np.float32
ONE = F32(1.0)


def taps(P=4, T=12, beta=6.0):
    """(P - 1, T) float32: tap j of phase p at t = j - (T/2 - 1) - p/P; sinc(t) I0(beta sqrt(1 - (t / (T/2))^2)) / I0(beta), 0 where
    the root's argument is negative; each phase divided by its own fp64 sum, rounded once"""
    out = np.zeros((P - 1, T), np.float32)
    for p in range(1, P):
        t = np.arange(T, dtype=np.float64) - (T // 2 - 1) - float(p) / P
        u = 1.0 - (t / (T // 2)) ** 2
        h = np.zeros(T, np.float64)
        ok = u >= 0.0
        h[ok] = np.sinc(t[ok]) * np.i0(beta * np.sqrt(u[ok])) / np.i0(beta)
        out[p - 1] = (h / h.sum()).astype(np.float32)
    return out


def window(W):
    """(2 W + 1) float32: 0.5 - 0.5 cos(2 pi (k + 1) / (2 W + 2)) divided by its fp64 sum, rounded once"""
    k = np.arange(2 * W + 1, dtype=np.float64)
    h = 0.5 - 0.5 * np.cos(2.0 * np.pi * (k + 1.0) / (2 * W + 2))
    return (h / h.sum()).astype(np.float32)


def _shifted(x, lo, n):
    """x[lo : lo + n] with zeros outside the array"""
    out = np.zeros(n, x.dtype)
    a, b = max(lo, 0), min(lo + n, len(x))
    if b > a:
        out[a - lo:b - lo] = x[a:b]
    return out


def envelope(x, tp, dtype=np.float32):
    """step 1: e[n] over the row x (its n_b samples; zeros outside), in `dtype`"""
    x = np.asarray(x, dtype=dtype)
    n = len(x)
    e = np.abs(x)
    tp = np.asarray(tp, dtype=dtype)
    if tp.size:
        T = tp.shape[1]
        for p in range(tp.shape[0]):
            acc = np.zeros(n, dtype)
            for j in range(T):
                acc = acc + tp[p, j] * _shifted(x, j - (T // 2 - 1), n)   # fl(acc + fl(t x)): two roundings in `dtype`
            e = np.maximum(e, np.abs(acc))
    return e


def true_peak64(x, tp, inset=0):
    """the meter in fp64 with the taps as given (float32 values, widened); inset: without that many samples at either end of the row"""
    e = envelope(np.asarray(x, np.float64), np.asarray(tp, np.float64), np.float64)
    e = e[inset:len(e) - inset]
    return float(e.max()) if len(e) else 0.0


def pcm16(v):
    """taco_wave_loudness's rule: clamp to [-1, 1], trunc(v * 32767.0f)"""
    return np.trunc(np.clip(np.asarray(v, F32), F32(-1.0), ONE) * F32(32767.0)).astype(np.int16)


def limit(x, G=1.0, ceiling=1.0, tp=None, win=None, L=None):
    """One row: x = its n_b samples (float32), G the gain as handed to the entry point, tp (P - 1, T) float32 (None or empty: P = 1),
    win (2 W + 1) float32 or None for measure-only; L: the row's width (zeros behind n_b).  -> dict: out, pcm (L), peaks (4) float32,
    counts (2) int32, and the intermediate e, r, m, s (n_b) for the property tests"""
    x = np.ascontiguousarray(x, dtype=F32)
    n = len(x)
    L = n if L is None else L
    tp = np.zeros((0, 2), F32) if tp is None else np.asarray(tp, F32)
    e = envelope(x, tp)
    tp_in = e.max() if n else F32(0.0)
    if win is None:
        return dict(out=None, pcm=None, e=e, peaks=np.array([tp_in, 1.0, 1.0, np.abs(x).max() if n else 0.0], F32),
                    counts=np.array([n, 0], np.int32))
    G = F32(G)
    if not (np.isfinite(G) and G > 0):
        G = ONE
    c = F32(ceiling)
    win = np.asarray(win, F32)
    W = len(win) // 2
    ge = G * e
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(ge > c, c / ge, ONE).astype(F32)
    rp = np.concatenate([np.ones(2 * W, F32), r, np.ones(2 * W, F32)])   # r over [-2 W, n + 2 W)
    # m over [-W, n + W): m[i] = min r[i - W .. i + W]
    m = rp[0:n + 2 * W].copy()
    for k in range(1, 2 * W + 1):
        m = np.minimum(m, rp[k:k + n + 2 * W])
    d = np.zeros(n, F32)
    for k in range(2 * W + 1):
        d = d + win[k] * (ONE - m[k:k + n])
    s = np.minimum(ONE - d, r)
    o = (G * x) * s
    out = np.zeros(L, F32)
    out[:n] = o
    return dict(out=out, pcm=pcm16(out), e=e, r=r, m=m[W:W + n], s=s,
                peaks=np.array([tp_in, G, s.min() if n else 1.0, np.abs(o).max() if n else 0.0], F32),
                counts=np.array([n, int((s < ONE).sum())], np.int32))


def limit_rows(x, samples=None, gain=None, **kw):
    """limit() per row of x (B, L) over its first samples[b] values -> out (B, L), pcm (B, L), peaks (B, 4), counts (B, 2)"""
    B, L = x.shape
    rows = [limit(x[b, :L if samples is None else int(np.clip(samples[b], 0, L))], 1.0 if gain is None else gain[b], L=L, **kw)
            for b in range(B)]
    stack = lambda k: None if rows[0][k] is None else np.stack([r[k] for r in rows])   # noqa: E731
    return stack('out'), stack('pcm'), stack('peaks'), stack('counts')


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def tone(n, cycles_per_sample, phase=0.0, amp=0.5):
    return (amp * np.sin(2.0 * np.pi * cycles_per_sample * np.arange(n) + phase)).astype(np.float32)


TONES = (('fs/8', 1 / 8, 0.0), ('fs/4 at 0 deg', 1 / 4, 0.0), ('fs/4 at 45 deg', 1 / 4, np.pi / 4), ('fs/3', 1 / 3, 0.0),
         ('5 fs/12', 5 / 12, 0.0))


def voiced(n, sr=16000, f0=110.0, seed=3):
    """a synthetic voiced row with the crest factor of speech: a glottal-like pulse train through two resonances, in syllables of
    uneven level -- the row whose one peak holds today's gain down"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    x = np.zeros(n)
    period = int(round(sr / f0))
    x[::period] = 1.0
    x += 0.02 * rng.standard_normal(n)   # (breath)
    y = np.zeros(n)
    for fc, bw, g in ((700.0, 110.0, 1.0), (1900.0, 160.0, 0.5)):
        r = np.exp(-np.pi * bw / sr)
        a1, a2 = -2.0 * r * np.cos(2.0 * np.pi * fc / sr), r * r
        y += g * lfilter([1.0], [1.0, a1, a2], x)
    env = 0.25 + 0.75 * np.clip(np.sin(2.0 * np.pi * 2.5 * t), 0.0, None) ** 2
    y = y * env
    y[n // 2] += 6.0 * np.abs(y).max()   # one click: a Griffin-Lim artefact
    return (0.5 * y / np.abs(y).max()).astype(np.float32)


# ---- the cases of the bit-for-bit comparison (shared by the host and the GPU tests) --------------------------------------------
CASE_W, CASE_P, CASE_T = 8, 4, 12
EDGE_NS = (0, 1, 5, 6, 16, 17, 33, 2047, 2048, 2049, 2048 + 16, 4096 + 1)
EDGE_L = 4099   # (odd: the rows of out and pcm start at every alignment)


def edge_rows():
    """-> (x (12, EDGE_L) with NaN behind each n_b, samples, gain, ceiling): noise with a unit impulse at sample 0, at n_b - 1, at 2047
    and at 2048 -- the dips straddle a chunk edge and the rows' two ends"""
    rng = np.random.default_rng(21)
    x = (0.2 * rng.standard_normal((len(EDGE_NS), EDGE_L))).astype(np.float32)
    for b, n in enumerate(EDGE_NS):
        for at in (0, n - 1, 2047, 2048):
            if 0 <= at < n:
                x[b, at] = -1.0 if at % 2 else 1.0
        x[b, n:] = np.nan
    gain = np.linspace(0.8, 2.0, len(EDGE_NS)).astype(np.float32)
    return x, np.array(EDGE_NS, np.int32), gain, 0.5


SHAPE_NAMES = ('impulse pairs', 'plateau', 'fs/4 at 45 deg', 'quiet', 'noise at G = 4')
SHAPE_L = 6000
SHAPE_CEILING = 0.4


def shape_rows(W=CASE_W):
    """-> (x (5, 6000), gain): two impulses 2 W - 1 apart (their dips merge) and two 4 W + 2 apart (they do not) on a noise floor; a
    plateau of equal samples above the ceiling, longer than 4 W and across the chunk edge; the fs/4 sine at 45 degrees whose samples
    (0.354) stay under the ceiling 0.4 while its true peak (0.5) does not; a row whose G tp_in stays under the ceiling; noise at G = 4"""
    from tests import wave_ref as wr
    rng = np.random.default_rng(22)
    L = SHAPE_L
    x = np.zeros((5, L), np.float32)
    x[0] = 0.01 * rng.standard_normal(L)
    for at in (1000, 1000 + 2 * W - 1, 3000, 3000 + 4 * W + 2):
        x[0, at] = 0.9
    x[1, 2030:2030 + 4 * W + 9] = 0.8
    x[2] = tone(L, 0.25, np.pi / 4)
    x[3] = 0.02 * rng.standard_normal(L)
    x[4] = wr.family('noise', L)
    return x, np.array([1.0, 1.0, 1.0, 2.0, 4.0], np.float32)
