"""NumPy restatements of taco_f0_range_curve (include/taco_hip.h): a tracked pitch contour turned into the per-frame step curve
that scales every frame's distance from the row's own level by k.
`curve` in float64 is the reference the device is held to; `curve(..., dtype=np.float32)` is the same definition in float32 with the
header's operation order (every product, sum and quotient rounded; the smoothing summed in the order j = -W .. W; the centre by
tests.f0_ref.stats' sequential float32 sums) and serves ONLY to size the bar F0_RANGE_STEP_ATOL below.  The neighbour search
(`neighbours`) is in integers and is held to a brute-force linear scan per frame (`neighbours_brute`).
Imports without a GPU and without the library; the constants are restated, not imported."""
import numpy as np

from tests import f0_ref as fr

ONE, MIN_STEP, MAX_STEP = 65536, 32768, 131072
MAX_SCALE_Q, MAX_SMOOTH, MAX_FRAMES = 4 * 65536, 8, 8192
SMOOTH, LIMIT = 2, 0.5                # the Python layer's UNTUNED defaults

# The bar on |device step_q - float64 restatement's step_q|, in step units (2^-16 of a ratio).  Measured, not guessed, and not tuned on
# the device's output: the float32 restatement against the float64 one on exactly the inputs of tests/test_gpu_f0_range.py
# (tests/f0_range_cases.all_cases), compared BEFORE the final rintf -- the unrounded 65536 * exp2(e), clamped to the step range.
# tests/test_f0_range_host.py repeats the measurement and holds the constant to it.  Largest difference over all of them: 0.697
# steps, on a row of 257 frames at k = 4 (the float32 centre of 180 sequentially summed logarithms near 7 is off by a few 1e-6
# octaves, times k - 1 = 3, times 65536 ln 2 = 45426 steps per octave); 0.26 at 8192 frames and k = 1.5, 0.21 with a base at the
# limit of one octave, below 0.2 elsewhere.
# Bar = 1 + 2 x that: the 1 for rintf at a tie boundary (two values a hair apart round to neighbouring integers), the factor 2 because
# the device's log2f / exp2f are another implementation than NumPy's with the same nominal accuracy.  A wrong neighbour, a dropped
# ballot word or a misplaced centre is an error of thousands of steps.
MEASURED_FLOAT32_STEP_ERROR = 0.70
F0_RANGE_STEP_ATOL = 1.0 + 2.0 * MEASURED_FLOAT32_STEP_ERROR


def row_frames(frames_b, frames_per_unit, F):
    return fr.row_frames(frames_b, frames_per_unit, F)


def clamp_scale(scale_q):
    return ONE if scale_q is None else min(max(int(scale_q), 0), MAX_SCALE_Q)


def neighbours(voiced):
    """voiced (n) bool -> (before, after) int64: the nearest voiced index strictly in front of / behind every frame, -1 for none"""
    voiced = np.asarray(voiced, dtype=bool)
    n = voiced.shape[0]
    idx = np.arange(n, dtype=np.int64)
    last = np.maximum.accumulate(np.where(voiced, idx, -1))
    first = np.minimum.accumulate(np.where(voiced, idx, n)[::-1])[::-1]
    before = np.concatenate([[-1], last[:-1]]) if n else last
    after = np.concatenate([first[1:], [n]]) if n else first
    return before.astype(np.int64), np.where(after >= n, -1, after).astype(np.int64)


def neighbours_brute(voiced):
    """the same by a linear scan per frame"""
    voiced = [bool(v) for v in voiced]
    n = len(voiced)
    before, after = [-1] * n, [-1] * n
    for f in range(n):
        for j in range(f - 1, -1, -1):
            if voiced[j]:
                before[f] = j
                break
        for j in range(f + 1, n):
            if voiced[j]:
                after[f] = j
                break
    return np.array(before, dtype=np.int64), np.array(after, dtype=np.int64)


def deviations(p, centre, dtype):
    """p (n) float32 periods of the live frames of a row with at least one voiced frame -> d (n) in `dtype`: steps 2 and 3"""
    voiced = p > 0
    n = p.shape[0]
    d = np.zeros(n, dtype=dtype)
    with np.errstate(all='ignore'):
        d[voiced] = np.log2(p[voiced].astype(dtype)) - dtype(centre)
    before, after = neighbours(voiced)
    f = np.arange(n, dtype=np.int64)
    gap = ~voiced
    both = gap & (before >= 0) & (after >= 0)
    pb, pa = before[both], after[both]
    t = (f[both] - pb).astype(dtype) / (pa - pb).astype(dtype)
    d[both] = d[pb] + t * (d[pa] - d[pb])
    only_b, only_a = gap & (before >= 0) & (after < 0), gap & (before < 0) & (after >= 0)
    d[only_b] = d[before[only_b]]
    d[only_a] = d[after[only_a]]
    assert d.dtype == dtype
    return d


def smooth(d, W):
    """step 4: the triangle of half-width W, the sum in the order j = -W .. W from +0, in d's dtype"""
    dtype = d.dtype.type
    n = d.shape[0]
    f = np.arange(n, dtype=np.int64)
    acc = np.zeros(n, dtype=dtype)
    for j in range(-W, W + 1):
        acc = acc + dtype(W + 1 - abs(j)) * d[np.clip(f + j, 0, n - 1)]
    return acc / dtype((W + 1) * (W + 1))


def curve(period, frames=None, frames_per_unit=1, scale_q=None, base_q=None, smooth_w=SMOOTH, limit=LIMIT, dtype=np.float64):
    """period (B, F) float32 -> (step_q (B, F) int32, stats (B, 3) in `dtype`, real (B, F) in `dtype`: the steps in front of rint,
    clamped to the step range).  frames / scale_q: None or B integers; base_q: None or (B, F) integers.  Nothing behind F_b is read."""
    period = np.asarray(period)
    assert period.dtype == np.float32 and period.ndim == 2
    B, F = period.shape
    assert 1 <= F <= MAX_FRAMES and 0 <= smooth_w <= MAX_SMOOTH and 0.0 < limit <= 1.0
    stats = fr.stats(period, None, frames, frames_per_unit, dtype=dtype)
    real = np.full((B, F), float(ONE), dtype=dtype)
    lim = dtype(np.float32(limit))          # (the C ABI takes a float)
    for b in range(B):
        Fb = row_frames(None if frames is None else frames[b], frames_per_unit, F)
        kq = clamp_scale(None if scale_q is None else scale_q[b])
        base = None if base_q is None else np.clip(np.asarray(base_q)[b, :Fb].astype(np.int64), MIN_STEP, MAX_STEP)
        if Fb == 0:
            continue
        if kq == ONE or stats[b, 0] == 0:
            if base is not None:
                real[b, :Fb] = base.astype(dtype)      # copied: no log, no exp
            continue
        d = deviations(period[b, :Fb], stats[b, 1], dtype)
        s = smooth(d, smooth_w)
        km1 = dtype(kq) * dtype(2.0 ** -16) - dtype(1.0)
        with np.errstate(all='ignore'):
            e = np.clip(km1 * s, -lim, lim)
            if base is not None:
                e = e + np.log2(base.astype(dtype) * dtype(2.0 ** -16))
            y = dtype(65536.0) * np.exp2(e)
        assert y.dtype == dtype
        real[b, :Fb] = np.clip(y, dtype(MIN_STEP), dtype(MAX_STEP))
    return np.rint(real).astype(np.int32), stats, real


def excursions(period, step_q, frames=None, frames_per_unit=1):
    """per row the float64 log2 of period * step / 65536 over its voiced frames -- the log-period a frame has behind the curve, since
    taco_frames_pitch_curve at step s moves a frame's harmonics by the ratio 65536 / s"""
    period, step_q = np.asarray(period), np.asarray(step_q)
    out = []
    for b in range(period.shape[0]):
        Fb = row_frames(None if frames is None else frames[b], frames_per_unit, period.shape[1])
        p, s = period[b, :Fb].astype(np.float64), step_q[b, :Fb].astype(np.float64)
        out.append(np.log2(p[p > 0] * s[p > 0] / 65536.0))
    return out
