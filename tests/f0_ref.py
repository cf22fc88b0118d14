"""NumPy restatements of taco_frames_f0 and taco_f0_stats (include/taco_hip.h): the pitch of magnitude frames.
`acf` in float64 is the reference the continuous part of the device's result is held to; `acf(..., dtype=np.float32)` is the same
definition in float32 with sequential sums (every product and every addition rounded, bins in ascending order) and serves ONLY to size
the tolerance F0_ACF_ATOL below.  `pick` is the exact part: the header's rules in float32, one rounded operation each, applied to
whatever float32 y it is given -- applied to the device's own acf it must give the device's period and strength bit for bit.
`stats` restates taco_f0_stats in float64, or in float32 with sequential sums (F0_STATS_ATOL).
Imports without a GPU and without the library; the constants are restated, not imported."""
import numpy as np

MAX_LAGS, MAX_FRAMES = 512, 8192
RATIO, THRESHOLD = 0.9, 0.3           # the Python layer's untuned defaults

# The bound on |device - fp64| over `acf`.  Measured, not guessed: the float32 restatement against the float64 one on exactly the
# inputs of tests/test_gpu_frames_f0.py (tests/f0_cases.all_cases; tests/test_frames_f0_host.py repeats the measurement and holds
# this constant to at least four times it).  Largest absolute error over all of them: 5.04e-6, on the mixed batch at C = 1025 with the
# production tables (1025 rounded products and additions per lag; 3.2e-6 at 512 lags without tables, up to 9.1e-7 at C <= 129); the
# values themselves are of order 1 (a normalised autocorrelation times a gain: at most 1.5 in magnitude on these inputs).
# Times 4 for another summation order and the few-ulp differences of the device's cosine and division.
MEASURED_FLOAT32_ACF_ERROR = 5.05e-6
# The same rule for the mean and the standard deviation of taco_f0_stats (tests/f0_cases.stats_cases): 4.03e-6 on the mean of 700
# values of log2(period) near 7 summed one after the other (4.6e-7 over 26 values, 3.2e-7 on the paired differences near 0).
MEASURED_FLOAT32_STATS_ERROR = 4.03e-6
F0_ACF_ATOL = 4.0 * MEASURED_FLOAT32_ACF_ERROR
F0_STATS_ATOL = 4.0 * MEASURED_FLOAT32_STATS_ERROR


def row_frames(frames_b, frames_per_unit, F):
    """F_b: frames[b] * frames_per_unit (Python integers: no overflow) clamped to [0, F]; None: F"""
    if frames_b is None:
        return int(F)
    return min(max(int(frames_b) * int(frames_per_unit), 0), int(F))


def tables(sr=16000, fmin=60.0, fmax=400.0, deemphasis=0.97, C=1025, win_length=1200):
    """(weight (C), gain (L), lag_min, lag_max) as tacotron_amd.lib.f0_tables defines them, float64, the window's autocorrelation as
    a direct sum of products"""
    lag_min, lag_max = int(np.floor(sr / fmax)), int(np.floor(sr / fmin))
    k = np.arange(C, dtype=np.float64)
    weight = 1.0 / np.abs(1.0 - deemphasis * np.exp(-1j * np.pi * k / (C - 1))) ** 2
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win_length) / win_length)
    wa = np.array([np.dot(w[:win_length - n], w[n:]) for n in range(lag_min - 1, lag_max + 2)])
    return weight, np.dot(w, w) / wa, lag_min, lag_max


def _cosines(C, lag_min, lag_max, dtype):
    N = 2 * (C - 1)
    n, k = np.arange(lag_min - 1, lag_max + 2, dtype=np.int64)[:, None], np.arange(C, dtype=np.int64)[None, :]
    return np.cos(2.0 * np.pi * ((n * k) % N).astype(np.float64) / N).astype(dtype)   # (L, C)


def acf_frames(m, weight, gain, lag_min, lag_max, dtype=np.float64):
    """m (C, n) float32 magnitudes of n frames -> y (L, n) in `dtype`; a frame whose float32 r0 is not > 0 gives zeros (the device
    forms m^2 in float32: 1e-30 squared is 0 there)"""
    C, n = m.shape
    L = lag_max - lag_min + 3
    u = np.full(C, 2.0, dtype=dtype)
    u[0] = u[-1] = 1.0
    w = np.ones(C, dtype=dtype) if weight is None else np.asarray(weight, dtype=np.float32).astype(dtype)
    g = np.ones(L, dtype=dtype) if gain is None else np.asarray(gain, dtype=np.float32).astype(dtype)
    cs = _cosines(C, lag_min, lag_max, dtype)
    m32 = m.astype(np.float32)
    with np.errstate(all='ignore'):
        p32 = (u.astype(np.float32) * w.astype(np.float32))[:, None] * (m32 * m32)
        sounding = np.cumsum(p32, axis=0, dtype=np.float32)[-1] > 0
        x = m.astype(dtype)
        p = (u * w)[:, None] * (x * x)
        if dtype == np.float64:
            r0, r = p.sum(axis=0), cs @ p
        else:
            r0, r = np.zeros(n, dtype=np.float32), np.zeros((L, n), dtype=np.float32)
            for k in range(C):   # sequential: one rounded product and one rounded addition per bin
                r0 = r0 + p[k]
                r = r + cs[:, k][:, None] * p[k][None, :]
        y = (r / np.where(sounding, r0, 1)[None, :]) * g[:, None]
    return np.where(sounding[None, :], y, dtype(0.0)).astype(dtype)


def acf(mag_t, frames=None, frames_per_unit=1, weight=None, gain=None, lag_min=40, lag_max=266, dtype=np.float64):
    """mag_t (B, C, F) float32 -> (B, L, F) in `dtype`; zeros behind F_b, and nothing behind F_b is read"""
    mag_t = np.asarray(mag_t)
    assert mag_t.dtype == np.float32 and mag_t.ndim == 3
    B, C, F = mag_t.shape
    L = lag_max - lag_min + 3
    assert C >= 9 and (C - 1) & (C - 2) == 0 and 2 <= lag_min <= lag_max <= C - 2 and L <= MAX_LAGS
    out = np.zeros((B, L, F), dtype=dtype)
    for b in range(B):
        Fb = row_frames(None if frames is None else frames[b], frames_per_unit, F)
        if Fb:
            out[b, :, :Fb] = acf_frames(mag_t[b, :, :Fb], weight, gain, lag_min, lag_max, dtype)
    return out


def pick(y, lag_min, ratio=RATIO, threshold=THRESHOLD):
    """y (..., L, F) float32, row j the lag lag_min - 1 + j -> (period, strength) (..., F) float32 by the header's exact rules.
    An all-zero column (an unvoiced frame, or one behind F_b) has no candidate and gives +0."""
    y = np.asarray(y)
    assert y.dtype == np.float32 and y.shape[-2] >= 3
    f32 = np.float32
    ym, y0, yp = y[..., :-2, :], y[..., 1:-1, :], y[..., 2:, :]
    with np.errstate(all='ignore'):
        cand = (y0 > ym) & (y0 >= yp)
        g = np.where(cand, y0, f32(-np.inf)).max(axis=-2)
        bar = f32(ratio) * g                                            # one float32 product
        ok = cand & (y0 >= bar[..., None, :])
        at = ok.argmax(axis=-2)                                         # the smallest lag; 0 when there is none
        take = lambda a: np.take_along_axis(a, at[..., None, :], axis=-2)[..., 0, :]   # noqa: E731
        a_m, a_0, a_p = take(ym), take(y0), take(yp)
        voiced = ok.any(axis=-2) & (a_0 >= f32(threshold))
        a = a_m - a_p
        t = a_0 + a_0
        d = (a_m - t) + a_p
        delta = np.clip((f32(0.5) * a) / np.where(d == 0, f32(1.0), d), f32(-0.5), f32(0.5))
        delta = np.where(d == 0, f32(0.0), delta)
        period = (at + lag_min).astype(f32) + delta
    assert period.dtype == np.float32 and a_0.dtype == np.float32
    return np.where(voiced, period, f32(0.0)), np.where(voiced, a_0, f32(0.0))


def track(mag_t, frames=None, frames_per_unit=1, weight=None, gain=None, lag_min=40, lag_max=266, ratio=RATIO, threshold=THRESHOLD):
    """the whole tracker on the float64 restatement: (period, strength) (B, F) float64.  The pick's rules are the same in any precision;
    this one is for what the METHOD measures, not for the device's bits"""
    y = acf(mag_t, frames, frames_per_unit, weight, gain, lag_min, lag_max)
    ym, y0, yp = y[:, :-2], y[:, 1:-1], y[:, 2:]
    cand = (y0 > ym) & (y0 >= yp)
    g = np.where(cand, y0, -np.inf).max(axis=1)
    ok = cand & (y0 >= (ratio * g)[:, None, :])
    at = ok.argmax(axis=1)
    take = lambda a: np.take_along_axis(a, at[:, None, :], axis=1)[:, 0, :]   # noqa: E731
    a_m, a_0, a_p = take(ym), take(y0), take(yp)
    voiced = ok.any(axis=1) & (a_0 >= threshold)
    d = (a_m - 2.0 * a_0) + a_p
    delta = np.where(d == 0, 0.0, np.clip(0.5 * (a_m - a_p) / np.where(d == 0, 1.0, d), -0.5, 0.5))
    return np.where(voiced, at + lag_min + delta, 0.0), np.where(voiced, a_0, 0.0)


def stats(period, other=None, frames=None, frames_per_unit=1, dtype=np.float64):
    """period (B, F) [, other (B, F)] float32 -> (B, 3) in `dtype`: count, mean and population standard deviation of log2(period), or
    of log2(other) - log2(period), over the frames below F_b in which every period given is > 0; float32: sequential sums"""
    period = np.asarray(period)
    assert period.dtype == np.float32 and period.ndim == 2
    B, F = period.shape
    out = np.zeros((B, 3), dtype=dtype)
    for b in range(B):
        Fb = row_frames(None if frames is None else frames[b], frames_per_unit, F)
        p = period[b, :Fb]
        keep = p > 0
        if other is not None:
            o = np.asarray(other)[b, :Fb]
            keep &= o > 0
        n = int(keep.sum())
        out[b, 0] = n
        if n == 0:
            continue
        x = np.log2(p[keep].astype(dtype))
        if other is not None:
            x = np.log2(o[keep].astype(dtype)) - x
        total = np.cumsum(x, dtype=dtype)[-1] if dtype == np.float32 else x.sum()
        mean = dtype(total / dtype(n))
        dev = x - mean
        sq = dev * dev
        ss = np.cumsum(sq, dtype=dtype)[-1] if dtype == np.float32 else sq.sum()
        out[b, 1], out[b, 2] = mean, np.sqrt(dtype(ss / dtype(n)))
    return out


def semitones(period_from, period_to):
    """12 log2 of the pitch ratio between two periods in samples"""
    return 12.0 * np.log2(np.asarray(period_from, dtype=np.float64) / np.asarray(period_to, dtype=np.float64))
