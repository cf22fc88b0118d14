"""NumPy restatements of taco_frames_pitch (include/taco_hip.h): the envelope-preserving pitch shift of magnitude frames.
`shift` in float64 is the reference the device is held to; `shift(..., dtype=np.float32)` is the same definition in float32 with
sequential sums (every product and every addition rounded, bins and quefrencies in ascending order) and serves ONLY to size the
tolerance: PITCH_RTOL below.  Imports without a GPU and without the library; the constants are restated, not imported, so that
tests/test_frames_pitch_host.py can hold the header and tacotron_amd.lib to them."""
import numpy as np

ONE, MIN_STEP, MAX_STEP, MAX_LIFTER, FLOOR = 65536, 32768, 131072, 64, 1e-8

# The bound on |device - fp64| / fp64 over `out`.  Measured, not guessed: the float32 restatement against the float64 one on exactly
# the inputs of tests/test_gpu_frames_pitch.py (tests/pitch_cases.all_cases; tests/test_frames_pitch_host.py repeats the
# measurement and holds this constant to it).  Largest relative error over all of them: 2.07e-5, on the frames that mix 0, 1e-30
# and 1e4 (|L| reaches 18.4, one rounding of it is 9.5e-7, and the cepstrum of a frame that jumps by 27.6 between neighbouring bins
# collects many of them); the mixed batch at C = 1025 gives 1.3e-6, the small shapes up to 5.0e-6.  Times 4 for another summation
# order and the few-ulp differences of the device's logf, expf and cosine.
MEASURED_FLOAT32_ERROR = 2.07e-5
PITCH_RTOL = 4.0 * MEASURED_FLOAT32_ERROR


def clamp_step(step_q):
    return min(max(int(step_q), MIN_STEP), MAX_STEP)


def row_frames(frames_b, frames_per_unit, F):
    """F_b: frames[b] * frames_per_unit (Python integers: no overflow) clamped to [0, F]; None: F"""
    if frames_b is None:
        return int(F)
    return min(max(int(frames_b) * int(frames_per_unit), 0), int(F))


def pitch_step(semitones):
    return int(round(65536.0 * 2.0 ** (-float(semitones) / 12.0)))


def _cosines(C, Q, dtype):
    N = 2 * (C - 1)
    n, k = np.arange(Q + 1, dtype=np.int64)[:, None], np.arange(C, dtype=np.int64)[None, :]
    return np.cos(2.0 * np.pi * ((n * k) % N).astype(np.float64) / N).astype(dtype)   # (Q + 1, C)


def cepstrum(L, Q):
    """c[n], n = 0 .. Q, of log-magnitudes L (C, ...) in L's dtype: float64 as one product, float32 bin by bin"""
    C = L.shape[0]
    N = 2 * (C - 1)
    cs = _cosines(C, Q, L.dtype)
    wt = np.full(C, 2.0, dtype=L.dtype)
    wt[0] = wt[-1] = 1.0
    if L.dtype == np.float64:
        return np.tensordot(cs * wt[None, :], L, axes=(1, 0)) / N
    acc = np.zeros((Q + 1,) + L.shape[1:], dtype=np.float32)
    for k in range(C):   # sequential: one rounded product and one rounded addition per bin
        acc = acc + cs[:, k].reshape((-1,) + (1,) * (L.ndim - 1)) * (wt[k] * L[k])[None]
    return acc / np.float32(N)


def envelope(c, C):
    """E[k] = c[0] + 2 sum_{n >= 1} c[n] cos(2 pi n k / N) over k = 0 .. C - 1, in c's dtype"""
    Q = c.shape[0] - 1
    cs = _cosines(C, Q, c.dtype)
    if c.dtype == np.float64:
        return c[0][None] + 2.0 * np.tensordot(cs[1:].T, c[1:], axes=(1, 0))
    E = np.broadcast_to(c[0][None], (C,) + c.shape[1:]).astype(np.float32)
    for n in range(1, Q + 1):
        E = E + cs[n].reshape((-1,) + (1,) * (c.ndim - 1)) * (np.float32(2.0) * c[n])[None]
    return E


def log_envelope(m, Q, dtype=np.float64):
    """(L, E) of magnitudes m (C, ...): the log-magnitudes over the floor and their log-envelope"""
    L = np.log(np.maximum(np.asarray(m).astype(dtype), dtype(FLOOR)))
    return L, envelope(cepstrum(L, Q), L.shape[0])


def shift_frames(m, step_q, Q, dtype=np.float64):
    """m (C, n) magnitudes of n frames -> (C, n): steps 1 to 5 of the definition at one step_q"""
    C = m.shape[0]
    s = clamp_step(step_q)
    L, E = log_envelope(m, Q, dtype)
    R = L - E
    p = np.arange(C, dtype=np.int64) * s
    i, frac = p >> 16, p & 0xFFFF
    w = (frac.astype(np.float64) / 65536.0).astype(dtype)[:, None]                    # exact in float32
    inner = i < C - 1
    i0 = np.where(inner, i, 0)
    Rp = R[i0] + w * (R[i0 + 1] - R[i0])
    Rp = np.where(inner[:, None], Rp, np.where(((i == C - 1) & (frac == 0))[:, None], R[C - 1][None], dtype(0.0)))
    return np.exp(E + Rp)


def shift(mag_t, frames=None, step_q=None, frames_per_unit=1, lifter=32, dtype=np.float64):
    """mag_t (B, C, F) float32 -> out (B, C, F) in `dtype`.  frames / step_q: None or B integers.  A row at step 65536 is the
    row itself; zeros behind F_b; nothing behind F_b is read."""
    mag_t = np.asarray(mag_t)
    assert mag_t.dtype == np.float32 and mag_t.ndim == 3
    B, C, F = mag_t.shape
    assert C >= 9 and (C - 1) & (C - 2) == 0 and 1 <= lifter <= min(MAX_LIFTER, (C - 1) // 2)
    out = np.zeros((B, C, F), dtype=dtype)
    for b in range(B):
        Fb = row_frames(None if frames is None else frames[b], frames_per_unit, F)
        s = ONE if step_q is None else clamp_step(step_q[b])
        if Fb == 0:
            continue
        out[b, :, :Fb] = mag_t[b, :, :Fb] if s == ONE else shift_frames(mag_t[b, :, :Fb], s, lifter, dtype)
    return out


def comb(C=1025, F=24, spacing=12.8, seed=0):
    """(mag (C, F) float32, the smooth log-envelope it was built under (C,)): harmonics every `spacing` bins (100 Hz at 16 kHz and
    C = 1025) as raised-cosine ripples of the log-magnitude, under two formant-like bumps; a little seeded frame-to-frame jitter"""
    k = np.arange(C, dtype=np.float64)
    env = 1.2 * np.exp(-0.5 * ((k - 0.12 * C) / (0.06 * C)) ** 2) + 0.9 * np.exp(-0.5 * ((k - 0.4 * C) / (0.1 * C)) ** 2) - 2.0 * k / C
    env = (env - env.mean()) / env.std()                      # spread 1.0
    ripple = 1.5 * np.cos(2.0 * np.pi * k / spacing)
    rng = np.random.default_rng(seed)
    jitter = 0.01 * rng.standard_normal((C, F))
    return np.exp(env[:, None] + ripple[:, None] + jitter).astype(np.float32), env


def peak_spacing(m, lo, hi):
    """mean distance between neighbouring local maxima of log m over bins [lo, hi)"""
    x = np.log(np.asarray(m, dtype=np.float64))
    k = np.arange(max(lo, 1), min(hi, len(x) - 1))
    peaks = k[(x[k] > x[k - 1]) & (x[k] >= x[k + 1])]
    return float(np.diff(peaks).mean())


def f0_lag(y, sr=16000, lo=60.0, hi=400.0):
    """(lag, value) of the largest normalised autocorrelation of waveform y over the lags of `hi` down to `lo` Hz"""
    y = np.asarray(y, dtype=np.float64)
    y = y - y.mean()
    lags = np.arange(int(sr / hi), int(sr / lo) + 1)
    r = np.array([np.dot(y[:-l], y[l:]) / np.sqrt(np.dot(y[:-l], y[:-l]) * np.dot(y[l:], y[l:])) for l in lags])
    return int(lags[r.argmax()]), float(r.max())
