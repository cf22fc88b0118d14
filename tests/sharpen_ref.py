"""NumPy restatements of taco_frames_sharpen and taco_frames_cepstats (include/taco_hip.h), built on tests/pitch_ref.py's cepstrum:
the cepstral post-filter, the per-row sums of the cepstra and their squares, and the global-variance ratio made of them.  `sharpen`
and `cepstats` in float64 are the references the device is held to; with dtype=np.float32 they are the same definitions in float32
with sequential sums and serve ONLY to size the two tolerances below.  The inputs of the GPU tests are generated here too
(all_cases), so that the CPU measurement runs on exactly what the device is given.  Imports without a GPU and without the library;
the constants are restated, not imported, so that tests/test_frames_sharpen_host.py can hold the header and tacotron_amd.lib to them."""
import numpy as np

from tests import pitch_ref as pr

FIRST, MIN_BETA, MAX_BETA, MAX_LIFTER, FLOOR = 2, -1.0, 1.0, 64, 1e-8

# The bounds on |device - fp64| / fp64: over `out` for the post-filter, over var[n], n >= 1, of every row with two frames or more for
# the statistics.  Measured, not guessed: the float32 restatements against the float64 ones on exactly the inputs of
# tests/test_gpu_frames_sharpen.py and tests/test_gpu_frames_cepstats.py (all_cases below; tests/test_frames_sharpen_host.py repeats
# the measurement and holds these constants to it).  Times 4 for another summation order and the few-ulp differences of the device's
# logf, expf and cospif.
#   out: 1.55e-6 on the production-width batch (C = 1025, Q = 32, beta = 0.4: a thousand roundings per cepstral coefficient, and D
#        collects 31 of them); the small shapes give up to 1.13e-6 (mixed_C129_Q32_F32).
#   var: 7.31e-6 on replay_second (C = 33, Q = 16; its first row has 3 frames: the variance of a few frames is a small difference
#        of two sums, each carrying the cepstrum's rounding); the production-width batch gives 1.57e-6, the mixed shapes up to 4.9e-7.
# Recorded rounded up (1.6e-6, 7.5e-6), so that the last bit of another NumPy's float32 log or exp does not lift the measurement
# above the record.
MEASURED_FLOAT32_ERROR = {'sharpen': 1.6e-6, 'cepstats': 7.5e-6}
SHARPEN_RTOL = 4.0 * MEASURED_FLOAT32_ERROR['sharpen']
CEPSTATS_RTOL = 4.0 * MEASURED_FLOAT32_ERROR['cepstats']

row_frames = pr.row_frames


def check_lifter(C, Q):
    assert C >= 9 and (C - 1) & (C - 2) == 0 and FIRST <= Q <= min(MAX_LIFTER, (C - 1) // 2), (C, Q)


def _seq_sum(x, dtype):
    """sum over axis 0, one rounded addition per element in ascending order"""
    acc = np.zeros(x.shape[1:], dtype=dtype)
    for k in range(x.shape[0]):
        acc = acc + x[k]
    return acc


def sharpen_frames(m, beta, Q, dtype=np.float64):
    """m (C, n) magnitudes of n frames -> (C, n) in `dtype`: the definition of taco_frames_sharpen at one beta"""
    m = np.asarray(m).astype(dtype)
    C = m.shape[0]
    L = np.log(np.maximum(m, dtype(FLOOR)))
    c = pr.cepstrum(L, Q)
    cs = pr._cosines(C, Q, dtype)
    b2 = dtype(2.0) * dtype(beta)
    if dtype == np.float64:
        D = b2 * np.tensordot(cs[FIRST:].T, c[FIRST:], axes=(1, 0))
        y = m * np.exp(D)
        P0, P1 = (m * m).sum(axis=0), (y * y).sum(axis=0)
    else:
        D = np.zeros_like(m)
        for n in range(FIRST, Q + 1):
            D = D + cs[n][:, None] * (b2 * c[n])[None]
        y = m * np.exp(D)
        P0, P1 = _seq_sum(m * m, dtype), _seq_sum(y * y, dtype)
    with np.errstate(divide='ignore', invalid='ignore'):
        g = np.where(P1 == 0, dtype(1.0), np.sqrt(P0 / P1)).astype(dtype)
    return y * g[None]


def sharpen(mag_t, beta, frames=None, frames_per_unit=1, lifter=32, dtype=np.float64):
    """mag_t (B, C, F) float32 -> out (B, C, F) in `dtype`.  beta == 0 is the input itself; zeros behind F_b; nothing behind F_b is
    read."""
    mag_t = np.asarray(mag_t)
    assert mag_t.dtype == np.float32 and mag_t.ndim == 3 and MIN_BETA <= beta <= MAX_BETA
    B, C, F = mag_t.shape
    check_lifter(C, lifter)
    out = np.zeros((B, C, F), dtype=dtype)
    for b in range(B):
        Fb = row_frames(None if frames is None else frames[b], frames_per_unit, F)
        if Fb:
            out[b, :, :Fb] = mag_t[b, :, :Fb] if beta == 0 else sharpen_frames(mag_t[b, :, :Fb], beta, lifter, dtype)
    return out


def cepstra(m, Q, dtype=np.float64):
    """c[n], n = 0 .. Q, of magnitudes m (C, ...) -> (Q + 1, ...) in `dtype`"""
    return pr.cepstrum(np.log(np.maximum(np.asarray(m).astype(dtype), dtype(FLOOR))), Q)


def cepstats(mag_t, frames=None, frames_per_unit=1, lifter=32, dtype=np.float64):
    """mag_t (B, C, F) float32 -> (sums (B, Q + 1, 2) float64, count (B) int64): the cepstra in `dtype`, their sums in float64"""
    mag_t = np.asarray(mag_t)
    assert mag_t.dtype == np.float32 and mag_t.ndim == 3
    B, C, F = mag_t.shape
    check_lifter(C, lifter)
    sums, count = np.zeros((B, lifter + 1, 2)), np.zeros(B, dtype=np.int64)
    for b in range(B):
        Fb = count[b] = row_frames(None if frames is None else frames[b], frames_per_unit, F)
        if Fb:
            c = cepstra(mag_t[b, :, :Fb], lifter, dtype).astype(np.float64)
            sums[b, :, 0], sums[b, :, 1] = c.sum(axis=1), (c * c).sum(axis=1)
    return sums, count


def variance(sums, count):
    """var (..., Q + 1) = sums[n, 1] / count - (sums[n, 0] / count)^2 in float64; NaN where count < 2"""
    sums, count = np.asarray(sums, dtype=np.float64), np.asarray(count, dtype=np.float64)[..., None]
    with np.errstate(divide='ignore', invalid='ignore'):
        var = sums[..., 1] / count - (sums[..., 0] / count) ** 2
    return np.where(count >= 2, var, np.nan)


def gv_ratio(sums_pred, n_pred, sums_rec, n_rec):
    """exp(mean over n = 1 .. Q of log(var_pred[n] / var_rec[n])) per utterance; NaN with fewer than 2 frames on either side"""
    vp, vr = variance(sums_pred, n_pred)[..., 1:], variance(sums_rec, n_rec)[..., 1:]
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.exp(np.log(vp / vr).mean(axis=-1))


# ---- the inputs of the GPU tests -----------------------------------------------------------------------------------------------------
EDGE_F = (1, 31, 32, 33, 65)                 # the kernels' frame tile is 32
SHAPES = ((9, (2, 4)), (17, (2, 8)), (129, (2, 32, 33, 64)))   # C, and Q = 2, the largest, and both sides of 32 at C = 129
BETAS = (0.4, -0.4, 1.0, -1.0, 0.25)
REPLAYS = (('first', (40, 9, 0)), ('second', (3, 40, 33)))


def moving_comb(C, F, seed=0):
    """(C, F) float32 magnitudes: harmonics as a raised-cosine ripple of the log-magnitude under two formant-like bumps whose places
    and heights move from frame to frame (seeded), over a moving tilt, and some jitter -- so the variance over the frames of every
    cepstral coefficient is not tiny against its squared mean"""
    rng = np.random.default_rng(seed)
    k = np.arange(C, dtype=np.float64)[:, None] / C
    p1, p2 = 0.12 + 0.05 * rng.standard_normal(F), 0.4 + 0.08 * rng.standard_normal(F)
    h1, h2 = 1.2 + 0.5 * rng.standard_normal(F), 0.9 + 0.5 * rng.standard_normal(F)
    tilt = 2.0 + 0.7 * rng.standard_normal(F)
    env = h1 * np.exp(-0.5 * ((k - p1) / 0.06) ** 2) + h2 * np.exp(-0.5 * ((k - p2) / 0.1) ** 2) - tilt * k
    ripple = (1.0 + 0.3 * rng.standard_normal(F)) * np.cos(2.0 * np.pi * k * C / max(C / 80.0, 3.1))
    return np.exp(env + ripple + 0.3 * rng.standard_normal((C, F))).astype(np.float32)


def mixed(C, F, seed):
    """B = 3: a moving comb cut 3 frames short (NaN behind), a full row of zeros, and an empty row (NaN throughout)"""
    frames = (max(F - 3, 1), F, 0)
    x = np.zeros((3, C, F), dtype=np.float32)
    x[0] = moving_comb(C, F, seed)
    x[0, :, frames[0]:] = np.nan
    x[2] = np.nan
    return x, frames


def production():
    x = np.stack([moving_comb(1025, 40, seed=1), moving_comb(1025, 40, seed=2)])
    x[1, :, 37:] = np.nan
    return x, (40, 37)


def small_batch(seed, B=3, C=33, F=40):
    return np.stack([moving_comb(C, F, seed=100 * seed + b) for b in range(B)])


def all_cases():
    """(name, mag_t, frames, frames_per_unit, beta, Q) of every comparison against the float64 restatements"""
    i = 0
    for C, Qs in SHAPES:
        for Q in Qs:
            for F in EDGE_F:
                x, frames = mixed(C, F, seed=1000 * C + 10 * Q + F)
                yield 'mixed_C%d_Q%d_F%d' % (C, Q, F), x, frames, 1, BETAS[i % len(BETAS)], Q
                i += 1
    x, frames = production()
    yield 'production', x, frames, 1, 0.4, 32
    yield 'past_2_31', small_batch(2, B=2), (2 ** 30, -2 ** 30), 1000, 0.5, 16
    yield 'per_unit_3', small_batch(3), (3, 15, 0), 3, -0.7, 16
    yield 'refusal_good', small_batch(7, B=2, C=17, F=8), (8, 5), 1, 0.4, 4
    for name, frames in REPLAYS:
        yield 'replay_' + name, small_batch(8), frames, 1, 0.6, 16


def rel_err(got, want):
    """largest |got - want| / want over the elements where want > 0 (elsewhere both must be exactly 0)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    pos = want > 0
    assert not got[~pos].any()
    return float((np.abs(got[pos] - want[pos]) / want[pos]).max()) if pos.any() else 0.0


def var_err(sums, count, want_sums, want_count):
    """largest relative error of var[n], n >= 1, over the rows with two frames or more whose frames differ (a row of equal frames
    has variance 0 in the reference: there |var| must stay below 1e-12 of 1 + mean^2); the counts must be equal"""
    assert np.array_equal(np.asarray(count, dtype=np.int64), np.asarray(want_count, dtype=np.int64))
    got, want = variance(sums, count)[..., 1:], variance(want_sums, want_count)[..., 1:]
    worst = 0.0
    for b in range(len(want_count)):
        if want_count[b] < 2:
            continue
        mean2 = (np.asarray(want_sums)[b, 1:, 0] / want_count[b]) ** 2
        flat = want[b] <= 1e-12 * (1.0 + mean2)
        assert (np.abs(got[b][flat]) <= 1e-12 * (1.0 + mean2[flat])).all()
        if (~flat).any():
            worst = max(worst, float((np.abs(got[b] - want[b])[~flat] / want[b][~flat]).max()))
    return worst
