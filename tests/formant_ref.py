"""NumPy restatement of taco_frames_formant (include/taco_hip.h), built on tests/pitch_ref.py's log-envelope: the formant shift of
magnitude frames -- the envelope read at k * s_b under the unmoved excitation, at unchanged frame energy.  `formant` in float64 is the
reference the device is held to; with dtype=np.float32 it is the same definition in float32 with sequential sums and serves ONLY to
size the tolerance below.  The inputs of the GPU tests are generated here too (all_cases), so that the CPU measurement runs on exactly
what the device is given.  Imports without a GPU and without the library; the constants are restated, not imported, so that
tests/test_frames_formant_host.py can hold the header and tacotron_amd.lib to them."""
import numpy as np

from tests import pitch_ref as pr

ONE, MIN_STEP, MAX_STEP, MAX_LIFTER, FLOOR = 65536, 32768, 131072, 64, 1e-8

# The bound on |device - fp64| / fp64 over `out`.  Measured, not guessed: the float32 restatement against the float64 one on exactly
# the inputs of tests/test_gpu_frames_formant.py (all_cases below; tests/test_frames_formant_host.py repeats the measurement and holds
# this constant to it).  Times 4 for another summation order and the few-ulp differences of the device's logf, expf and cospif.
#   6.06e-6 on `floor` (C = 129, Q = 32: combs with a tenth of their bins forced to 0, 1e-30 or 1e4; |L| reaches 18.4, and the
#   difference E' - E of two envelopes that each carry the cepstrum's rounding stands in an exponent); the production-width batch
#   (C = 1025, Q = 32, +-4 semitones) gives 4.45e-6, the mixed shapes up to 2.73e-6 (mixed_C129_Q33_F31).
# Recorded rounded up (6.2e-6), so that the last bit of another NumPy's float32 log or exp does not lift the measurement above the
# record.
MEASURED_FLOAT32_ERROR = 6.2e-6
FORMANT_RTOL = 4.0 * MEASURED_FLOAT32_ERROR

row_frames = pr.row_frames
clamp_step = pr.clamp_step


def formant_step(semitones):
    return int(round(65536.0 * 2.0 ** (-float(semitones) / 12.0)))


def check_lifter(C, Q):
    assert C >= 9 and (C - 1) & (C - 2) == 0 and 1 <= Q <= min(MAX_LIFTER, (C - 1) // 2), (C, Q)


def _seq_sum(x, dtype):
    """sum over axis 0, one rounded addition per element in ascending order"""
    acc = np.zeros(x.shape[1:], dtype=dtype)
    for k in range(x.shape[0]):
        acc = acc + x[k]
    return acc


def moved_envelope(E, step_q):
    """E (C, ...) -> E' (C, ...) in E's dtype: E read at p = k * s, between bins i = p >> 16 and i + 1 with weight (p & 0xFFFF) 2^-16,
    and held at E[C - 1] from the top bin on"""
    C = E.shape[0]
    p = np.arange(C, dtype=np.int64) * clamp_step(step_q)
    i, frac = p >> 16, p & 0xFFFF
    w = (frac.astype(np.float64) / 65536.0).astype(E.dtype).reshape((-1,) + (1,) * (E.ndim - 1))   # exact in float32
    inner = i < C - 1
    i0 = np.where(inner, i, 0)
    Ep = E[i0] + w * (E[i0 + 1] - E[i0])
    return np.where(inner.reshape(w.shape), Ep, E[C - 1][None])


def formant_frames(m, step_q, Q, dtype=np.float64):
    """m (C, n) magnitudes of n frames -> (C, n) in `dtype`: the definition of taco_frames_formant at one step_q"""
    m = np.asarray(m).astype(dtype)
    _, E = pr.log_envelope(m, Q, dtype)
    y = m * np.exp(moved_envelope(E, step_q) - E)
    if dtype == np.float64:
        P0, P1 = (m * m).sum(axis=0), (y * y).sum(axis=0)
    else:
        P0, P1 = _seq_sum(m * m, dtype), _seq_sum(y * y, dtype)
    with np.errstate(divide='ignore', invalid='ignore'):
        g = np.where(P1 == 0, dtype(1.0), np.sqrt(P0 / P1)).astype(dtype)
    return y * g[None]


def formant(mag_t, frames=None, step_q=None, frames_per_unit=1, lifter=32, dtype=np.float64):
    """mag_t (B, C, F) float32 -> out (B, C, F) in `dtype`.  frames / step_q: None or B integers.  A row at step 65536 is the row
    itself; zeros behind F_b; nothing behind F_b is read."""
    mag_t = np.asarray(mag_t)
    assert mag_t.dtype == np.float32 and mag_t.ndim == 3
    B, C, F = mag_t.shape
    check_lifter(C, lifter)
    out = np.zeros((B, C, F), dtype=dtype)
    for b in range(B):
        Fb = row_frames(None if frames is None else frames[b], frames_per_unit, F)
        s = ONE if step_q is None else clamp_step(step_q[b])
        if Fb:
            out[b, :, :Fb] = mag_t[b, :, :Fb] if s == ONE else formant_frames(mag_t[b, :, :Fb], s, lifter, dtype)
    return out


# ---- the inputs of the GPU tests -----------------------------------------------------------------------------------------------------
EDGE_F = (1, 31, 32, 33, 65)                 # the kernel's frame tile is 32
SHAPES = ((9, (1, 4)), (17, (1, 8)), (129, (1, 32, 33, 64)))   # C, and Q = 1, the largest, and both sides of 32 at C = 129
# +-3 semitones, both ends of the range, and one value on the far side of each end (the device clamps those)
STEPS = (formant_step(3), formant_step(-3), MIN_STEP, MAX_STEP, MIN_STEP - 1000, MAX_STEP + 1000)
REPLAYS = (('first', (40, 9, 0), (ONE, 40000, 100000)), ('second', (3, 40, 33), (MAX_STEP, ONE, 60000)))


def moving_comb(C, F, seed=0):
    """(C, F) float32 magnitudes: harmonics as a raised-cosine ripple of the log-magnitude under two formant-like bumps whose places
    and heights move from frame to frame (seeded), over a moving tilt, and some jitter"""
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


def floor_frames(C=129, F=6):
    """row 0: all zeros; rows 1 to 3: a comb with a tenth of its bins forced to 0, 1e-30 or 1e4, at both ends of the range and at +3
    semitones; row 4: zeros but one bin.  A tenth, not more: 1e-30 exp(E' - E) must stay a normal float32 (above 1.2e-38) for a
    relative bound to mean anything, and with most of the bins forced the envelope swings by more than the 18 that leaves"""
    rng = np.random.default_rng(77)
    x = np.zeros((5, C, F), dtype=np.float32)
    for b in (1, 2, 3):
        x[b] = pr.comb(C, F, spacing=6.4, seed=7 + b)[0]
        forced = rng.choice(np.array([0.0, 1e-30, 1e4], dtype=np.float32), size=(C, F))
        hit = rng.random((C, F)) < 0.1
        x[b][hit] = forced[hit]
    x[4, C // 3] = 3.0
    return x, (40000, MIN_STEP, 55109, MAX_STEP, 99999)


def small_batch(seed, B=3, C=33, F=40):
    return np.stack([moving_comb(C, F, seed=100 * seed + b) for b in range(B)])


def all_cases():
    """(name, mag_t, frames, frames_per_unit, step_q, Q) of every comparison against the float64 restatement"""
    i = 0
    for C, Qs in SHAPES:
        for Q in Qs:
            for F in EDGE_F:
                x, frames = mixed(C, F, seed=1000 * C + 10 * Q + F)
                yield 'mixed_C%d_Q%d_F%d' % (C, Q, F), x, frames, 1, tuple(STEPS[(i + b) % len(STEPS)] for b in range(3)), Q
                i += 1
    x, frames = production()
    yield 'production', x, frames, 1, (formant_step(4), formant_step(-4)), 32
    x, steps = floor_frames()
    yield 'floor', x, None, 1, steps, 32
    yield 'beside_one', small_batch(4), (40, 40, 31), 1, (formant_step(2), ONE, formant_step(-7)), 16
    yield 'past_2_31', small_batch(2, B=2), (2 ** 30, -2 ** 30), 1000, (55555, 77777), 16
    yield 'per_unit_3', small_batch(3), (3, 15, 0), 3, (55555, 77777, MIN_STEP), 16
    yield 'refusal_good', small_batch(7, B=2, C=17, F=8), (8, 5), 1, (40000, ONE), 4
    for name, frames, steps in REPLAYS:
        yield 'replay_' + name, small_batch(8), frames, 1, steps, 16


def rel_err(got, want):
    """largest |got - want| / want over the elements where want > 0 (elsewhere both must be exactly 0)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    pos = want > 0
    assert not got[~pos].any()
    return float((np.abs(got[pos] - want[pos]) / want[pos]).max()) if pos.any() else 0.0
