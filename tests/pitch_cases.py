"""The inputs of tests/test_gpu_frames_pitch.py, generated from seeds: one list, so that the CPU measurement that sizes
tests.pitch_ref.PITCH_RTOL (tests/test_frames_pitch_host.py) runs on exactly what the device is given.  No GPU, no library."""
import numpy as np

from tests import pitch_ref as pr

MIXED_FRAMES = (23, 0, 5, 13, 23)
MIXED_STEPS = (65536, 70000, 32768, 131072, 61858)
EDGE_F = (1, 31, 32, 33, 63, 64, 65, 129)        # the kernel's frame tile is 32: one case on each side of an edge, and 1 and 129
SMALL = ((17, 1), (17, 3), (17, 8), (33, 16))    # (C, Q)
REPLAYS = (('first', (40, 9, 0), (65536, 40000, 100000)), ('second', (3, 40, 33), (131072, 65536, 60000)))
LIFTER_PATHS = ((129, 32), (129, 33), (129, 64), (1025, 64))   # Q = 32 | 33: one or two blocks of 32 quefrencies


def mags(B, C, F, seed=0, zeros=0.0):
    """magnitudes as exp() leaves them: positive, over many binades; a share `zeros` of the bins exactly 0"""
    rng = np.random.default_rng(seed)
    x = np.exp(rng.standard_normal((B, C, F)) * 2.0).astype(np.float32)
    if zeros:
        x[rng.random((B, C, F)) < zeros] = 0.0
    return x


def nan_behind(x, frames, per_unit=1):
    x = x.copy()
    for b, f in enumerate(frames):
        x[b, :, pr.row_frames(f, per_unit, x.shape[2]):] = np.nan
    return x


def mixed():
    x = mags(5, 1025, 23, seed=0)
    x[4] = pr.comb(1025, 23, seed=4)[0]
    return nan_behind(x, MIXED_FRAMES)


def small(C, Q, F):
    """three rows: a cut one going up, a full one going down, a full one at an odd step"""
    frames = (max(F - 3, 0), F, F)
    x = nan_behind(mags(3, C, F, seed=1000 * C + 10 * Q + F, zeros=0.1 if F % 2 else 0.0), frames)
    return x, frames, (40000, 131072, 65537)


def floor_frames(C=65, F=6):
    """row 0: all zeros; row 1: 0, 1e-30 and 1e4 mixed (two thirds of the bins under the floor); row 2: zeros but one bin"""
    rng = np.random.default_rng(77)
    x = np.zeros((3, C, F), dtype=np.float32)
    x[1] = rng.choice(np.array([0.0, 1e-30, 1e4], dtype=np.float32), size=(C, F))
    x[2, C // 3] = 3.0
    return x, (50000, 80000, 99999)


def lifter_path(C, Q):
    F = 5
    return mags(2, C, F, seed=C + Q, zeros=0.1), (F, F - 1), (45000, 100000)


def per_unit(r):
    """device `frames` in units of r frames at F = 40: 3 units, a product past F, and 0"""
    frames = (3, 40 // r + 2, 0)
    return nan_behind(mags(3, 33, 40, seed=r), frames, r), frames, (55555, 77777, 32768)


def all_cases():
    """(name, mag_t, frames, step_q, frames_per_unit, Q) of every comparison against the float64 restatement"""
    yield 'mixed', mixed(), MIXED_FRAMES, MIXED_STEPS, 1, 32
    for C, Q in SMALL:
        for F in EDGE_F:
            x, fr, st = small(C, Q, F)
            yield 'small_C%d_Q%d_F%d' % (C, Q, F), x, fr, st, 1, Q
    x, st = floor_frames()
    yield 'floor', x, None, st, 1, 32
    for C, Q in LIFTER_PATHS:
        x, fr, st = lifter_path(C, Q)
        yield 'lifter_C%d_Q%d' % (C, Q), x, fr, st, 1, Q
    for r in (2, 3, 5):
        x, fr, st = per_unit(r)
        yield 'per_unit_%d' % r, x, fr, st, r, 16
    x, _, st = per_unit(2)
    yield 'past_2_31', mags(2, 33, 40, seed=2), (2 ** 30, -2 ** 30), st[:2], 1000, 16
    yield 'clamped', mags(3, 17, 9, seed=5), None, (0, -5, 2 ** 30), 1, 4
    yield 'refusal_good', mags(2, 17, 8, seed=7), (8, 5), (40000, 65536), 1, 4
    for name, fr, st in REPLAYS:
        yield 'replay_' + name, mags(3, 33, 40, seed=8), fr, st, 1, 16


def rel_err(got, want):
    """largest |got - want| / want over the elements where want > 0 (elsewhere both must be exactly 0)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    pos = want > 0
    assert not got[~pos].any()
    return float((np.abs(got[pos] - want[pos]) / want[pos]).max()) if pos.any() else 0.0
