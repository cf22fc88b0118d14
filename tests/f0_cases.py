"""The inputs of tests/test_gpu_frames_f0.py, generated from seeds: one list, so that the CPU measurement that sizes
tests.f0_ref.F0_ACF_ATOL and F0_STATS_ATOL (tests/test_frames_f0_host.py) runs on exactly what the device is given.  No GPU, no
library."""
from collections import namedtuple

import numpy as np

from tests import f0_ref as fr
from tests import pitch_ref as pr
from tests.pitch_cases import mags, nan_behind

Case = namedtuple('Case', 'name x frames per_unit weight gain lag_min lag_max ratio threshold')
StatsCase = namedtuple('StatsCase', 'name period other frames per_unit')

MIXED_FRAMES = (23, 0, 5, 13, 23)
EDGE_F = (1, 31, 32, 33, 63, 64, 65, 129)     # the kernel's frame tile is 32: one case on each side of an edge, and 1 and 129
# (C, lag_min, lag_max): L = 16 (every lag C = 17 has), 3 (one lag), 32 (exactly one tile of lags) and 19
SMALL = ((17, 2, 15), (17, 5, 5), (33, 2, 31), (33, 4, 20))
# L = 33, 64, 65 (a straddled tile, two full ones, two and one row), 33 again away from lag 2; 512: the cap, two tiles per wave
LAG_PATHS = ((129, 2, 32), (129, 2, 63), (129, 2, 64), (129, 60, 90), (1025, 40, 549))
REPLAYS = (('first', (40, 9, 0)), ('second', (3, 40, 33)))


def small_tables(C, L, seed):
    """a per-bin weight in [0.5, 2) and a per-lag gain in [0.8, 1.5): arbitrary, so that a dropped or misplaced entry shows"""
    rng = np.random.default_rng(seed)
    return (0.5 + 1.5 * rng.random(C)).astype(np.float32), (0.8 + 0.7 * rng.random(L)).astype(np.float32)


def voices(B, C, F, lag_min, lag_max, seed):
    """rows of harmonic combs (pitch_ref.comb) whose period wanders over the band of lags, one row in three plain seeded
    magnitudes (pitch_cases.mags: no pitch at all, many low maxima)"""
    rng = np.random.default_rng(seed)
    x = mags(B, C, F, seed=seed)
    N = 2 * (C - 1)
    for b in range(B):
        if b % 3 == 1:
            continue
        for f in range(F):
            period = lag_min + (lag_max - lag_min) * rng.random()
            x[b, :, f] = pr.comb(C, 1, spacing=N / max(period, 2.5), seed=seed + 31 * b + f)[0][:, 0]
    return x


def mixed():
    """5 rows x 23 frames at the production bin count and tables: combs, noise, and row 4 the comb of the acoustic check"""
    w, g, lag_min, lag_max = fr.tables()
    x = voices(5, 1025, 23, lag_min, lag_max, seed=0)
    x[4] = pr.comb(1025, 23, seed=4)[0]
    return Case('mixed', nan_behind(x, MIXED_FRAMES), MIXED_FRAMES, 1, w.astype(np.float32), g.astype(np.float32), lag_min, lag_max,
                fr.RATIO, fr.THRESHOLD)


def small(C, lag_min, lag_max, F):
    """three rows: a cut one, two full ones; tables on odd F, none on even; the threshold 0.3, 0 and -1 in turn"""
    frames = (max(F - 3, 0), F, F)
    seed = 1000 * C + 10 * lag_max + F
    x = nan_behind(voices(3, C, F, lag_min, lag_max, seed), frames)
    w, g = small_tables(C, lag_max - lag_min + 3, seed) if F % 2 else (None, None)
    return Case('small_C%d_%d_%d_F%d' % (C, lag_min, lag_max, F), x, frames, 1, w, g, lag_min, lag_max, (0.9, 1.0, 0.5)[F % 3],
                (0.3, 0.0, -1.0)[F % 3])


def lag_path(C, lag_min, lag_max):
    F = 5
    w, g = small_tables(C, lag_max - lag_min + 3, C + lag_max)
    return Case('lags_C%d_%d_%d' % (C, lag_min, lag_max), voices(2, C, F, lag_min, lag_max, C + lag_max), (F, F - 1), 1,
                w if lag_max % 2 else None, g, lag_min, lag_max, 0.9, 0.1)


def silent(C=65, F=6):
    """row 0: all zeros; row 1: every bin 1e-30 (its square underflows); row 2: one bin of the spectrum alone -- r[n] is one cosine,
    and over lags 2 .. 5 at bin 2 of 64 it only falls: no interior maximum; row 3: a voiced comb next to them"""
    x = np.zeros((4, C, F), dtype=np.float32)
    x[1] = 1e-30
    x[2, 2] = 3.0
    x[3] = pr.comb(C, F, spacing=128.0 / 9.0, seed=5)[0]
    return Case('silent', x, None, 1, None, None, 2, 5, 0.9, 0.0)


def per_unit(r):
    """device `frames` in units of r frames at F = 40: 3 units, a product past F, and 0"""
    frames = (3, 40 // r + 2, 0)
    return Case('per_unit_%d' % r, nan_behind(voices(3, 33, 40, 3, 30, seed=r), frames, r), frames, r, None, None, 3, 30, 0.9, 0.0)


def all_cases():
    """every comparison against the float64 restatement"""
    yield mixed()
    for C, lo, hi in SMALL:
        for F in EDGE_F:
            yield small(C, lo, hi, F)
    yield silent()
    for C, lo, hi in LAG_PATHS:
        yield lag_path(C, lo, hi)
    for r in (2, 3, 5):
        yield per_unit(r)
    yield Case('past_2_31', voices(2, 33, 40, 3, 30, seed=2), (2 ** 30, -2 ** 30), 1000, None, None, 3, 30, 0.9, 0.0)
    yield Case('refusal_good', voices(2, 17, 8, 2, 15, seed=7), (8, 5), 1, None, None, 3, 12, 0.9, 0.0)
    for name, frames in REPLAYS:
        yield Case('replay_' + name, voices(3, 33, 40, 2, 31, seed=8), frames, 1, None, None, 2, 31, 0.9, 0.0)


def acf_err(got, want):
    """largest |got - want| over the elements; where want is exactly 0 (unvoiced frames, frames behind a row) got must be too"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    dead = ~want.any(axis=-2, keepdims=True) & np.ones(want.shape, dtype=bool)
    assert not got[dead].any()
    return float(np.abs(got - want).max())


def track(F, seed, voiced=0.7, lo=40.0, hi=266.0):
    """a row of F periods in samples as taco_frames_f0 leaves them: a share `voiced` in [lo, hi), the rest 0"""
    rng = np.random.default_rng(seed)
    p = (lo + (hi - lo) * rng.random(F)).astype(np.float32)
    p[rng.random(F) >= voiced] = 0.0
    return p


def stats_cases():
    """rows with no, one and many voiced frames (700: three trips of a 256-thread workgroup), NaN behind a cut row; paired with a
    track that is partly unvoiced itself"""
    F = 700
    period = np.stack([np.zeros(F, dtype=np.float32), track(F, 1), track(F, 2, 1.0), track(F, 3)])
    period[1, 5:] = 0.0
    period[1, :5] = (0.0, 0.0, 123.456, 0.0, 0.0)          # one voiced frame
    frames = (F, F, F, 411)
    period[3, 411:] = np.nan
    other = np.stack([track(F, 11), track(F, 12, 1.0), track(F, 13, 0.6), track(F, 14, 0.5)])
    other[3, 411:] = np.nan
    yield StatsCase('unpaired', period, None, frames, 1)
    yield StatsCase('paired', period, other, frames, 1)
    yield StatsCase('null_frames', period[:3], other[:3], None, 1)
    yield StatsCase('per_unit', period, None, (1, 2 ** 30, 0, 137), 3)
    yield StatsCase('short', np.stack([track(33, 21), track(33, 22, 0.2)]), None, (33, 20), 1)


def stats_err(got, want):
    """largest error of the mean and of the standard deviation; the counts must agree exactly"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.array_equal(got[:, 0], want[:, 0]), (got[:, 0], want[:, 0])
    return float(np.abs(got[:, 1:] - want[:, 1:]).max())
