"""The inputs of tests/test_gpu_f0_range.py, generated from seeds: one list, so that the CPU measurement that sizes
tests.f0_range_ref.F0_RANGE_STEP_ATOL (tests/test_f0_range_host.py) runs on exactly what the device is given.  The smallest shapes
at which the kernel can go wrong: a workgroup of 256 threads per row, one 64-bit ballot word per 64 frames.  No GPU, no library."""
from collections import namedtuple

import numpy as np

from tests import f0_range_ref as rr

Case = namedtuple('Case', 'name period frames per_unit scale_q base_q smooth limit')

FS = (1, 5, 63, 64, 65, 128, 256, 257, 700, 8192)
SCALES = (0.0, 0.5, 1.0, 1.5, 4.0)
SMOOTHS = (0, 1, 2, 8)
LO, HI = 40.0, 266.0                  # the tracker's range of periods in samples


def contour(F, seed, amp=0.45, cycles=2.5, jitter=0.02):
    """F periods in [40, 266] samples: a slow sinusoid of log2(period) around 7 (128 samples: 125 Hz at 16 kHz) with a little
    seeded jitter; amp 0.45 octaves reaches 94 .. 175 samples"""
    rng = np.random.default_rng(seed)
    f = np.arange(F, dtype=np.float64)
    x = 7.0 + amp * np.sin(2.0 * np.pi * (cycles * f / max(F, 40) + rng.random())) + jitter * rng.standard_normal(F)
    return np.clip(2.0 ** x, LO, HI).astype(np.float32)


def q(k):
    return int(round(65536.0 * k))


# voiced patterns over the live frames of a row: name -> mask(Fb, rng)
def _gaps(*spans):
    def make(Fb, rng):
        m = np.ones(Fb, dtype=bool)
        for a, b in spans:           # frames a .. b unvoiced, both ends included
            m[a:b + 1] = False
        return m
    return make


def _only(where):
    def make(Fb, rng):
        m = np.zeros(Fb, dtype=bool)
        m[where(Fb)] = True
        return m
    return make


PATTERNS = {
    'none': lambda Fb, rng: np.zeros(Fb, dtype=bool),
    'all': lambda Fb, rng: np.ones(Fb, dtype=bool),
    'random': lambda Fb, rng: rng.random(Fb) < 0.7,
    'sparse': lambda Fb, rng: rng.random(Fb) < 0.05,
    'single_first': _only(lambda Fb: [0]),
    'single_last': _only(lambda Fb: [Fb - 1]),
    'single_middle': _only(lambda Fb: [Fb // 2]),
    'start_only': _only(lambda Fb: slice(0, min(3, Fb))),
    'end_only': _only(lambda Fb: slice(max(Fb - 3, 0), Fb)),
    'two_ends': _only(lambda Fb: [0, Fb - 1]),
}
# gaps that begin and end on the frames next to a ballot word's edge (63 | 64) and a workgroup trip's edge (255 | 256); the last
# one is longer than two ballot words; they need F_b >= 257
EDGE_GAPS = {
    'gap_63_64': _gaps((63, 64)),
    'gap_64_65': _gaps((64, 65)),
    'gap_63_63_65_65': _gaps((63, 63), (65, 65)),
    'gap_64_255': _gaps((64, 255)),
    'gap_65_256': _gaps((65, 256)),
    'gap_63_254': _gaps((63, 254)),
    'gap_255_256': _gaps((255, 256)),
    'gap_1_62_128_191': _gaps((1, 62), (128, 191)),
    'gap_70_250': _gaps((70, 250)),
}


def rows(F, frames, patterns, seed, amp=0.45):
    """(B, F) periods: row b a contour voiced by patterns[b] over its first F_b frames, NaN behind them"""
    rng = np.random.default_rng(seed)
    out = np.empty((len(patterns), F), dtype=np.float32)
    for b, name in enumerate(patterns):
        Fb = rr.row_frames(None if frames is None else frames[b], 1, F)
        p = contour(F, seed + 17 * b, amp)
        mask = ({**PATTERNS, **EDGE_GAPS}[name])(Fb, rng) if Fb else np.zeros(0, dtype=bool)
        p[:Fb][~mask] = 0.0
        p[Fb:] = np.nan
        out[b] = p
    return out


def bases(B, F, seed, wild=False):
    """a (B, F) base curve: steps of +-4 semitones in blocks of 7 frames; wild: values on both sides of the clamp as well"""
    rng = np.random.default_rng(seed)
    lo, hi = (20000, 200000) if wild else (52016, 82570)
    v = rng.integers(lo, hi + 1, size=(B, (F + 6) // 7))
    return np.repeat(v, 7, axis=1)[:, :F].astype(np.int32)


def all_cases():
    """every comparison against the float64 restatement"""
    names = list(PATTERNS)
    for i, F in enumerate(FS):       # every F with B = 1 .. 3, the settings in turn; row 1 is cut short with NaN behind it
        B = 1 + i % 3
        frames = tuple(F if b != 1 else max(F - 3, 0) for b in range(B))
        pats = [names[(2 + i + 3 * b) % len(names)] for b in range(B)]
        pats[0] = 'random'
        yield Case('F%d' % F, rows(F, frames, pats, 100 + F), frames, 1, tuple(q(SCALES[(i + 2 * b + 3) % 5]) for b in range(B)),
                   bases(B, F, F) if i % 2 else None, SMOOTHS[i % 4], rr.LIMIT)
    for j, F in enumerate((5, 65, 257)):     # every pattern that fits, at one word, two words and past a workgroup trip
        for i, name in enumerate(names):
            yield Case('%s_F%d' % (name, F), rows(F, None, [name], 200 + i), None, 1, (q(SCALES[(i + j) % 5 if (i + j) % 5 != 2 else 3]),),
                       bases(1, F, i) if (i + j) % 2 else None, SMOOTHS[(i + j) % 4], rr.LIMIT)
    for i, name in enumerate(EDGE_GAPS):
        F = (257, 700)[i % 2]
        yield Case('%s_F%d' % (name, F), rows(F, None, [name, name], 300 + i), None, 1, (q(1.5), q(0.0)), bases(2, F, i) if i % 2 else None,
                   SMOOTHS[i % 4], rr.LIMIT)
    # the scales, among them values the device clamps
    yield Case('scales_a', rows(65, None, ['random'] * 3, 400), None, 1, (q(0.0), q(0.5), q(1.0)), None, 2, rr.LIMIT)
    yield Case('scales_b', rows(65, None, ['random'] * 3, 401), None, 1, (q(1.5), q(4.0), q(1.0)), bases(3, 65, 1), 2, rr.LIMIT)
    yield Case('scales_clamped', rows(65, None, ['random'] * 2, 402), None, 1, (-5, 10 * 65536), None, 1, rr.LIMIT)
    yield Case('scale_null', rows(65, None, ['random'] * 2, 403), None, 1, None, bases(2, 65, 2, wild=True), 1, rr.LIMIT)
    # every W, also with F_b <= W
    for W in SMOOTHS:
        yield Case('smooth_%d_short' % W, rows(9, (9, 1, 4), ['random', 'all', 'two_ends'], 500 + W), (9, 1, 4), 1, (q(1.5), q(0.5), q(4.0)),
                   None, W, rr.LIMIT)
        yield Case('smooth_%d_F128' % W, rows(128, None, ['random'], 510 + W), None, 1, (q(0.5),), None, W, rr.LIMIT)
    # base values on both sides of the clamp
    yield Case('base_wild', rows(130, (130, 100), ['random', 'sparse'], 600), (130, 100), 1, (q(1.5), q(0.0)), bases(2, 130, 3, wild=True), 2,
               rr.LIMIT)
    # contours whose excursion hits the limit: 0.45 octaves x (k - 1) = 1.35, and x -1 at k = 0
    for limit in (0.25, 0.5, 1.0):
        yield Case('limit_%g' % limit, rows(200, None, ['all', 'random'], 700), None, 1, (q(4.0), q(0.0)), None, 0, limit)
    yield Case('limit_base', rows(200, None, ['random'], 701), None, 1, (q(4.0),), bases(1, 200, 4, wild=True), 2, 1.0)
    # empty rows, and frames in units
    yield Case('empty_row', rows(70, (0, 70), ['random', 'random'], 800), (0, 70), 1, (q(1.5), q(1.5)), bases(2, 70, 5), 2, rr.LIMIT)
    p = rows(40, (21, 40, 0), ['random', 'random', 'random'], 801)
    yield Case('per_unit_7', p, (3, 2 ** 30, 0), 7, (q(1.5), q(0.5), q(4.0)), None, 2, rr.LIMIT)
    yield Case('past_2_31', rows(40, (40, 0), ['random', 'random'], 802), (2 ** 30, -2 ** 30), 1000, (q(1.5), q(1.5)), None, 2, rr.LIMIT)
    # the cap: 128 ballot words, 32 trips
    yield Case('cap_gaps', rows(8192, (8192, 8000), ['sparse', 'gap_70_250'], 900), (8192, 8000), 1, (q(1.5), q(0.5)), bases(2, 8192, 6), 8,
               rr.LIMIT)
    yield Case('replay_first', rows(300, None, ['random'] * 3, 950), (300, 120, 257), 1, (q(1.5), q(0.5), q(1.0)), None, 2, rr.LIMIT)
    yield Case('replay_second', rows(300, None, ['random'] * 3, 950), (64, 300, 0), 1, (q(0.0), q(4.0), q(1.5)), None, 2, rr.LIMIT)


def step_err(got, want):
    """largest |got - want| over the elements, in step units"""
    return float(np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64)).max())
