"""The inputs of tests/test_gpu_frame_dtw_path.py, built on the host so that tests/test_frame_dtw_path_host.py can check the
restatement on exactly them (and measure the float32 error behind path_ref.PATH_SCORES_ATOL on them) without a GPU.  Every case
and its restatement are computed once per process.  Imports without a GPU and without the library."""
import functools

import numpy as np

from tests import path_ref as pr

THREADS = 256   # kDtwThreads of dtw.hip: cells of one anti-diagonal a workgroup takes per pass
GROSS = 1.2


def mel_like(rng, B, F, C=80):
    """smooth log-mel-like frames: a random walk over the frames around -5 (as tests/test_gpu_frame_dtw.py draws them)"""
    return (np.cumsum(rng.standard_normal((B, F, C)) * 0.3, axis=1) - 5.0).astype(np.float32)


def dct_basis(C=80, first=1, count=13):
    """tacotron_amd.lib.dct_basis restated (the host tests compare the two)"""
    k = np.arange(first, first + count, dtype=np.float64)[:, None]
    c = np.arange(C, dtype=np.float64)[None, :]
    rows = np.sqrt(2.0 / C) * np.cos(np.pi * (c + 0.5) * k / C)
    rows[k[:, 0] == 0] = np.sqrt(1.0 / C)
    return rows.astype(np.float32)


def _case(a, b, na, nb, basis, shift=(0, 0)):
    return {'a': a, 'b': b, 'na': na, 'nb': nb, 'basis': basis, 'shift': shift}


@functools.lru_cache(maxsize=None)
def dtw_cases():
    """{name: {'a', 'b', 'na', 'nb', 'basis', 'shift'}}"""
    out = {}
    rng = np.random.default_rng(0)                            # the 6-row core case of tests/test_gpu_frame_dtw.py
    a = rng.standard_normal((6, 12, 5)).astype(np.float32)
    b = rng.standard_normal((6, 9, 5)).astype(np.float32)
    out['small tables'] = _case(a, b, [1, 1, 7, 12, 0, 4], [1, 7, 1, 9, 5, 0], None)
    rng = np.random.default_rng(2)                            # the integer frames of its test_ties
    a = rng.integers(0, 2, (5, 40, 3)).astype(np.float32)
    b = rng.integers(0, 2, (5, 33, 3)).astype(np.float32)
    a[0], b[0] = 0.0, 0.0                                     # every cell ties
    b[1, :33] = a[1, :33]
    out['ties'] = _case(a, b, [40, 33, 40, 2, 3], [33, 33, 30, 3, 2], None)
    zeros = np.zeros((2, 3, 1), dtype=np.float32)
    out['ties, both orders'] = _case(zeros, zeros, [2, 3], [3, 2], None)
    x = rng.standard_normal((1, 21, 4)).astype(np.float32)
    out['doubled'] = _case(x, np.repeat(x, 2, axis=1), None, None, None)
    rng = np.random.default_rng(4)                            # one cell over a workgroup pass, one over a wave, thin tables
    a = rng.standard_normal((4, 300, 3)).astype(np.float32)
    b = rng.standard_normal((4, 300, 3)).astype(np.float32)
    out['diagonal lengths'] = _case(a, b, [THREADS + 1, 65, 3, 300], [THREADS + 1, 65, 300, 3], None)
    rng = np.random.default_rng(5)                            # the product shape, ragged, one float off the 256-byte alignment
    out['product shape'] = _case(mel_like(rng, 4, 360), mel_like(rng, 4, 360), [360, 301, 77, 258], [333, 360, 150, 257], dct_basis(),
                                 shift=(1, 1))
    rng = np.random.default_rng(6)                            # the coefficients do not fit LDS: they go to the workspace
    F, C, K = 1024, 24, 32
    basis = (rng.standard_normal((K, C)) / np.sqrt(C)).astype(np.float32)
    out['envelope'] = _case(mel_like(rng, 1, F, C), mel_like(rng, 1, F, C), None, None, basis)
    rng = np.random.default_rng(3)                            # the clean half of the isolation case
    a = rng.standard_normal((4, 70, 6)).astype(np.float32)
    b = rng.standard_normal((4, 50, 6)).astype(np.float32)
    out['isolation'] = _case(a, b, [70, 31, 5, 66], [50, 44, 50, 1], rng.standard_normal((4, 6)).astype(np.float32))
    return out


@functools.lru_cache(maxsize=None)
def dtw_ref(name):
    """(cost, steps, path_a, path_b) of path_ref.dtw32_path on dtw_cases()[name]; treat as read-only"""
    c = dtw_cases()[name]
    return pr.dtw32_path(c['a'], c['b'], c['na'], c['nb'], c['basis'])


def periods(rng, B, F, voiced=0.7):
    """(B, F) float32 periods in samples, 0 where unvoiced.  The voiced values sit within 0.3 % of the grid 40 * 1.07^k, k = 0 .. 28
    (40 .. 266 samples), so the ratio of any two is within 0.6 % of a power of 1.07 -- 1.145 and 1.225 are the nearest to GROSS =
    1.2: no pair is within 1e-3 (relative) of the gross threshold, and the gross count does not hang on one ulp"""
    k = rng.integers(0, 29, (B, F))
    p = 40.0 * 1.07 ** k * (1.0 + 0.003 * rng.uniform(-1.0, 1.0, (B, F)))
    run = np.cumsum(rng.standard_normal((B, F)), axis=1)      # voiced and unvoiced stretches, not salt and pepper
    lim = np.quantile(run, voiced, axis=1, keepdims=True)
    return np.where(run <= lim, p, 0.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def score_cases():
    """{name: {'period_a', 'period_b', 'path_a', 'path_b', 'steps'}}; the paths of the first are the product shape's own"""
    out = {}
    c = dtw_cases()['product shape']
    _, steps, path_a, path_b = dtw_ref('product shape')
    rng = np.random.default_rng(21)
    pa, pb = periods(rng, 4, 360), periods(rng, 4, 360)
    pa[1], pb[1] = periods(rng, 1, 360, 1.0)[0], periods(rng, 1, 360, 1.0)[0]     # row 1: every cell voiced in both
    pa[2], pb[2, ::2] = 0.0, 0.0                                                  # row 2: no cell voiced in both (a never is)
    pa[3, 1:], pb[3, 1:] = 0.0, 0.0                                               # row 3: one cell, (0, 0)
    pa[3, 0], pb[3, 0] = 100.0, 131.0
    out['product paths'] = {'period_a': pa, 'period_b': pb, 'path_a': path_a, 'path_b': path_b, 'steps': steps}
    # hand-made: Fa = 5, Fb = 4, P = 8
    pa = np.array([[100, 0, 50, 80, 0]] * 5, dtype=np.float32)
    pb = np.array([[100, 130, 0, 40]] * 5, dtype=np.float32)
    ia = np.array([[0, 1, 2, 3, 4, -1, -1, -1],          # a plain path of 5 cells
                   [0, 1, 5, -1, 3, 1 << 30, 4, 4],      # entries out of range inside steps: skipped
                   [0, 0, 1, 2, 2, 3, 4, 4],             # steps above P: clamped to the 8 entries
                   [0, 1, 2, 3, 4, 4, 4, 4],             # steps negative: nothing
                   [2, 3, 3, 3, 3, 3, 3, 3]], dtype=np.int32)   # steps 2
    ib = np.array([[0, 0, 1, 2, 3, -1, -1, -1],
                   [0, 1, 2, 2, 4, 3, -7, 3],
                   [0, 1, 1, 1, 2, 3, 3, 3],
                   [0, 1, 2, 3, 3, 3, 3, 3],
                   [0, 3, 3, 3, 3, 3, 3, 3]], dtype=np.int32)
    out['hand-made'] = {'period_a': pa, 'period_b': pb, 'path_a': ia, 'path_b': ib,
                        'steps': np.array([5, 8, 1 << 20, -3, 2], dtype=np.int32)}
    return out
