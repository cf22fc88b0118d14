"""CPU: the restatements of taco_frame_dtw_path and taco_path_f0_scores (tests/path_ref.py) on hand-worked paths and on every input
of tests/test_gpu_frame_dtw_path.py (tests/path_cases.py), the measurement behind path_ref.PATH_SCORES_ATOL, the signatures the
Python layer declares and its argument checks.  No GPU call."""
import ctypes as C

import numpy as np
import pytest

from tests import dtw_ref as dr
from tests import path_cases as pc
from tests import path_ref as pr


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def path_of(got, row=0):
    cost, steps, pa, pb = got
    n = int(steps[row])
    assert (pa[row, n:] == -1).all() and (pb[row, n:] == -1).all()
    return list(zip(pa[row, :n].tolist(), pb[row, :n].tolist()))


# ---- hand-worked paths -----------------------------------------------------------------------------------------------------------------
def test_tie_orders_by_hand():
    """All-zero frames: every D ties and the order of the candidates alone decides (tests/test_frame_dtw_host.py works the counts).
    2 x 3: (1, 2) takes the diagonal (0, 1), and (0, 1) has only (0, 0) to come from.  3 x 2: (2, 1) takes the diagonal (1, 0)."""
    a = np.zeros((1, 2, 1), dtype=np.float32)
    b = np.zeros((1, 3, 1), dtype=np.float32)
    assert path_of(pr.dtw32_path(a, b)) == [(0, 0), (0, 1), (1, 2)]
    assert path_of(pr.dtw32_path(b, a)) == [(0, 0), (1, 0), (2, 1)]
    # a = [0, 1, 1] against b = [0, 0, 1] (worked there as (D, N)): (2, 2) from (1, 2), that from (0, 1), that from (0, 0)
    a = np.array([[[0.], [1.], [1.]]], dtype=np.float32)
    b = np.array([[[0.], [0.], [1.]]], dtype=np.float32)
    got = pr.dtw32_path(a, b)
    assert got[0].tolist() == [0.0] and path_of(got) == [(0, 0), (0, 1), (1, 2), (2, 2)]
    both = pr.dtw32_path(np.zeros((2, 3, 1), dtype=np.float32), np.zeros((2, 3, 1), dtype=np.float32), [2, 3], [3, 2])
    assert path_of(both, 0) == [(0, 0), (0, 1), (1, 2)] and path_of(both, 1) == [(0, 0), (1, 0), (2, 1)]
    assert both[2].shape == (2, 5) and both[2].dtype == np.int32 and both[3].dtype == np.int32


def test_a_sequence_against_its_repetition():
    rng = np.random.default_rng(1)
    n = 17
    x = rng.standard_normal((2, n, 6)).astype(np.float32)
    twice = np.repeat(x, 2, axis=1)
    cost, steps, pa, pb = pr.dtw32_path(x, twice)
    assert cost.tolist() == [0.0, 0.0] and steps.tolist() == [2 * n, 2 * n]
    t = np.arange(2 * n)
    for r in range(2):
        assert np.array_equal(pa[r, :2 * n], t // 2) and np.array_equal(pb[r, :2 * n], t)      # i_t = t // 2
        assert (pa[r, 2 * n:] == -1).all() and pa.shape[1] == 3 * n - 1
    cost, steps, pa, pb = pr.dtw32_path(twice, x)
    assert np.array_equal(pa[0, :2 * n], t) and np.array_equal(pb[0, :2 * n], t // 2)
    cost, steps, pa, pb = pr.dtw32_path(x, x)
    assert np.array_equal(pa[0, :n], np.arange(n)) and np.array_equal(pb[0, :n], np.arange(n)) and steps.tolist() == [n, n]


def test_empty_rows_and_single_lines():
    x = np.arange(24, dtype=np.float32).reshape(2, 4, 3)
    cost, steps, pa, pb = pr.dtw32_path(x, x, [0, 9], [4, -2])
    assert steps.tolist() == [0, 0] and (pa == -1).all() and (pb == -1).all()
    got = pr.dtw32_path(x, x, [1, 4], [4, 1])
    assert path_of(got, 0) == [(0, 0), (0, 1), (0, 2), (0, 3)] and path_of(got, 1) == [(0, 0), (1, 0), (2, 0), (3, 0)]


# ---- every case of the GPU test ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(pc.dtw_cases()))
def test_paths_of_the_gpu_cases(name):
    """monotone from (0, 0) to (na - 1, nb - 1) in `steps` cells; cost and steps are dtw_ref.dtw32's; the local distances re-summed
    along the path in order give the cost's bits"""
    c = pc.dtw_cases()[name]
    cost, steps, pa, pb = pc.dtw_ref(name)
    c32, s32 = dr.dtw32(c['a'], c['b'], c['na'], c['nb'], c['basis'])
    assert np.array_equal(bits(cost), bits(c32)) and np.array_equal(steps, s32)
    B, Fa, Fb = c['a'].shape[0], c['a'].shape[1], c['b'].shape[1]
    assert pa.shape == (B, Fa + Fb - 1) and pb.shape == pa.shape
    na = np.clip(np.full(B, Fa) if c['na'] is None else np.asarray(c['na']), 0, Fa)
    nb = np.clip(np.full(B, Fb) if c['nb'] is None else np.asarray(c['nb']), 0, Fb)
    for r in range(B):
        n = int(steps[r])
        assert (pa[r, n:] == -1).all() and (pb[r, n:] == -1).all()
        if na[r] == 0 or nb[r] == 0:
            assert n == 0
            continue
        i, j = pa[r, :n].astype(np.int64), pb[r, :n].astype(np.int64)
        assert (i[0], j[0]) == (0, 0) and (i[-1], j[-1]) == (na[r] - 1, nb[r] - 1)
        di, dj = np.diff(i), np.diff(j)
        assert ((di == 0) | (di == 1)).all() and ((dj == 0) | (dj == 1)).all() and (di + dj >= 1).all()
        assert max(na[r], nb[r]) <= n <= na[r] + nb[r] - 1
        again = pr.path_cost(c['a'][r, :na[r]], c['b'][r, :nb[r]], c['basis'], i, j)
        assert bits(again) == bits(cost[r]), (name, r, again, cost[r])
    if name == 'envelope':
        assert Fa + Fb - 1 == 2047 and 1024 <= steps[0] <= 2047


def test_the_cases_are_the_cost_only_tests_cases(built_lib):
    assert np.array_equal(pc.dct_basis(), built_lib.dct_basis())
    assert pc.THREADS == 256 and built_lib.DTW_MAX_FRAMES == 1024 == pc.dtw_cases()['envelope']['a'].shape[1]


# ---- path_scores ------------------------------------------------------------------------------------------------------------------------
def test_path_scores_by_hand():
    s = pc.score_cases()['hand-made']
    counts, means = pr.path_scores(s['period_a'], s['period_b'], s['path_a'], s['path_b'], s['steps'], pc.GROSS)
    # row 0: cells (0,0) (1,0) (2,1) (3,2) (4,3) -> periods (100,100) (0,100) (50,130) (80,0) (0,40)
    #        both: (100,100) x = 0; (50,130) x = log2 2.6, gross (130 > 60).  a only: (80,0).  b only: (0,100), (0,40)
    x = np.log2(2.6)
    assert counts[0].tolist() == [5, 2, 1, 2, 1]
    assert abs(means[0, 0] - x / 2) < 1e-12 and abs(means[0, 1] - np.sqrt(x * x / 2)) < 1e-12
    # row 1: entries 2, 3, 4, 5, 6 are out of range and skipped; left: (0,0) (1,1) (4,3) -> (100,100) (0,130) (0,40)
    assert counts[1].tolist() == [3, 1, 0, 2, 0] and means[1].tolist() == [0.0, 0.0]
    # row 2: steps clamped to 8: (0,0) (0,1) (1,1) (2,1) (2,2) (3,3) (4,3) (4,3)
    #        -> (100,100) (100,130) (0,130) (50,130) (50,0) (80,40) (0,40) (0,40); gross: 100/130 (1.3), 50/130, 80/40
    xs = np.array([0.0, np.log2(1.3), np.log2(2.6), -1.0])
    assert counts[2].tolist() == [8, 4, 1, 3, 3]
    assert abs(means[2, 0] - xs.mean()) < 1e-12 and abs(means[2, 1] - np.sqrt((xs * xs).mean())) < 1e-12
    assert counts[3].tolist() == [0, 0, 0, 0, 0] and means[3].tolist() == [0.0, 0.0]          # steps < 0
    # row 4: (2,0) (3,3) -> (50,100) x = 1, gross; (80,40) x = -1, gross
    assert counts[4].tolist() == [2, 2, 0, 0, 2] and abs(means[4, 0]) < 1e-12 and abs(means[4, 1] - 1.0) < 1e-12
    assert counts.dtype == np.int32 and means.dtype == np.float64


def test_product_rows_have_none_one_and_all_voiced():
    s = pc.score_cases()['product paths']
    counts, _ = pr.path_scores(s['period_a'], s['period_b'], s['path_a'], s['path_b'], s['steps'], pc.GROSS)
    assert np.array_equal(counts[:, 0], s['steps'])
    assert 0 < counts[0, 1] < counts[0, 0] and counts[0, 2] > 0 and counts[0, 3] > 0 and 0 < counts[0, 4] < counts[0, 1]
    assert counts[1, 1] == counts[1, 0] and counts[2, 1] == 0 and counts[2, 2] == 0 and counts[3, 1] == 1 and counts[3, 4] == 1


def test_no_cell_sits_on_the_gross_threshold():
    for name, s in pc.score_cases().items():
        Fa, Fb = s['period_a'].shape[1], s['period_b'].shape[1]
        for r in range(len(s['steps'])):
            n = min(max(int(s['steps'][r]), 0), Fa + Fb - 1)
            i, j = s['path_a'][r, :n].astype(np.int64), s['path_b'][r, :n].astype(np.int64)
            ok = (i >= 0) & (i < Fa) & (j >= 0) & (j < Fb)
            pa, pb = s['period_a'][r, i[ok]].astype(np.float64), s['period_b'][r, j[ok]].astype(np.float64)
            both = (pa > 0) & (pb > 0)
            pa, pb = pa[both], pb[both]
            assert (np.abs(pa / (pc.GROSS * pb) - 1.0) > 1e-3).all() and (np.abs(pb / (pc.GROSS * pa) - 1.0) > 1e-3).all(), (name, r)


def test_the_tolerance_is_four_times_the_measured_float32_error():
    worst = 0.0
    for name, s in pc.score_cases().items():
        args = (s['period_a'], s['period_b'], s['path_a'], s['path_b'], s['steps'], pc.GROSS)
        c64, m64 = pr.path_scores(*args)
        c32, m32 = pr.path_scores(*args, dtype=np.float32)
        assert m32.dtype == np.float32 and np.array_equal(c32, c64)
        err = float(np.abs(m32.astype(np.float64) - m64).max())
        print('  %-14s float32 against float64: %.3e' % (name, err))
        worst = max(worst, err)
    print('  worst %.3e, MEASURED_FLOAT32_PATH_SCORES_ERROR %.3e' % (worst, pr.MEASURED_FLOAT32_PATH_SCORES_ERROR))
    assert worst <= pr.MEASURED_FLOAT32_PATH_SCORES_ERROR <= 1.05 * worst          # the constant IS the measurement
    assert pr.PATH_SCORES_ATOL == 4.0 * pr.MEASURED_FLOAT32_PATH_SCORES_ERROR


# ---- the Python layer --------------------------------------------------------------------------------------------------------------------
def test_exports(built_lib):
    lib = built_lib
    P, I = C.c_void_p, C.c_int
    assert lib.EXPORTS['taco_frame_dtw_path_workspace_bytes'] == (C.c_int64, [I, I, I, I])
    assert lib.EXPORTS['taco_frame_dtw_path'] == (I, [P] * 10 + [I] * 5 + [P])
    assert lib.EXPORTS['taco_path_f0_scores'] == (I, [P] * 5 + [C.c_float] + [P] * 2 + [I] * 3 + [P])
    for name in ('taco_frame_dtw_path_workspace_bytes', 'taco_frame_dtw_path', 'taco_path_f0_scores'):
        assert getattr(lib._lib, name).argtypes == lib.EXPORTS[name][1]
    header = open(lib.os.path.join(lib.os.path.dirname(lib.os.path.dirname(lib.__file__)), 'include', 'taco_hip.h')).read()
    assert 'int taco_frame_dtw_path(' in header and 'int taco_path_f0_scores(' in header and 'NOT provided: the warping path' not in header


def test_workspace_bytes(built_lib):
    lib = built_lib
    assert lib.frame_dtw_path_workspace_bytes(1, 1, 1, 1) == 1                              # never 0 for an accepted shape
    assert lib.frame_dtw_path_workspace_bytes(32, 360, 360, 13) == 32 * 719 * 360           # the table alone: a byte per cell and diagonal
    M = lib.DTW_MAX_FRAMES
    assert lib.frame_dtw_path_workspace_bytes(2, M, M, 32) == lib.frame_dtw_workspace_bytes(2, M, M, 32) + 2 * (2 * M - 1) * M
    for bad in ((0, 5, 5, 3), (1, 0, 5, 3), (1, 5, M + 1, 3), (1, 5, 5, 33), (1, 5, 5, 0)):   # what frame_dtw_workspace_bytes refuses
        with pytest.raises(lib.TacoError):
            lib.frame_dtw_path_workspace_bytes(*bad)


def test_wrapper_argument_checks_need_no_gpu(built_lib):
    import torch
    lib = built_lib
    a = torch.zeros(2, 5, 4)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)   # noqa: E731
    for bad in (lambda: lib.frame_dtw_path(a, torch.zeros(2, 5, 3)), lambda: lib.frame_dtw_path(a, torch.zeros(3, 5, 4)),
                lambda: lib.frame_dtw_path(a, a, na=torch.zeros(2)), lambda: lib.frame_dtw_path(a, a, basis=torch.zeros(3, 5)),
                lambda: lib.frame_dtw_path(a.double(), a), lambda: lib.frame_dtw_path(torch.zeros(1, 5, 33), torch.zeros(1, 5, 33)),
                lambda: lib.frame_dtw_path(torch.zeros(1, lib.DTW_MAX_FRAMES + 1, 4), torch.zeros(1, 5, 4)),
                lambda: lib.frame_dtw_path(a, a, cost=torch.zeros(3)), lambda: lib.frame_dtw_path(a, a, path_a=i32(2, 8)),
                lambda: lib.frame_dtw_path(a, a, path_b=torch.zeros(2, 9)),
                lambda: lib.frame_dtw_path(a, a)):                                          # (last: right arguments, no GPU)
        with pytest.raises(ValueError):
            bad()
    pa, pb = torch.zeros(2, 5), torch.zeros(2, 4)
    good = dict(period_a=pa, period_b=pb, path_a=i32(2, 8), path_b=i32(2, 8), steps=i32(2))
    for change in (dict(period_a=pa.double()), dict(period_a=pa[0]), dict(period_b=torch.zeros(3, 4)), dict(period_b=pb.double()),
                   dict(period_a=torch.zeros(2, lib.DTW_MAX_FRAMES + 1), path_a=i32(2, lib.DTW_MAX_FRAMES + 4), path_b=i32(2, lib.DTW_MAX_FRAMES + 4)),
                   dict(path_a=i32(2, 9)), dict(path_b=torch.zeros(2, 8)), dict(steps=i32(3)), dict(steps=None), dict(gross=1.0),
                   dict(gross=0.5), dict(gross=float('nan')), dict(gross=1.0 + 1e-9), dict(counts=i32(2, 4)), dict(means=torch.zeros(2, 3)),
                   dict()):                                                                 # (last: right arguments, no GPU)
        with pytest.raises(ValueError):
            lib.path_f0_scores(**dict(good, **change))
    assert lib.PATH_SCORE_COUNTS == ('cells', 'both_voiced', 'a_only', 'b_only', 'gross')


def test_aligned_columns():
    from tacotron_amd import evaluate as ev
    assert ev.ALIGNED_COLUMNS == ('path_voiced', 'f0_rmse_cents', 'f0_bias_cents', 'vuv_error', 'gross_error')
    cols = ev.aligned_columns([[10, 4, 1, 2, 1], [6, 0, 3, 3, 0], [0, 0, 0, 0, 0]], [[0.1, 0.2], [0, 0], [0, 0]])
    assert cols.shape == (3, 5) and cols.dtype == np.float64
    assert np.allclose(cols[0], [4, 240.0, 120.0, 0.3, 0.25]) and cols[1, 0] == 0 and cols[1, 3] == 1.0
    assert np.isnan(cols[1, [1, 2, 4]]).all() and np.isnan(cols[2, 1:]).all()
    assert np.allclose(ev.aligned_summary(cols), (240.0, 0.65, 0.25)) and all(np.isnan(x) for x in ev.aligned_summary(cols[2:]))
    a = ev.parse_args(['--f0-aligned'])
    assert a.f0_aligned and not a.f0 and not ev.parse_args(['--f0']).f0_aligned
