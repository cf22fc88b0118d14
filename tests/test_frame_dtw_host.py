"""CPU: the host side of the held-out evaluation -- the NumPy restatement of taco_frame_dtw (tests/dtw_ref.py) against a plain
per-cell dynamic programme and on cases whose answer is known, lib.dct_basis / MCD_DB, the --holdout draw of train.py and the
batching of tacotron_amd.evaluate.  No GPU call."""
import math

import numpy as np
import pytest

from tests import dtw_ref as dr


def cells(u, v):
    """the header's recurrence cell by cell in float32, written independently of dtw_ref's anti-diagonal form"""
    f = np.float32
    na, nb = len(u), len(v)
    D = np.zeros((na, nb), dtype=f)
    N = np.zeros((na, nb), dtype=np.int64)
    for i in range(na):
        for j in range(nb):
            s = f(0)
            for k in range(u.shape[1]):
                t = f(u[i, k] - v[j, k])
                s = f(s + f(t * t))
            d = f(np.sqrt(s))
            if i == 0 and j == 0:
                D[i, j], N[i, j] = d, 1
                continue
            cand = [(i - 1, j - 1), (i - 1, j), (i, j - 1)]
            cand = [(p, q) for p, q in cand if p >= 0 and q >= 0]
            best = cand[0]
            for c in cand[1:]:
                if D[c] < D[best]:
                    best = c
            D[i, j], N[i, j] = f(D[best] + d), N[best] + 1
    return D[-1, -1], int(N[-1, -1])


@pytest.mark.parametrize('na,nb,K', [(1, 1, 3), (1, 6, 2), (6, 1, 2), (7, 5, 4), (5, 9, 1), (12, 12, 13)])
def test_the_anti_diagonal_restatement_is_the_per_cell_recurrence(na, nb, K):
    rng = np.random.default_rng(na * 100 + nb)
    for integers in (False, True):   # (integers: many ties)
        a = rng.integers(0, 3, (1, na, K)).astype(np.float32) if integers else rng.standard_normal((1, na, K)).astype(np.float32)
        b = rng.integers(0, 3, (1, nb, K)).astype(np.float32) if integers else rng.standard_normal((1, nb, K)).astype(np.float32)
        cost, steps = dr.dtw32(a, b)
        want = cells(a[0], b[0])
        assert cost.dtype == np.float32 and steps.dtype == np.int32
        assert cost[0].view(np.uint32) == np.float32(want[0]).view(np.uint32) and steps[0] == want[1]
        c64, s64 = dr.dtw64(a, b)
        assert abs(float(cost[0]) - c64[0]) <= 2 * dr.dtw_bound(na + nb - 1, K) * c64[0]


def test_identical_and_doubled_sequences():
    rng = np.random.default_rng(1)
    n = 17
    x = rng.standard_normal((2, n, 6)).astype(np.float32)
    cost, steps = dr.dtw32(x, x)
    assert cost.tolist() == [0.0, 0.0] and steps.tolist() == [n, n]           # the diagonal: first in the order on ties
    twice = np.repeat(x, 2, axis=1)
    cost, steps = dr.dtw32(x, twice)
    assert cost.tolist() == [0.0, 0.0] and steps.tolist() == [2 * n, 2 * n]   # every frame of x meets its two copies
    cost, steps = dr.dtw32(twice, x)
    assert cost.tolist() == [0.0, 0.0] and steps.tolist() == [2 * n, 2 * n]


def test_lengths_clamp_and_empty_rows():
    x = np.arange(24, dtype=np.float32).reshape(2, 4, 3)
    cost, steps = dr.dtw32(x, x, [0, 9], [4, -2])
    assert cost.tolist() == [0.0, 0.0] and steps.tolist() == [0, 0]
    cost, steps = dr.dtw32(x, x, [4, 9], [4, 2])
    assert steps.tolist() == [4, 4]


def test_tie_order_on_integer_frames():
    """All-zero frames: every cell costs 0 and every D ties, so N follows the order of the candidates alone.  a of 2 frames against b
    of 3: (1, 2) takes the diagonal (0, 1), N 2 -> 3 steps; with (i-1, j) first it would come from (0, 2), N 3 -> 4.  Transposed,
    (2, 1) takes the diagonal (1, 0) -> 3 steps; with (i, j-1) first it would come from (2, 0) -> 4."""
    a = np.zeros((1, 2, 1), dtype=np.float32)
    b = np.zeros((1, 3, 1), dtype=np.float32)
    assert dr.dtw32(a, b)[1].tolist() == [3]
    assert dr.dtw32(b, a)[1].tolist() == [3]
    # a = [0, 1, 1] against b = [0, 0, 1], worked by hand as (D, N) with the candidates in the header's order:
    #   row 0: (0, 1) (0, 2) (1, 3)
    #   row 1: (1, 2) (1, 2): (0, 0) ties with (0, 1), the diagonal wins;  (0, 3): from (0, 1)
    #   row 2: (2, 3) (2, 3): (1, 0) ties with (1, 1), the diagonal wins;  (0, 4): from (1, 2), D 0, against (1, 1) D 1 and (2, 1) D 2
    a = np.array([[[0.], [1.], [1.]]], dtype=np.float32)
    b = np.array([[[0.], [0.], [1.]]], dtype=np.float32)
    cost, steps = dr.dtw32(a, b)
    assert cost.tolist() == [0.0] and steps.tolist() == [4]
    assert cells(a[0], b[0]) == (0.0, 4)


def test_frames_active_restatement():
    floor = np.float32(-18.4375)
    x = np.full((5, 6, 3), floor, dtype=np.float32)
    x[1, 5, 2] = -18.0            # only the last frame
    x[2, 0, 0] = 1.0              # only frame 0
    x[3, 2:, :] = np.nan          # NaN frames behind frame 1
    x[3, 1, 1] = 0.0
    x[4, 3, 0] = np.nextafter(floor, np.float32(0))   # one ulp above the floor counts; the floor itself (row 0) does not
    assert dr.frames_active(x, floor).tolist() == [0, 6, 1, 2, 4]


def test_dct_basis_and_mcd_db(built_lib):
    lib = built_lib
    full = lib.dct_basis(80, 0, 80).astype(np.float64)
    assert np.abs(full @ full.T - np.eye(80)).max() < 1e-6
    basis = lib.dct_basis()
    assert basis.shape == (13, 80) and basis.dtype == np.float32
    assert np.array_equal(basis, lib.dct_basis(80, 0, 80)[1:14])
    assert np.abs(basis.astype(np.float64) @ basis.astype(np.float64).T - np.eye(13)).max() < 1e-6
    assert np.abs(basis.astype(np.float64).sum(axis=1)).max() < 1e-5          # no c0: a constant frame has no coefficient
    assert np.allclose(lib.dct_basis(80, 0, 1), np.sqrt(1 / 80))
    c = np.arange(80)
    assert np.allclose(basis[2], np.sqrt(2 / 80) * np.cos(np.pi * (c + 0.5) * 3 / 80), atol=1e-7)
    for bad in ((0, 0, 1), (80, 70, 13), (80, -1, 3), (80, 0, 0)):
        with pytest.raises(ValueError):
            lib.dct_basis(*bad)
    assert lib.MCD_DB == 10.0 * math.sqrt(2.0) / math.log(10.0) and abs(lib.MCD_DB - 6.14185) < 1e-5


def test_wrapper_argument_checks_need_no_gpu(built_lib):
    import torch
    lib = built_lib
    a = torch.zeros(2, 5, 4)
    for bad in (lambda: lib.frame_dtw(a, torch.zeros(2, 5, 3)), lambda: lib.frame_dtw(a, torch.zeros(3, 5, 4)),
                lambda: lib.frame_dtw(a, a, na=torch.zeros(2)), lambda: lib.frame_dtw(a, a, basis=torch.zeros(3, 5)),
                lambda: lib.frame_dtw(a.double(), a), lambda: lib.frame_dtw(torch.zeros(1, 5, 33), torch.zeros(1, 5, 33)),
                lambda: lib.frame_dtw(torch.zeros(1, lib.DTW_MAX_FRAMES + 1, 4), torch.zeros(1, 5, 4)),
                lambda: lib.frame_dtw(a, a, cost=torch.zeros(3)), lambda: lib.frame_dtw(a, a),   # (last: right arguments, no GPU)
                lambda: lib.frames_active(a[0], 0.0), lambda: lib.frames_active(a, float('nan')), lambda: lib.frames_active(a, 0.0)):
        with pytest.raises(ValueError):
            bad()
    assert lib.frame_dtw_workspace_bytes(32, 360, 360, 13) == 0
    assert lib.frame_dtw_workspace_bytes(1, lib.DTW_MAX_FRAMES, lib.DTW_MAX_FRAMES, 13) == 0      # 128 KiB: still LDS
    assert lib.frame_dtw_workspace_bytes(2, lib.DTW_MAX_FRAMES, lib.DTW_MAX_FRAMES, 32) == 2 * 2048 * 33 * 4
    for bad in ((0, 5, 5, 3), (1, 0, 5, 3), (1, 5, lib.DTW_MAX_FRAMES + 1, 3), (1, 5, 5, 33), (1, 5, 5, 0)):
        with pytest.raises(lib.TacoError):
            lib.frame_dtw_workspace_bytes(*bad)


def test_holdout_draw():
    from tacotron_amd.train import holdout_draw
    n, B, seed = 300, 32, 1003
    draw = holdout_draw(n, 40, B, seed)
    seen = np.concatenate([draw(s) for s in range(10000 // B + 1)])
    assert len(seen) >= 10000 and seen.min() == 0 and seen.max() == n - 41      # never one of the last 40; all the others do come
    # N = 0: the values of the draw the feeders make on their own (data.DeviceCorpus / DeviceFeeder: rng.integers(n, size=B))
    own = np.random.default_rng(seed)
    draw0 = holdout_draw(n, 0, B, seed)
    for s in range(5):
        assert np.array_equal(draw0(s), own.integers(n, size=B))
    for bad in (n, n + 1, -1):
        with pytest.raises(ValueError):
            holdout_draw(n, bad, B, seed)


def test_train_without_holdout_keeps_the_feeders_own_draw():
    """--holdout 0 passes no draw at all: DeviceCorpus on the CPU gives the batches it gave before the option existed"""
    import torch
    from tacotron_amd.data import DeviceCorpus
    from tacotron_amd.train import holdout_draw, parse_args
    assert parse_args([]).holdout == 0 and parse_args(['--holdout', '7']).holdout == 7
    data = {'text': torch.arange(50, dtype=torch.int32)[:, None].repeat(1, 2)}
    plain = DeviceCorpus(data, 4, device='cpu', seed=1000)
    held = DeviceCorpus(data, 4, device='cpu', seed=1000, draw=holdout_draw(50, 10, 4, 1000))
    zero = DeviceCorpus(data, 4, device='cpu', seed=1000, draw=holdout_draw(50, 0, 4, 1000))
    for _ in range(50):
        p, h, z = plain.next()['text'], held.next()['text'], zero.next()['text']
        assert torch.equal(p, z) and int(h.max()) < 40


def test_evaluate_batching_pads_and_unpads(built_lib):
    from tacotron_amd.evaluate import holdout_batches, mcd_rows, unpad
    batches = holdout_batches(20, 7, 3)
    assert [(i.tolist(), v) for i, v in batches] == [([13, 14, 15], 3), ([16, 17, 18], 3), ([19, 19, 19], 1)]
    assert all(i.dtype == np.int64 for i, _ in batches)
    assert [(i.tolist(), v) for i, v in holdout_batches(20, 6, 3)] == [([14, 15, 16], 3), ([17, 18, 19], 3)]
    assert [(i.tolist(), v) for i, v in holdout_batches(5, 5, 8)] == [([0, 1, 2, 3, 4, 4, 4, 4], 5)]
    keep = np.arange(20) % 2 == 1
    assert [(i.tolist(), v) for i, v in holdout_batches(20, 7, 3, keep)] == [([13, 15, 17], 3), ([19, 19, 19], 1)]
    assert holdout_batches(20, 1, 3, np.arange(20) < 5) == []
    for bad in (0, 21, -3):
        with pytest.raises(ValueError):
            holdout_batches(20, bad, 3)
    per = [np.array([1., 2., 3.]), np.array([4., 5., 6.]), np.array([7., 7., 7.])]
    assert unpad(batches, per).tolist() == [1., 2., 3., 4., 5., 6., 7.]
    assert unpad(batches, [i for i, _ in batches]).tolist() == [13, 14, 15, 16, 17, 18, 19]
    rows = mcd_rows([3, 4], [10, 0], [12, 5], [14, 0], [7.0, 0.0])
    assert rows.shape == (2, 6) and rows.dtype == np.float64
    assert rows[0].tolist() == [3.0, 10.0, 12.0, 14.0, 7.0, built_lib.MCD_DB * 7.0 / 14.0] and np.isnan(rows[1, 5])
