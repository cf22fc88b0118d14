"""NumPy restatements of taco_frame_dtw_path and taco_path_f0_scores (include/taco_hip.h), for the tests only.

`dtw32_path` is tests/dtw_ref.py's float32 walk -- its `coefficients`, the same anti-diagonal recurrence operation by operation, the
same tie order -- keeping what the cost-only form throws away: which predecessor every cell took.  The path is read off that table
backwards from (na - 1, nb - 1).  Its cost and steps must equal dtw_ref.dtw32's bit for bit (tests/test_frame_dtw_path_host.py holds
it to that on every case used), and the device's cost bits, steps and both path arrays are compared with it exactly.
`path_scores` restates taco_path_f0_scores in float64, or in float32 with sequential sums (PATH_SCORES_ATOL).  The counts are exact
in either: the voicing tests are comparisons and the gross test is one rounded float32 product per side, whatever `dtype` is.
Imports without a GPU and without the library."""
import numpy as np

from tests import dtw_ref as dr

F32 = np.float32
DIAG, UP, LEFT = 0, 1, 2        # the predecessor a cell took: (i-1, j-1), (i-1, j), (i, j-1) -- the header's order

# The bound on |device - fp64| over the means of taco_path_f0_scores.  Measured, not guessed: the float32 restatement (sequential
# sums) against the float64 one on exactly the inputs of tests/test_gpu_frame_dtw_path.py (tests/path_cases.score_cases;
# tests/test_frame_dtw_path_host.py repeats the measurement and holds this constant to it).  Largest absolute error over all of
# them: 1.92e-7, on a hand-made row of a few cells (x = log2 pb - log2 pa is the difference of two float32 logarithms near 6 and
# itself below 1.4 in magnitude: the rounding of the two logarithms is the error, not the sum); 8.7e-8 on the product-shaped rows of
# a few hundred cells.  Times 4 for another summation order and the device's logarithm and square root.
MEASURED_FLOAT32_PATH_SCORES_ERROR = 1.92e-7
PATH_SCORES_ATOL = 4.0 * MEASURED_FLOAT32_PATH_SCORES_ERROR


def local_distances(u, v):
    """coefficient rows u (na, K), v (nb, K) float32 -> d (na, nb) float32: step 2 of the header, one rounded operation each"""
    u, v = np.asarray(u, dtype=F32), np.asarray(v, dtype=F32)
    s = np.zeros((len(u), len(v)), dtype=F32)
    for k in range(u.shape[1]):
        t = u[:, k:k + 1] - v[None, :, k]
        s = s + t * t
    d = np.sqrt(s)
    assert d.dtype == F32
    return d


def _walk_path(u, v):
    """dtw_ref._walk in float32 with the direction table -> (cost, steps, way (na, nb) uint8)"""
    na, nb, K = len(u), len(v), u.shape[1]
    inf = F32(np.inf)
    D = [np.full(na, inf, dtype=F32) for _ in range(3)]
    N = [np.zeros(na, dtype=np.int64) for _ in range(3)]
    way = np.zeros((na, nb), dtype=np.uint8)
    for d in range(na + nb - 1):
        i = np.arange(max(0, d - (nb - 1)), min(na - 1, d) + 1)
        j = d - i
        t = u[i] - v[j]
        s = np.zeros(len(i), dtype=F32)
        for k in range(K):
            s = s + t[:, k] * t[:, k]
        dist = np.sqrt(s)
        assert dist.dtype == F32
        cur, p1, p2 = d % 3, (d + 2) % 3, (d + 1) % 3
        if d == 0:
            best, count = dist, np.ones(1, dtype=np.int64)
        else:
            im = np.maximum(i - 1, 0)
            have = (i > 0) & (j > 0)
            pd, pn = np.where(have, D[p2][im], inf), np.where(have, N[p2][im], 0)
            took = np.full(len(i), DIAG, dtype=np.uint8)
            cd, ok = D[p1][im], i > 0
            take = ok & (~have | (cd < pd))
            pd, pn, have, took = np.where(take, cd, pd), np.where(take, N[p1][im], pn), have | ok, np.where(take, UP, took)
            cd, ok = D[p1][i], j > 0
            take = ok & (~have | (cd < pd))
            pd, pn, took = np.where(take, cd, pd), np.where(take, N[p1][i], pn), np.where(take, LEFT, took)
            best, count = pd + dist, pn + 1
            assert best.dtype == F32
            way[i, j] = took
        D[cur][i], N[cur][i] = best, count
    last = (na + nb - 2) % 3
    return D[last][na - 1], int(N[last][na - 1]), way


def backtrack(way, steps):
    """way (na, nb) as _walk_path leaves it -> (i (steps), j (steps)) in chronological order"""
    na, nb = way.shape
    pi, pj = np.empty(steps, dtype=np.int32), np.empty(steps, dtype=np.int32)
    i, j = na - 1, nb - 1
    for t in range(steps - 1, -1, -1):
        pi[t], pj[t] = i, j
        if t == 0:
            break
        w = way[i, j]
        i, j = i - (w != LEFT), j - (w != UP)
    assert (i, j) == (0, 0), 'the path of %d cells ends at (%d, %d)' % (steps, i, j)
    return pi, pj


def dtw32_path(a, b, na=None, nb=None, basis=None):
    """-> (cost (B) float32, steps (B) int32, path_a (B, P) int32, path_b (B, P) int32), P = Fa + Fb - 1: the device's bits.  Entries
    t >= steps are -1"""
    a, b = np.asarray(a, dtype=F32), np.asarray(b, dtype=F32)
    B, P = a.shape[0], a.shape[1] + b.shape[1] - 1
    cost, steps = np.zeros(B, dtype=F32), np.zeros(B, dtype=np.int32)
    path_a, path_b = np.full((B, P), -1, dtype=np.int32), np.full((B, P), -1, dtype=np.int32)
    for r, (u, v) in enumerate(dr._rows(a, b, na, nb, basis)):
        if len(u) == 0 or len(v) == 0:
            continue
        cost[r], n, way = _walk_path(u, v)
        steps[r] = n
        path_a[r, :n], path_b[r, :n] = backtrack(way, n)
    return cost, steps, path_a, path_b


def path_cost(a_row, b_row, basis, pi, pj):
    """the float32 local distances of the cells (pi[t], pj[t]) summed in order: what the recurrence added up along its own path"""
    u, v = dr.coefficients(a_row, basis), dr.coefficients(b_row, basis)
    t = u[pi] - v[pj]
    s = np.zeros(len(pi), dtype=F32)
    for k in range(u.shape[1]):
        s = s + t[:, k] * t[:, k]
    d = np.sqrt(s)
    total = d[0]
    for x in d[1:]:
        total = F32(total + x)
    return F32(total)


def path_scores(period_a, period_b, path_a, path_b, steps, gross=1.2, dtype=np.float64):
    """-> (counts (B, 5) int32, means (B, 2) in `dtype`) as the header defines them; float32: sequential sums over the cells in
    path order"""
    period_a, period_b = np.asarray(period_a), np.asarray(period_b)
    assert period_a.dtype == F32 and period_b.dtype == F32
    path_a, path_b = np.asarray(path_a, dtype=np.int64), np.asarray(path_b, dtype=np.int64)
    B, Fa = period_a.shape
    Fb = period_b.shape[1]
    P = Fa + Fb - 1
    assert path_a.shape == (B, P) and path_b.shape == (B, P)
    g = F32(gross)
    counts, means = np.zeros((B, 5), dtype=np.int32), np.zeros((B, 2), dtype=dtype)
    for r in range(B):
        n = min(max(int(steps[r]), 0), P)
        i, j = path_a[r, :n], path_b[r, :n]
        ok = (i >= 0) & (i < Fa) & (j >= 0) & (j < Fb)
        pa, pb = period_a[r, i[ok]], period_b[r, j[ok]]
        with np.errstate(invalid='ignore'):
            va, vb = pa > 0, pb > 0
            both = va & vb
            ga, gb = g * pa, g * pb                     # float32 products, rounded once
            assert ga.dtype == F32
            far = both & ((pa > gb) | (pb > ga))
        counts[r] = [ok.sum(), both.sum(), (va & ~vb).sum(), (vb & ~va).sum(), far.sum()]
        m = int(both.sum())
        if m == 0:
            continue
        x = np.log2(pb[both].astype(dtype)) - np.log2(pa[both].astype(dtype))
        sq = x * x
        if dtype == np.float32:
            assert x.dtype == F32
            s1, s2 = np.cumsum(x, dtype=F32)[-1], np.cumsum(sq, dtype=F32)[-1]
        else:
            s1, s2 = x.sum(), sq.sum()
        means[r] = dtype(s1 / dtype(m)), np.sqrt(dtype(s2 / dtype(m)))
    return counts, means
