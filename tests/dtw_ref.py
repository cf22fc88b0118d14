"""NumPy restatements of taco_frames_active and taco_frame_dtw (include/taco_hip.h), for the tests only.

`dtw32` restates sections 1-4 of the header operation by operation in float32 -- NumPy rounds every elementwise product, sum and
difference of float32 arrays to float32 and fuses nothing, np.sqrt is correctly rounded -- so the device's cost BITS and steps are
compared with it exactly.  It is vectorised by anti-diagonal, as the kernel is (per-cell Python loops at 1024 x 1024 would take
minutes).  `dtw64` runs the same recurrence in float64 over the SAME float32 coefficients: the yardstick of `dtw_bound`.

dtw_bound(steps_max, K) = (steps_max + K / 2 + 3) 2^-24, relative to the float64 cost.  Why: fp32 addition is monotone, so the fp32
recurrence is the minimum over paths of the fp32-evaluated path sums, and the difference of two minima is at most the worst
single-path error.  One path: a local distance carries 2^-24 from the subtraction (doubled by the square, halved by the root), 2^-24
from each square and at most K - 1 from the sum of K positive terms (halved by the root), 2^-24 from the root: K / 2 + 3 at the
most; the n <= steps_max terms of a path add n - 1 more roundings.  Tests allow twice the bound, as align_ref.means_bound's do."""
import numpy as np

F32 = np.float32
_INF32 = np.float32(np.inf)


def coefficients(x, basis):
    """x (F, C) float32, basis (K, C) float32 or None -> (F, K) float32: acc = +0, then acc = acc + (basis[k, c] * x[i, c]), c ascending"""
    x = np.ascontiguousarray(x, dtype=F32)
    if basis is None:
        return x.copy()
    basis = np.ascontiguousarray(basis, dtype=F32)
    acc = np.zeros((x.shape[0], basis.shape[0]), dtype=F32)
    for c in range(x.shape[1]):
        acc = acc + x[:, c:c + 1] * basis[None, :, c]
    assert acc.dtype == F32
    return acc


def _walk(u, v, dtype):
    """the recurrence over coefficient rows u (na, K), v (nb, K) in `dtype` arithmetic -> (cost, steps)"""
    na, nb, K = len(u), len(v), u.shape[1]
    if na == 0 or nb == 0:
        return dtype(0), 0
    u, v = u.astype(dtype), v.astype(dtype)
    inf = dtype(np.inf)
    D = [np.full(na, inf, dtype=dtype) for _ in range(3)]
    N = [np.zeros(na, dtype=np.int64) for _ in range(3)]
    for d in range(na + nb - 1):
        i = np.arange(max(0, d - (nb - 1)), min(na - 1, d) + 1)
        j = d - i
        t = u[i] - v[j]
        s = np.zeros(len(i), dtype=dtype)
        for k in range(K):
            s = s + t[:, k] * t[:, k]
        dist = np.sqrt(s)
        assert dist.dtype == dtype
        cur, p1, p2 = d % 3, (d + 2) % 3, (d + 1) % 3
        if d == 0:
            best, count = dist, np.ones(1, dtype=np.int64)
        else:
            im = np.maximum(i - 1, 0)
            # candidates in the order (i-1, j-1), (i-1, j), (i, j-1); a later one wins only when strictly smaller.  A candidate
            # outside the table is +inf and count 0: it never wins against a finite one, and every cell but (0, 0) has one
            pd = np.where((i > 0) & (j > 0), D[p2][im], inf)
            pn = np.where((i > 0) & (j > 0), N[p2][im], 0)
            have = (i > 0) & (j > 0)
            cd, ok = D[p1][im], i > 0
            take = ok & (~have | (cd < pd))
            pd, pn, have = np.where(take, cd, pd), np.where(take, N[p1][im], pn), have | ok
            cd, ok = D[p1][i], j > 0
            take = ok & (~have | (cd < pd))
            pd, pn = np.where(take, cd, pd), np.where(take, N[p1][i], pn)
            best, count = pd + dist, pn + 1
            assert best.dtype == dtype
        D[cur][i], N[cur][i] = best, count
    last = (na + nb - 2) % 3
    return D[last][na - 1], int(N[last][na - 1])


def _rows(a, b, na, nb, basis):
    a, b = np.asarray(a, dtype=F32), np.asarray(b, dtype=F32)
    B, Fa, Fb = a.shape[0], a.shape[1], b.shape[1]
    na = np.full(B, Fa) if na is None else np.clip(np.asarray(na, dtype=np.int64), 0, Fa)
    nb = np.full(B, Fb) if nb is None else np.clip(np.asarray(nb, dtype=np.int64), 0, Fb)
    for r in range(B):
        yield coefficients(a[r, :na[r]], basis), coefficients(b[r, :nb[r]], basis)


def dtw32(a, b, na=None, nb=None, basis=None):
    """-> (cost (B) float32, steps (B) int32): the device's bits"""
    out = [_walk(u, v, F32) for u, v in _rows(a, b, na, nb, basis)]
    return np.array([c for c, _ in out], dtype=F32), np.array([n for _, n in out], dtype=np.int32)


def dtw64(a, b, na=None, nb=None, basis=None):
    """-> (cost (B) float64, steps (B)): float64 recurrence over the float32 coefficients"""
    out = [_walk(u, v, np.float64) for u, v in _rows(a, b, na, nb, basis)]
    return np.array([c for c, _ in out], dtype=np.float64), np.array([n for _, n in out], dtype=np.int64)


def dtw_bound(steps_max, K):
    return (steps_max + K / 2.0 + 3.0) * 2.0 ** -24


def frames_active(x, floor):
    """x (B, F, C) -> (B) int32: 1 + the last frame with an element > floor (a NaN is not), 0 when there is none"""
    x = np.asarray(x, dtype=F32)
    with np.errstate(invalid='ignore'):
        hit = (x > F32(floor)).any(axis=2)
    last = np.where(hit.any(axis=1), x.shape[1] - np.argmax(hit[:, ::-1], axis=1), 0)
    return last.astype(np.int32)
