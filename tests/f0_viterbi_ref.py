"""NumPy float32 restatement of taco_f0_viterbi (include/taco_hip.h): rules 1-7, every arithmetic step one explicit float32 operation
(a subtraction, an absolute value, a product, an addition), so that applied to the float32 acf the device read it gives the device's
period, strength and score bit for bit and its counts exactly.  `paths` is the whole call; `candidates` and `best_path` are its two
halves, stacked over rows of equal length (the per-frame loop of the recurrence is the only Python loop).
Imports without a GPU and without the library; the constants are restated, not imported."""
import numpy as np

MAX_CAND, MAX_LAGS, MAX_FRAMES = 15, 512, 8192
f32 = np.float32
NEG = f32(-np.inf)


def row_frames(frames_b, frames_per_unit, F):
    """F_b: frames[b] * frames_per_unit (Python integers: no overflow) clamped to [0, F]; None: F"""
    if frames_b is None:
        return int(F)
    return min(max(int(frames_b) * int(frames_per_unit), 0), int(F))


def candidates(y, bias, K):
    """Rules 1 and 2.  y (R, L, n) float32 -> (idx (R, K, n) int64: the kept rows in ascending order, -1 where absent;
    v (R, K, n) float32: their local scores, -inf where absent)"""
    y = np.asarray(y)
    assert y.dtype == np.float32 and y.ndim == 3 and y.shape[1] >= 3 and 1 <= K <= MAX_CAND
    R, L, n = y.shape
    ym, y0, yp = y[:, :-2], y[:, 1:-1], y[:, 2:]
    with np.errstate(all='ignore'):
        cand = (y0 > ym) & (y0 >= yp)                                   # (R, L - 2, n); entry j is row j + 1
        v = y0 if bias is None else y0 - np.asarray(bias, dtype=f32)[None, 1:-1, None]   # one float32 subtraction
        assert v.dtype == np.float32
        # the total order: candidates first, larger v first, smaller row on equal v (lexsort is stable: ties keep ascending rows)
        order = np.lexsort((-np.where(cand, v, f32(0.0)), ~cand), axis=1)
    kf = np.minimum(cand.sum(axis=1), K)                                # (R, n)
    top = order[:, :K, :]                                               # (R, <= K, n)
    if top.shape[1] < K:
        top = np.concatenate([top, np.zeros((R, K - top.shape[1], n), dtype=top.dtype)], axis=1)
    present = np.arange(K)[None, :, None] < kf[:, None, :]
    rows = np.sort(np.where(present, top + 1, L), axis=1)               # ascending rows, the absent ones (L) behind them
    idx = np.where(present, rows, -1)                                   # (after the sort `present` is again the first k_f slots)
    vk = np.take_along_axis(v, np.clip(rows - 1, 0, L - 3), axis=1)
    return idx, np.where(present, vk, NEG).astype(f32)


def best_path(idx, v, lg, threshold, jump_cost, switch_cost):
    """Rules 3 to 5 (and the pieces of 6 and 7 that come out of the recurrence).  idx, v (R, K, n) from `candidates`, n >= 1 ->
    (s (R, n) int64: the slot of every frame, score (R) float32, local (R, n) int64: the lowest slot of the largest local score)"""
    R, K, n = v.shape
    lg = np.asarray(lg, dtype=f32)
    thr, jump, sw = f32(threshold), f32(jump_cost), f32(switch_cost)
    vs = np.concatenate([v, np.full((R, 1, n), thr, dtype=f32)], axis=1)           # (R, K + 1, n): slot K scores the threshold
    lgs = np.where(idx >= 0, lg[np.clip(idx, 0, len(lg) - 1)], f32(0.0)).astype(f32)   # (R, K, n)
    local = vs.argmax(axis=1)                                                      # the first of equal maxima: the lowest slot
    voiced = np.arange(K + 1) < K
    both = voiced[:, None] & voiced[None, :]                                       # [p, c]
    one = voiced[:, None] != voiced[None, :]
    fixed = np.where(one, sw, f32(0.0)).astype(f32)                                # switch_cost, or +0 between slot K and itself
    back = np.zeros((R, n, K + 1), dtype=np.int64)
    with np.errstate(all='ignore'):
        E = vs[:, :, 0]
        m = E.max(axis=1)
        score = m.copy()
        D = E - m[:, None]
        for f in range(1, n):
            diff = lgs[:, :, f - 1, None] - lgs[:, None, :, f]                     # (R, p, c): one subtraction
            T = np.broadcast_to(fixed, (R, K + 1, K + 1)).copy()
            T[:, :K, :K] = jump * np.abs(diff)                                     # its absolute value, one product
            assert T.dtype == np.float32
            x = D[:, :, None] - T                                                  # (R, p, c)
            back[:, f] = x.argmax(axis=1)                                          # the lowest p of the largest difference
            E = x.max(axis=1) + vs[:, :, f]
            m = E.max(axis=1)
            D = E - m[:, None]
            score = score + m
        assert D.dtype == np.float32 and score.dtype == np.float32
    s = np.zeros((R, n), dtype=np.int64)
    s[:, n - 1] = D.argmax(axis=1)
    rr = np.arange(R)
    for f in range(n - 1, 0, -1):
        s[:, f - 1] = back[rr, f, s[:, f]]
    return s, score, local


def parabola(ym, y0, yp, lag):
    """the pick's refinement (taco_frames_f0's a, t, d and clamp): -> period float32"""
    with np.errstate(all='ignore'):
        a = ym - yp
        t = y0 + y0
        d = (ym - t) + yp
        delta = np.clip((f32(0.5) * a) / np.where(d == 0, f32(1.0), d), f32(-0.5), f32(0.5))
        delta = np.where(d == 0, f32(0.0), delta)
        return lag.astype(f32) + delta


def paths(acf, frames=None, frames_per_unit=1, bias=None, lg=None, lag_min=40, K=4, threshold=0.3, jump_cost=0.0, switch_cost=0.0):
    """acf (B, L, F) float32 -> (period (B, F) float32, strength (B, F) float32, counts (B, 4) int32, score (B) float32); nothing at
    or behind F_b and nothing of another row is read"""
    acf = np.asarray(acf)
    assert acf.dtype == np.float32 and acf.ndim == 3 and lg is not None
    B, L, F = acf.shape
    period, strength = np.zeros((B, F), dtype=f32), np.zeros((B, F), dtype=f32)
    counts, score = np.zeros((B, 4), dtype=np.int32), np.zeros(B, dtype=f32)
    for b in range(B):
        n = row_frames(None if frames is None else frames[b], frames_per_unit, F)
        if n == 0:
            continue
        y = acf[b:b + 1, :, :n]
        idx, v = candidates(y, bias, K)
        s, sc, local = best_path(idx, v, lg, threshold, jump_cost, switch_cost)
        s, local, idx = s[0], local[0], idx[0]
        on = s < K
        i = np.where(on, idx[np.minimum(s, K - 1), np.arange(n)], 1)
        cols = np.arange(n)
        ym, y0, yp = y[0, i - 1, cols], y[0, i, cols], y[0, i + 1, cols]
        period[b, :n] = np.where(on, parabola(ym, y0, yp, lag_min - 1 + i), f32(0.0))
        strength[b, :n] = np.where(on, y0, f32(0.0))
        off = s == K
        counts[b] = (n, int(on.sum()), int((s != local).sum()), int((off[1:] != off[:-1]).sum()))
        score[b] = sc[0]
    return period, strength, counts, score
