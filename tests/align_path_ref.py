"""NumPy restatement of taco_alignment_path (include/taco_hip.h): the best monotone path through one attention matrix, in float32
with plain loops -- one rounded addition per cell, so the device's bits are these bits -- and a brute force over every admissible
path for the small shapes on which the restatement itself is checked."""
import itertools

import numpy as np

F32 = np.float32


def weights(a):
    """w(t, s) = a[t, s] if a[t, s] > 0, else +0 (NaN, negative values and -0 give +0)"""
    a = np.asarray(a, F32)
    with np.errstate(invalid='ignore'):
        return np.where(a > 0, a, F32(0)).astype(F32)


def row_args(Td, Tt, text_length, steps):
    L = min(max(int(text_length), 1), Tt)
    n = Td if steps is None else min(max(int(steps), 0), Td)
    return L, n


def best_path(a, text_length, steps=None, max_jump=4):
    """a (Td, Tt) -> (path (Td,) int32, dur (Tt,) int32, counts (3,) int32 = {n, e, skipped}, mass float32)"""
    a = np.asarray(a, F32)
    Td, Tt = a.shape
    J = int(max_jump)
    assert 1 <= J <= 15
    L, n = row_args(Td, Tt, text_length, steps)
    path = np.full(Td, -1, np.int32)
    dur = np.zeros(Tt, np.int32)
    if n == 0:
        return path, dur, np.zeros(3, np.int32), F32(0)
    w = weights(a)
    Q = np.zeros((n, L), F32)
    D = np.zeros((n, L), np.int32)
    reach = lambda t, s: s <= min(L - 1, J * t)   # noqa: E731
    Q[0, 0] = w[0, 0]
    for t in range(1, n):
        for s in range(L):
            if not reach(t, s):
                continue
            best, bd = None, 0
            for d in range(0, min(J, s) + 1):
                if not reach(t - 1, s - d):
                    continue
                if best is None or Q[t - 1, s - d] > best:   # (strictly larger only: the smallest d wins ties)
                    best, bd = Q[t - 1, s - d], d
            assert best is not None
            Q[t, s] = F32(w[t, s] + best)
            D[t, s] = bd
    e, mass = 0, Q[n - 1, 0]
    for s in range(1, L):
        if reach(n - 1, s) and Q[n - 1, s] > mass:
            e, mass = s, Q[n - 1, s]
    s = e
    for t in range(n - 1, -1, -1):
        path[t] = s
        s -= D[t, s]
    for t in range(n):
        dur[path[t]] += 1
    skipped = int(sum(1 for s in range(e + 1) if dur[s] == 0))
    return path, dur, np.array([n, e, skipped], np.int32), F32(mass)


def best_path_fast(a, text_length, steps=None, max_jump=4):
    """best_path with each step's cells taken together (one NumPy operation per d): the same additions, hence the same bits, for
    the shapes on which the plain loops would take minutes.  tests/test_alignment_path_host.py holds the two together."""
    a = np.asarray(a, F32)
    Td, Tt = a.shape
    J = int(max_jump)
    L, n = row_args(Td, Tt, text_length, steps)
    path = np.full(Td, -1, np.int32)
    dur = np.zeros(Tt, np.int32)
    if n == 0:
        return path, dur, np.zeros(3, np.int32), F32(0)
    w = weights(a[:n, :L])
    D = np.zeros((n, L), np.int8)
    s = np.arange(L)
    q = np.full(J + L, -1, F32)                     # J sentinels in front; unreachable cells hold -1 (every reachable Q is >= 0)
    q[J] = w[0, 0]
    for t in range(1, n):
        cand = np.stack([q[J - d:J - d + L] for d in range(J + 1)])   # cand[d, s] = Q(t-1, s-d)
        D[t] = cand.argmax(0)                       # (the first maximum: the smallest d)
        now = (w[t] + cand.max(0)).astype(F32)
        now[s > min(L - 1, J * t)] = -1
        q[J:] = now
    last = q[J:]
    e = int(last.argmax())
    mass = last[e]
    c = e
    for t in range(n - 1, -1, -1):
        path[t] = c
        c -= int(D[t, c])
    dur[:L] = np.bincount(path[:n], minlength=L)
    skipped = int((dur[:e + 1] == 0).sum())
    return path, dur, np.array([n, e, skipped], np.int32), F32(mass)


def best_paths(al, text_length, steps=None, max_jump=4, one=best_path):
    """the batch: al (B, Td, Tt) -> (path (B, Td), dur (B, Tt), counts (B, 3), mass (B,))"""
    al = np.asarray(al, F32)
    out = [one(al[b], text_length[b], None if steps is None else steps[b], max_jump) for b in range(al.shape[0])]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack([o[2] for o in out]),
            np.array([o[3] for o in out], F32))


def admissible_paths(n, L, J):
    """every path of n steps that starts on character 0, never goes back, advances by at most J and stays below L"""
    for incs in itertools.product(range(J + 1), repeat=n - 1):
        p = np.concatenate([[0], np.cumsum(incs)]).astype(np.int64) if n > 1 else np.zeros(1, np.int64)
        if p[-1] < L:
            yield p


def path_mass(w, p):
    """the mass on path p, added in step order in float32 as the recurrence adds it"""
    m = F32(w[0, p[0]])
    for t in range(1, len(p)):
        m = F32(w[t, p[t]] + m)
    return m


def brute_force(a, text_length, steps=None, max_jump=4):
    """(the largest mass over all admissible paths, the list of paths that attain it) -- None, [] for an empty row"""
    a = np.asarray(a, F32)
    Td, Tt = a.shape
    L, n = row_args(Td, Tt, text_length, steps)
    if n == 0:
        return None, []
    w = weights(a)
    best, arg = None, []
    for p in admissible_paths(n, L, int(max_jump)):
        m = path_mass(w, p)
        if best is None or m > best:
            best, arg = m, [p]
        elif m == best:
            arg.append(p)
    return best, arg
