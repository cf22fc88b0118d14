"""NumPy restatement of taco_tensor_stats (include/taco_hip.h), for tests only: the bucket rule from the float's bits, a second
formulation of it through np.frexp to check the first against, counts and extremes from masks, the sums in fp64 by math.fsum as the
"true" value, and the bounds any fp64 summation order stays inside."""
import math

import numpy as np

COUNTS = ('size', 'finite', 'nan', 'pinf', 'ninf', 'zeros')
MOMENTS = ('sum', 'sumsq', 'min', 'max', 'absmax')


def n_bins(e_lo, e_hi, s):
    return 2 * ((e_hi - e_lo + 1) << s) + 1


def bucket_bits(x, e_lo, e_hi, s):
    """Bin of every element of the fp32 array x by the header's integer rule (only meaningful for the finite ones)."""
    bits = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.int64)
    u = bits & 0x7fffffff
    k = u >> (23 - s)
    lo, hi = (127 + e_lo) << s, ((127 + e_hi + 1) << s) - 1
    m = np.where(k < lo, 0, np.minimum(k, hi) - lo + 1)
    nm = (e_hi - e_lo + 1) << s
    return nm + np.where(bits >> 31 != 0, -m, m)


def bucket_frexp(x, e_lo, e_hi, s):
    """The same bins from the value: |x| = f 2^e with f in [0.5, 1) (np.frexp); octave e - 1, sub-bucket floor((2 f - 1) 2^s)."""
    x = np.ascontiguousarray(x, np.float32).astype(np.float64)
    a = np.abs(x)
    f, e = np.frexp(a)
    octave = e.astype(np.int64) - 1
    sub = np.floor((2.0 * f - 1.0) * (1 << s)).astype(np.int64)
    m = ((octave - e_lo) << s) + sub + 1
    nm = (e_hi - e_lo + 1) << s
    m = np.where(a < math.ldexp(1.0, e_lo), 0, np.minimum(m, nm))
    return nm + np.where(np.signbit(x), -m, m)


def _ordered_key(v):
    """finite fp32 values as integers in their order, -0 below +0"""
    bits = v.view(np.uint32).astype(np.int64)
    return np.where(bits >> 31 != 0, -(bits & 0x7fffffff) - 1, bits)


def stats(x, e_lo=-24, e_hi=15, s=2):
    """(counts (6) int64, moments (5) float64, hist (NB) int64) of one segment, the sums by math.fsum."""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    nan, pinf, ninf = np.isnan(x), x == np.inf, x == -np.inf
    fin = ~(nan | pinf | ninf)
    v = x[fin]
    counts = np.array([x.size, v.size, nan.sum(), pinf.sum(), ninf.sum(), (x == 0).sum()], dtype=np.int64)
    v64 = v.astype(np.float64)
    if v.size:
        key = _ordered_key(v)
        moments = np.array([math.fsum(v64), math.fsum(v64 * v64), v[np.argmin(key)], v[np.argmax(key)], np.abs(v).max()], dtype=np.float64)
    else:
        moments = np.array([0.0, 0.0, np.inf, -np.inf, 0.0])
    hist = np.bincount(bucket_bits(v, e_lo, e_hi, s), minlength=n_bins(e_lo, e_hi, s)).astype(np.int64)
    return counts, moments, hist


def sum_bounds(x):
    """(bound on |sum - fsum|, bound on |sumsq - fsum(x^2)|) for fp64 summation of the finite elements in ANY order: each of the
    size - 1 additions rounds a partial sum no larger than sum |x| by at most 2^-53 of it (the squares themselves are exact)."""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    v = x[np.isfinite(x)].astype(np.float64)
    return x.size * 2.0 ** -53 * math.fsum(np.abs(v)), x.size * 2.0 ** -53 * math.fsum(v * v)


def stats_many(base, segments, e_lo=-24, e_hi=15, s=2):
    """stats of every (offset, size) segment of the flat fp32 array base, stacked: counts (n, 6), moments (n, 5), hist (n, NB)."""
    rows = [stats(base[o:o + n], e_lo, e_hi, s) for o, n in segments]
    return tuple(np.stack([r[i] for r in rows]) for i in range(3))


def edge_values(e_lo, e_hi, s):
    """The lower edges of the positive buckets m = 1 .. Nm as fp32, straight from the rule: bits (lo + m - 1) << (23 - s)."""
    lo, nm = (127 + e_lo) << s, (e_hi - e_lo + 1) << s
    return ((np.arange(nm, dtype=np.int64) + lo) << (23 - s)).astype(np.uint32).view(np.float32)


def prev_toward_zero(v):
    """The fp32 value one step closer to 0 (of a non-zero finite value)"""
    return (np.ascontiguousarray(v, np.float32).view(np.uint32) - np.uint32(1)).view(np.float32)
