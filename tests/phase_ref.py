"""NumPy restatement of the device phases of taco_griffinlim_rows (include/taco_hip.h): element (b, k, t) of the (B, 1025, F)
phase matrix has index i = (b * 1025 + k) * F + t, h = splitmix64(seed * 0xD1342543DE82EF95 + i) in 64-bit wrap-around
arithmetic, u = h >> 40 (24 bits) and the angle 2 pi u / 2^24.  All integers, so the device and this file agree exactly on u."""
import numpy as np

SEED_MUL = np.uint64(0xD1342543DE82EF95)


def splitmix64(x):
    """the output function of the splitmix64 generator (Steele, Lea, Flood 2014; Vigna's reference code) on uint64 arrays"""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over='ignore'):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def phase_hash(seed, B, F, nbin=1025):
    """h of every element, (B, nbin, F) uint64"""
    i = np.arange(B * nbin * F, dtype=np.uint64).reshape(B, nbin, F)
    with np.errstate(over='ignore'):
        base = np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF) * SEED_MUL
        return splitmix64(base + i)


def phase_u(seed, B, F, nbin=1025):
    """the 24-bit integers u, (B, nbin, F) int64"""
    return (phase_hash(seed, B, F, nbin) >> np.uint64(40)).astype(np.int64)


def phase_angles(seed, B, F, nbin=1025):
    """the angles 2 pi u / 2^24 in fp64"""
    return 2.0 * np.pi * phase_u(seed, B, F, nbin).astype(np.float64) / float(1 << 24)
