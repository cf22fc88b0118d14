"""NumPy restatement of taco_wave_join (include/taco_hip.h) -- TEST INFRASTRUCTURE for the join kernels of csrc/vocoder.hip: the
offsets and totals in Python integers, the edge ramps in fp32 with exactly the entry point's operations (one rounded addition and one
rounded division for the weight, one rounded multiply for the sample), the exact peak, and PCM16 by tests/wave_ref.py's pcm_fp32 with
the prompt's peak.  Samples outside a ramp are copied, so their bits are the input's."""
from __future__ import annotations

import numpy as np

from tests import wave_ref

F32 = np.float32


def piece_lengths(bounds, L):
    """len_i = clamp(bounds[i][1] - bounds[i][0], 0, L)"""
    b = np.asarray(bounds, dtype=np.int64).reshape(-1, 2)
    return [int(min(max(e - s, 0), L)) for s, e in b]


def ramp(f):
    """w(k) = (k + 0.5) / f for k < f, in fp32"""
    k = np.arange(f, dtype=np.int64).astype(F32)
    w = (k + F32(0.5)) / F32(f)
    assert w.dtype == F32
    return w


def faded(x, fade, is_first, is_last):
    """the len(x) samples of one piece with its ramps: f = min(fade, len // 2) samples at the front unless it is the prompt's first
    piece, at the back unless it is the last"""
    x = np.array(x, dtype=F32)
    f = min(int(fade), len(x) // 2)
    if f > 0:
        w = ramp(f)
        if not is_first:
            x[:f] = x[:f] * w
        if not is_last:
            x[len(x) - f:] = x[len(x) - f:] * w[::-1]
    assert x.dtype == F32
    return x


def join(pieces, bounds, first, gap, fade, Lj, L=None):
    """pieces (N, >= L) fp32, bounds (N, 2), first (P + 1), gap (N) -> (out (P, Lj) fp32, pcm (P, Lj) int16, offsets (N) int32,
    total (P) int32, peak (P) fp32)"""
    pieces = np.asarray(pieces, dtype=F32)
    N = pieces.shape[0]
    L = pieces.shape[1] if L is None else int(L)
    P = len(first) - 1
    lens = piece_lengths(bounds, L)
    out = np.zeros((P, Lj), F32)
    pcm = np.zeros((P, Lj), np.int16)
    offsets = np.zeros(N, np.int32)
    total = np.zeros(P, np.int32)
    peak = np.zeros(P, F32)
    for p in range(P):
        lo, hi = int(first[p]), int(first[p + 1])
        o = 0
        for i in range(lo, hi):
            offsets[i] = min(o, Lj)
            v = faded(pieces[i, :lens[i]], fade, i == lo, i == hi - 1)
            keep = min(lens[i], max(0, Lj - o))
            out[p, o:o + keep] = v[:keep]
            if i == hi - 1:
                total[p] = min(Lj, o + lens[i])
            o += lens[i] + int(gap[i])
        t = int(total[p])
        peak[p] = np.max(np.abs(out[p, :t])) if t else 0.0
        pcm[p] = wave_ref.pcm_fp32(out[p], peak[p])
    return out, pcm, offsets, total, peak


# ---- the small case of the GPU tests -----------------------------------------------------------------------------------------------
CORE = dict(N=5, P=3, L=2500, lens=[2500, 0, 7, 1, 1300], first=[0, 3, 3, 5], gap=[100, 0, 5, 33, 9], fade=16, Lj=4001)


def core_pieces(scale=0.3, seed=21, pitch=None, L=CORE['L'], lens=CORE['lens']):
    """(N, pitch) fp32 noise of the given scale with NaN behind every len_i, and bounds (N, 2) with a non-zero trim start (the
    pieces are stored from index 0: only the difference counts)"""
    rng = np.random.default_rng(seed)
    pitch = L if pitch is None else pitch
    x = (scale * rng.standard_normal((len(lens), pitch))).astype(F32)
    for i, n in enumerate(lens):
        x[i, n:] = np.nan
    bounds = np.array([[512 * (i % 3), 512 * (i % 3) + n] for i, n in enumerate(lens)], dtype=np.int32)
    return x, bounds
