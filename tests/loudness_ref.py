"""fp64 NumPy restatement of taco_wave_loudness (include/taco_hip.h) -- TEST INFRASTRUCTURE for csrc/loudness.hip: the K-weighting
from its closed forms, hop sums and 400 ms blocks (one block for a row shorter than 400 ms), the two gates in the power domain and
each block's distance from them, the readings, the gain under a sample-peak ceiling, and step 5's PCM16 in NumPy fp32."""
from __future__ import annotations

import math

import numpy as np
from scipy.signal import lfilter

TABLE_48K = (1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
             1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621)
Z_ABS = float(np.float32(10.0 ** ((-70.0 + 0.691) / 10.0)))   # the fp32 value, widened: the device's gate


def k_weighting(sr):
    """b0 b1 b2 a1 a2 of the shelf, then of the high-pass, in fp64"""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / sr)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    shelf = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0,
             2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / sr)
    d = 1.0 + K / Q + K * K
    return shelf + [1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / d, (1.0 - K / Q + K * K) / d]


def device_coefficients(sr):
    """the values the device filters with: rounded once to fp32, widened"""
    return [float(np.float32(c)) for c in k_weighting(sr)]


def k_filter(x, sr):
    """step 1 in fp64, with the device's coefficients, from a zero state"""
    c = device_coefficients(sr)
    x = np.asarray(x, dtype=np.float64)
    if x.size == 0:
        return x.copy()
    u = lfilter(c[0:3], [1.0, c[3], c[4]], x)
    return lfilter(c[5:8], [1.0, c[8], c[9]], u)


def lufs(z):
    return -0.691 + 10.0 * math.log10(z) if z > 0 else -math.inf


def block_powers(y, sr):
    """step 2: z (nb) for the n = len(y) K-weighted samples of a row"""
    n, H = len(y), sr // 10
    if n == 0:
        return np.zeros(0)
    nh = n // H
    if nh < 4:
        return np.array([np.sum(y * y) / n])
    h = np.sum((y[:nh * H] ** 2).reshape(nh, H), axis=1)
    return (h[:-3] + h[1:-2] + h[2:-1] + h[3:]) / (4.0 * H)


def gates(z):
    """step 3 -> (past the absolute gate, past both gates) as boolean arrays, and the relative threshold (0 when nothing passes)"""
    pa = z > Z_ABS
    thr = 0.1 * float(z[pa].mean()) if pa.any() else 0.0
    return pa, pa & (z > thr), thr


def gate_margin(z):
    """LU between either gate and the block nearest to it (inf when no block has a finite level)"""
    pa, _, thr = gates(z)
    zz = z[z > 0]
    if zz.size == 0:
        return math.inf
    m = np.abs(10 * np.log10(zz / Z_ABS)).min()
    if thr > 0:
        m = min(m, np.abs(10 * np.log10(zz / thr)).min())
    return float(m)


def measure(x, sr):
    """steps 1 to 4 for one row -> dict(I, M, blocks=(nb, past_abs, past_both), z, margin)"""
    z = block_powers(k_filter(x, sr), sr)
    pa, pb, _ = gates(z)
    return dict(I=lufs(float(z[pb].mean())) if pb.any() else -math.inf, M=lufs(float(z.max())) if z.size else -math.inf,
                blocks=(int(z.size), int(pa.sum()), int(pb.sum())), z=z, margin=gate_margin(z))


def level(x, sr, target, ceiling):
    """steps 1 to 5 in fp64 -> the dict of measure() plus g, limited, peak_out and out"""
    x = np.asarray(x, dtype=np.float64)
    r = measure(x, sr)
    peak = float(np.abs(x).max()) if x.size else 0.0
    g, limited = 1.0, 0
    if r['I'] > -math.inf and peak > 0:
        g = 10.0 ** ((target - r['I']) / 20.0)
        if peak * g > ceiling:
            g, limited = ceiling / peak, 1
    r.update(g=g, limited=limited, peak_out=peak * g, out=x * g)
    return r


def pcm_fp32(x, g):
    """step 5 in NumPy fp32 with the device's g: out = x g (one rounded multiply), pcm = trunc(clamp(out, -1, 1) * 32767)"""
    out = np.asarray(x, dtype=np.float32) * np.float32(g)
    assert out.dtype == np.float32
    v = np.minimum(np.maximum(out, np.float32(-1.0)), np.float32(1.0))
    return out, np.trunc(v * np.float32(32767.0)).astype(np.int16)


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def sine(sr, seconds, amp=1.0, f=997.0):
    return amp * np.sin(2 * np.pi * f * np.arange(int(round(sr * seconds))) / sr)


def gating_case(sr=16000):
    """10 s of 0.1 sin(997 Hz), 5 s of zeros, 5 s of 0.001 sin: the silence falls to the absolute gate, the quiet tail to the
    relative one"""
    return np.concatenate([sine(sr, 10, 0.1), np.zeros(5 * sr), sine(sr, 5, 0.001)])


def hum_dc(L, sr):
    """60 Hz plus DC: what the high-pass is there to remove"""
    return (0.3 * np.sin(2 * np.pi * 60.0 * np.arange(L) / sr) + 0.25).astype(np.float32)


def chunk_carry_rows(chunk, sr=48000):
    """L = 5 chunks + 1: a unit impulse at the LAST sample of every chunk; a DC step in the middle of chunk 2"""
    L = 5 * chunk + 1
    a = np.zeros(L, np.float32)
    a[chunk - 1::chunk] = 1.0
    b = np.zeros(L, np.float32)
    b[2 * chunk + chunk // 2:] = 0.5
    return np.stack([a, b])
