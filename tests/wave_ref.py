"""fp64 NumPy restatement of taco_wave_finish (include/taco_hip.h) -- TEST INFRASTRUCTURE for the waveform finishing kernels of
csrc/vocoder.hip: de-emphasis with its first-order error bound, the energy trim (tests/audio_ref.py's rule with a free top_db)
and its decision margin, the peak, and PCM16 both by the entry point's fp32 rule and by write_wav's float64 rule."""
from __future__ import annotations

import numpy as np

from tests import audio_ref

TRIM_HOP = audio_ref.TRIM_HOP
SR = 16000
U = 2.0 ** -24   # unit roundoff of fp32


def coeff(a):
    """the coefficient the device sees: float32, widened"""
    return float(np.float32(a))


def _recur(x, a, lag=0):
    """y[n] = x[n - lag] + a y[n-1] in fp64 (lag 0 or 1)"""
    x = np.asarray(x, dtype=np.float64)
    y = np.zeros(len(x))
    acc = 0.0
    prev = 0.0
    for n in range(len(x)):
        acc = (x[n] if lag == 0 else prev) + a * acc
        prev = x[n]
        y[n] = acc
    return y


def deemphasis(x, a):
    """y[0] = x[0], y[n] = x[n] + a y[n-1]"""
    return _recur(x, coeff(a))


def preemphasis(y, a):
    """the front end's e[0] = y[0], e[n] = y[n] - a y[n-1]"""
    y = np.asarray(y, dtype=np.float64)
    if len(y) == 0:
        return y.copy()
    return np.append(y[0], y[1:] - coeff(a) * y[:-1])


def error_bound(x, a, const=16.0):
    """E[n] = 2^-24 (16 S[n] + 2 T[n]) + 1e-30 with S[n] = |x[n]| + a S[n-1], T[n] = a (T[n-1] + S[n-1]): the first-order bound of
    any fp32 evaluation whose lag-k term passes through at most 2k + 16 roundings"""
    a = coeff(a)
    S = _recur(np.abs(np.asarray(x, dtype=np.float64)), a)
    T = a * _recur(S, a, lag=1)   # T[n] = a S[n-1] + a T[n-1]
    return U * (const * S + 2.0 * T) + 1e-30


def frame_db(y):
    ms = audio_ref.frame_ms(y)
    return 10 * np.log10(np.maximum(1e-10, ms)) - 10 * np.log10(np.maximum(1e-10, ms.max()))


def trim_bounds(y, top_db):
    """[s, e) of taco_wave_finish step 2 for the n = len(y) samples of a row"""
    n = len(y)
    if n == 0:
        return 0, 0
    if top_db == 0:
        return 0, n
    nz = np.flatnonzero(frame_db(y) > -float(top_db))
    if nz.size == 0:
        return 0, 0
    return int(nz[0] * TRIM_HOP), int(min(n, (nz[-1] + 1) * TRIM_HOP))


def trim_margin(y, top_db):
    """decibels between the threshold and the frame nearest to it"""
    return float(np.min(np.abs(frame_db(y) + float(top_db))))


def finish(x, a, top_db):
    """-> (y (n) fp64, (s, e), peak) for one row of n = len(x) samples"""
    y = deemphasis(x, a)
    s, e = trim_bounds(y, top_db)
    peak = float(np.max(np.abs(y[s:e]))) if e > s else 0.0
    return y, (s, e), peak


def pcm_fp32(out, peak):
    """step 4 in NumPy fp32: v = peak > 1 ? y / peak : y (one rounded division), q = trunc(v * 32767) (one rounded multiply)"""
    v = np.asarray(out, dtype=np.float32)
    pk = np.float32(peak)
    if pk > np.float32(1.0):
        v = v / pk
    assert v.dtype == np.float32
    return np.trunc(v * np.float32(32767.0)).astype(np.int16)


def pcm_write_wav(samples):
    """tacotron_amd.test.write_wav's float64 rule"""
    x = np.asarray(samples, dtype=np.float64)
    peak = np.max(np.abs(x)) if x.size else 0.0
    if peak > 1.0:
        x = x / peak
    return (x * 32767.0).astype('<i2')


# ---- inputs ----------------------------------------------------------------------------------------------------------------
L_FULL = 107700   # 300 (360 - 1): the flagship inference shape


def family(name, L=L_FULL, seed=11):
    """the four signal families of the de-emphasis bound, as fp32"""
    rng = np.random.default_rng(seed)
    t = np.arange(L) / SR
    if name == 'noise':
        x = 0.1 * rng.standard_normal(L)
    elif name == 'sine_dc':
        x = 0.5 * np.sin(2 * np.pi * 110 * t) + 0.2
    elif name == 'same_sign':
        x = np.abs(0.5 * rng.standard_normal(L))
    elif name == 'bursts':
        x = np.exp(-((t * 4) % 1.0) * 6) * np.sin(2 * np.pi * 150 * t) + 0.01 * rng.standard_normal(L)
    else:
        raise ValueError(name)
    return x.astype(np.float32)


FAMILIES = ('noise', 'sine_dc', 'same_sign', 'bursts')


def burst(L, s, e, floor, seed=7):
    """floor * N(0, 1) everywhere; inside [s, e) a 180 Hz tone of amplitude 0.3 with a 3 Hz tremolo plus 0.02 N(0, 1)"""
    rng = np.random.default_rng(seed)
    x = floor * rng.standard_normal(L)
    t = np.arange(L) / SR
    tone = 0.3 * (1.0 + 0.25 * np.sin(2 * np.pi * 3 * t)) * np.sin(2 * np.pi * 180 * t) + 0.02 * rng.standard_normal(L)
    x[s:e] += tone[s:e]
    return x.astype(np.float32)


# (L, burst [s, e), floor, {top_db: fp64 bounds}); every case keeps every frame at least 1 dB from every listed threshold
TRIM_CASES = [
    (107700, (20011, 70003), 1e-5, (60.0, 40.0, 25.0)),
    (59700, (8000, 59700), 3e-6, (60.0, 40.0, 25.0)),
    (5000, (1200, 3100), 1e-5, (60.0, 40.0, 25.0)),
]
