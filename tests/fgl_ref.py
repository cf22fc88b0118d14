"""fp64 NumPy restatement of fast Griffin-Lim (include/taco_hip.h taco_griffinlim_fast) -- TEST INFRASTRUCTURE ONLY.

Perraudin, Balazs and Sondergaard, "A fast Griffin-Lim algorithm" (2013), in the form the C ABI states it, on the stft / istft of
oracle/griffinlim_numpy.py:  t_i = STFT(ISTFT(M angles_i)),  c_i = t_i (i = 0) or t_i + a (t_i - t_{i-1}),  angles_{i+1} = the
unit phasor of c_i.  The phasor is formed as the oracle forms it (exp(1j * angle(.)), angle(0) = 0), so that momentum 0 is
oracle.griffinlim_numpy.griffinlim to the last bit.  Next to the waveform it returns the n_iter + 1 spectral-convergence values
|| |t_i| - M || / || M ||: in front of every round, and of the waveform returned.

`case` / `speechy`: the four inputs the momentum claim was measured on."""
import numpy as np

from oracle import griffinlim_numpy as gl


def griffinlim_fast(mag, angles0, n_iter, momentum):
    """mag (1025, F), angles0 (1025, F) radians -> (waveform (300 (F - 1)), conv (n_iter + 1))"""
    mag = np.abs(np.asarray(mag, dtype=np.float64))
    angles = np.exp(1j * np.asarray(angles0, dtype=np.float64))
    norm = np.linalg.norm(mag)
    conv, prev = [], None
    for i in range(n_iter):
        t = gl.stft(gl.istft(mag * angles))
        conv.append(np.linalg.norm(np.abs(t) - mag) / norm if norm > 0 else 0.0)
        c = t if (i == 0 or momentum == 0) else t + momentum * (t - prev)
        prev = t
        angles = np.exp(1j * np.angle(c))
    wave = gl.istft(mag * angles)
    conv.append(np.linalg.norm(np.abs(gl.stft(wave)) - mag) / norm if norm > 0 else 0.0)
    return wave, np.array(conv)


def case(F, seed):
    """`_case` of tests/test_gpu_vocoder.py: a magnitude matrix that IS the STFT of a signal, plus noise-floor bins; random phases"""
    rng = np.random.default_rng(seed)
    y = np.cumsum(rng.standard_normal(300 * (F - 1))) * 0.01 + np.sin(np.arange(300 * (F - 1)) * 0.05)
    mag = np.abs(gl.stft(y)) + 1e-3
    ph = 2 * np.pi * rng.random(mag.shape)
    return mag, ph


def speechy(F, seed):
    """24 harmonics of a vibrato pitch (120 +- 30 Hz) under a 3 Hz syllable envelope, plus a noise floor"""
    rng = np.random.default_rng(seed)
    n = 300 * (F - 1)
    t = np.arange(n) / 16000.0
    f0 = 120 + 30 * np.sin(2 * np.pi * 0.7 * t)
    phi = 2 * np.pi * np.cumsum(f0) / 16000.0
    y = sum(np.sin(k * phi) / k for k in range(1, 25)) * (0.5 + 0.5 * np.sin(2 * np.pi * 3 * t)) ** 2 + 0.02 * rng.standard_normal(n)
    mag = np.abs(gl.stft(y))
    ph = 2 * np.pi * rng.random(mag.shape)
    return mag, ph


CASES = (('case(24, 11)', case, 24, 11), ('case(41, 3)', case, 41, 3), ('speechy(96, 1)', speechy, 96, 1),
         ('speechy(96, 2)', speechy, 96, 2))


def fp32_inputs(fn, F, seed):
    """the inputs as the device sees them: rounded to fp32, handed to the restatement in fp64"""
    mag, ph = fn(F, seed)
    return mag.astype(np.float32), ph.astype(np.float32)
