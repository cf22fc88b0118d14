"""fp64 restatement of resampy.resample(x, sr_orig, sr_new, filter='kaiser_best') as librosa.load applies it: the literal per-output
loop of resampy's interpolation (one floating time register per output, T = t * (1 / ratio)), vectorised over the taps only.  Written
without tacotron_amd.audio.resample_filter, which the tests compare against it.  NumPy only; imports without a GPU.

The filter constants are resampy's published design for 'kaiser_best' (64 zero crossings, 512 table entries per crossing, Kaiser
beta, rolloff); like the product's copy of them they could not be compared with resampy itself offline."""
import numpy as np

NUM_ZEROS, PRECISION = 64, 9
BETA, ROLLOFF = 14.769656459379492, 0.9475937167399596
U = 2.0 ** -24                       # fp32 unit roundoff

_WIN = []


def window():
    """half window, 32769 entries"""
    if not _WIN:
        num_table = 2 ** PRECISION
        n = num_table * NUM_ZEROS
        sinc_win = ROLLOFF * np.sinc(ROLLOFF * np.linspace(0, NUM_ZEROS, n + 1))
        _WIN.append(np.kaiser(2 * n + 1, BETA)[n:] * sinc_win)
    return _WIN[0].copy()


def lengths(n_orig, sr_orig, sr_new):
    """(n_calc, n_len): resampy computes int(n ratio) samples, librosa's fix=True pads to int(ceil(n ratio))"""
    ratio = float(sr_new) / sr_orig
    return int(n_orig * ratio), int(np.ceil(n_orig * ratio))


def resample(x, sr_orig, sr_new):
    """x: 1-D samples (any float dtype; used as fp64).  -> (y (n_len) fp64 with y[n_calc:] = 0, S (n_calc) = sum |w_i x_i| per
    output, K (n_calc) the number of taps each output summed)"""
    x = np.asarray(x, dtype=np.float64)
    n_orig = len(x)
    ratio = float(sr_new) / sr_orig
    num_table = 2 ** PRECISION
    win = window()
    if ratio < 1:
        win *= ratio
    delta = np.zeros_like(win)
    delta[:-1] = np.diff(win)
    scale = min(1.0, ratio)
    step = int(scale * num_table)
    nwin = len(win)
    n_calc, n_len = lengths(n_orig, sr_orig, sr_new)
    y, S, K = np.zeros(n_len), np.zeros(n_calc), np.zeros(n_calc, dtype=np.int64)
    time_increment = 1.0 / ratio
    for t in range(n_calc):
        T = t * time_increment
        nn = int(T)
        frac = scale * (T - nn)
        f = frac * num_table
        off = int(f)
        eta = f - off
        i = np.arange(min(nn + 1, (nwin - off) // step))
        w = win[off + i * step] + eta * delta[off + i * step]
        terms = w * x[nn - i]
        frac = scale - frac
        f = frac * num_table
        off = int(f)
        eta = f - off
        k = np.arange(min(n_orig - nn - 1, (nwin - off) // step))
        w = win[off + k * step] + eta * delta[off + k * step]
        terms2 = w * x[nn + k + 1]
        y[t] = terms.sum() + terms2.sum()
        S[t] = np.abs(terms).sum() + np.abs(terms2).sum()
        K[t] = len(i) + len(k)
    return y, S, K


def bound(S, K):
    """|fp32 result - fp64 result| allowed per output: (K + 4) 2^-24 S.  In a K-term fp32 dot product summed in any order, fused or
    not, a term passes through at most K roundings (its product and K - 1 additions): K 2^-24 S to first order.  Its tap is the
    fp32 rounding of the fp64 table entry and the product of the two wings' sums is formed separately: two more roundings per tap
    and wing, the constant 4.  Derived from the arithmetic, fixed before any device result existed, not tuned to one."""
    return (K + 4) * U * S


def pcm16(x):
    """float samples in [-1, 1) -> int16, and back as the fp32 samples a decoder gives (v 2^-15)"""
    q = np.clip(np.round(np.asarray(x) * 32768.0), -32768, 32767).astype(np.int16)
    return q, q.astype(np.float32) * np.float32(2.0 ** -15)
