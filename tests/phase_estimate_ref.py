"""NumPy restatement of the single-pass phase estimate (include/taco_hip.h taco_phase_estimate) -- TEST INFRASTRUCTURE ONLY.

Beauregard, Harish and Wyse, "Single pass spectrogram inversion" (DSP 2015), in the form the C ABI states it: every spectral peak of a
frame is a sinusoid, its frequency refined by a parabola through three bins, its phase advanced by hop x frequency from the previous
frame, and the bins of its lobe locked to it.  Only fp32 subtraction, multiplication, one IEEE division and integers: float32 /
uint32 / int64 here give the bits of the device, and the GPU tests demand that.

`edge_rows`: the edge frames the GPU test splices into otherwise ordinary rows."""
import numpy as np

K, N_FFT, HOP = 1025, 2048, 300
SCALE = np.float32(2.0 * np.pi / 16777216.0)   # 2 pi / 2^24 as the fp32 constant of step 6


def frame_tables(m):
    """steps 1 to 4 of one frame: m (K) float32 magnitudes (already absolute) -> (own (K) int64, -1 = none; adv (K) uint32 of every
    bin's OWN parabola, meaningful at peaks only)"""
    m = np.asarray(m, dtype=np.float32)
    j = np.arange(K, dtype=np.int64)
    peak = np.zeros(K, dtype=bool)
    with np.errstate(invalid='ignore'):
        peak[1:K - 1] = (m[1:K - 1] > m[0:K - 2]) & (m[1:K - 1] >= m[2:K])
    a, b, c = np.zeros(K, np.float32), m, np.zeros(K, np.float32)
    a[1:], c[:K - 1] = m[:K - 1], m[1:]
    with np.errstate(all='ignore'):
        den = (a - np.float32(2.0) * b) + c
        p = np.where(den == 0, np.float32(0.0), (np.float32(0.5) * (a - c)) / np.where(den == 0, np.float32(1.0), den)).astype(np.float32)
        p = np.where(np.isfinite(p), np.clip(p, np.float32(-0.5), np.float32(0.5)), np.float32(0.0)).astype(np.float32)
        q = np.rint(p * np.float32(65536.0)).astype(np.int64)
    adv = (((300 * (j * 65536 + q)) << 5) & 0xFFFFFFFF).astype(np.uint32)
    left = np.maximum.accumulate(np.where(peak, j, -1))
    big = 1 << 30
    sufmin = np.minimum.accumulate(np.where(peak, j, big)[::-1])[::-1]        # smallest peak index >= j
    right = np.full(K, -1, dtype=np.int64)
    right[:K - 1] = np.where(sufmin[1:] == big, -1, sufmin[1:])
    rising = np.zeros(K, dtype=bool)
    with np.errstate(invalid='ignore'):
        rising[:K - 1] = m[1:] > m[:K - 1]
    return np.where(rising, right, left), adv


def frame_update(acc, m):
    """step 5: acc (K) uint32 in front of the frame, m (K) magnitudes -> acc' (K) uint32"""
    own, adv = frame_tables(np.abs(np.asarray(m, dtype=np.float32)))
    o = np.maximum(own, 0)
    return np.where(own >= 0, (acc[o].astype(np.int64) + adv[o].astype(np.int64)) & 0xFFFFFFFF, acc.astype(np.int64)).astype(np.uint32)


def phase_of(acc):
    """step 6: acc' (K) uint32 -> (K) float32 radians"""
    j = np.arange(K, dtype=np.int64)
    u = ((acc.astype(np.int64) + (j << 31)) & 0xFFFFFFFF) >> 8
    return u.astype(np.float32) * SCALE


def phase_estimate_row(mag, Fb=None):
    """mag (K, F) -> phase0 (K, F) float32 over the first Fb frames (None: all), exactly 0 behind; columns t >= Fb are never read"""
    mag = np.asarray(mag)
    F = mag.shape[1]
    Fb = F if Fb is None else max(0, min(int(Fb), F))
    out = np.zeros((K, F), dtype=np.float32)
    acc = np.zeros(K, dtype=np.uint32)
    for t in range(Fb):
        acc = frame_update(acc, mag[:, t])
        out[:, t] = phase_of(acc)
    return out


def phase_estimate(mag_t, frames=None, frames_per_unit=1):
    """mag_t (B, K, F), frames (B) or None -> phase0 (B, K, F) float32"""
    mag_t = np.asarray(mag_t)
    B = mag_t.shape[0]
    return np.stack([phase_estimate_row(mag_t[b], None if frames is None else int(frames[b]) * int(frames_per_unit)) for b in range(B)])


# ---- edge frames (GPU test): each a (K) float32 column of normal fp32 numbers ----------------------------------------------------------
def _ordinary(rng):
    return (np.abs(rng.standard_normal(K)) + 0.05).astype(np.float32)


def edge_frames(seed=0):
    """{name: (K) float32}"""
    rng = np.random.default_rng(seed)
    e = {}
    x = _ordinary(rng)
    x[300:340] = np.float32(0.75)                       # a plateau inside the row
    e['plateau_inside'] = x
    x = _ordinary(rng)
    x[0:25] = np.float32(0.6)                           # ... and one reaching bin 0
    e['plateau_bin0'] = x
    e['all_zero'] = np.zeros(K, dtype=np.float32)       # no peaks: every accumulator is carried across it
    x = np.full(K, 0.1, dtype=np.float32)
    x[1], x[1023] = 2.0, 3.0                            # peaks at bins 1 and 1023 (and a flat floor between them)
    e['peaks_1_1023'] = x
    e['rising'] = (0.01 + np.arange(K) * 1e-3).astype(np.float32)      # monotone up to bin 1024: no owner anywhere
    e['falling'] = (2.0 - np.arange(K) * 1e-3).astype(np.float32)      # monotone down: no peak, nothing rises
    e['negative'] = (-_ordinary(rng)).astype(np.float32)                # the absolute value is taken
    x = _ordinary(rng)
    x[500:503] = (1e-10, 1.0, 1.0)                      # a = 1e-10, b = c = 1
    x[503] = 0.5
    x[600:603] = (np.nextafter(np.float32(1.0), np.float32(0.0)), 1.0, 1.0)   # (a - 2 b) + c rounds to 0: p = 0
    x[603] = 0.5
    e['den_zero'] = x
    x = np.full(K, 0.2, dtype=np.float32)
    x[400:405] = (0.2, 1.0, 0.5, 0.5, 1.5)              # two peaks around a trough of two equal bins
    x[405] = 0.3
    x[700:703] = (1.0, 0.4, 1.0)                        # ... and around one bin with equal neighbours left and right
    x[699], x[703] = 0.3, 0.3
    e['shared_trough'] = x
    return e


def splice(mag, columns):
    """a copy of mag (K, F) with the given {t: (K) column} put in"""
    out = np.array(mag, dtype=np.float32, copy=True)
    for t, col in columns.items():
        out[:, t] = col
    return out
