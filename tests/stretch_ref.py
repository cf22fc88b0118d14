"""NumPy restatement of taco_frames_stretch (include/taco_hip.h): the speaking-rate resampling of magnitude frames, in float32,
one row at a time.  Imports without a GPU and without the library; the constants are restated, not imported, so that
tests/test_frames_stretch_host.py can hold the header and tacotron_amd.lib to them."""
import numpy as np

ONE, MIN_STEP, MAX_STEP, MAX_FRAMES = 65536, 16384, 262144, 8192


def clamp_step(step_q):
    return min(max(int(step_q), MIN_STEP), MAX_STEP)


def row_frames(frames_b, frames_per_unit, F):
    """F_b: frames[b] * frames_per_unit (Python integers: no overflow) clamped to [0, F]; None: F"""
    if frames_b is None:
        return int(F)
    return min(max(int(frames_b) * int(frames_per_unit), 0), int(F))


def out_frames(F_b, step_q, Fo=None):
    """Fo_b: 0 for an empty row, else ((F_b - 1) << 16) // s_b + 1, at most Fo when given"""
    if F_b <= 0:
        return 0
    n = ((int(F_b) - 1) << 16) // clamp_step(step_q) + 1
    return n if Fo is None else min(int(Fo), n)


def positions(Fo_b, step_q):
    """(i, frac) of output frames 0 .. Fo_b - 1: p = j s_b, i = p >> 16, frac = p & 0xFFFF"""
    p = np.arange(Fo_b, dtype=np.int64) * clamp_step(step_q)
    return p >> 16, p & 0xFFFF


def stretch(mag_t, frames=None, step_q=None, frames_per_unit=1, Fo=None):
    """mag_t (B, C, F) float32 -> (out (B, C, Fo) float32, frames_out (B) int32).  frames / step_q: None or B integers.
    Fo: default the largest Fo_b of the batch (at least 1)."""
    mag_t = np.asarray(mag_t)
    assert mag_t.dtype == np.float32 and mag_t.ndim == 3
    B, C, F = mag_t.shape
    Fb = [row_frames(None if frames is None else frames[b], frames_per_unit, F) for b in range(B)]
    sq = [ONE if step_q is None else int(step_q[b]) for b in range(B)]
    if Fo is None:
        Fo = max(1, max(out_frames(Fb[b], sq[b]) for b in range(B)))
    out = np.zeros((B, C, Fo), dtype=np.float32)
    frames_out = np.zeros(B, dtype=np.int32)
    for b in range(B):
        n = out_frames(Fb[b], sq[b], Fo)
        frames_out[b] = n
        if n == 0:
            continue
        i, frac = positions(n, sq[b])
        w = frac.astype(np.float32) * np.float32(2.0 ** -16)            # exact
        exact = frac == 0
        assert i.max() <= Fb[b] - 1 and (i[~exact] + 1 <= Fb[b] - 1).all()
        i1 = np.where(exact, i, i + 1)                                   # (w == 0: element i + 1 is not touched)
        row = mag_t[b, :, :Fb[b]]                                        # nothing behind F_b can be reached
        a, c = row[:, i], row[:, i1]
        with np.errstate(invalid='ignore', over='ignore'):
            d = (c - a).astype(np.float32)
            m = (w[None, :] * d).astype(np.float32)
            y = (a + m).astype(np.float32)
        out[b, :, :n] = np.where(exact[None, :], a, y)
    return out, frames_out
