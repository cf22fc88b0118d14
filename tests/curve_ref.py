"""NumPy restatements of the three prosody-curve entry points (include/taco_hip.h): taco_path_curve, taco_frames_stretch_curve and
taco_frames_pitch_curve.  The time map is integer arithmetic in Python / int64 (no overflow to reason about), the interpolation
float32 as tests/stretch_ref.py does it, the pitch per frame through tests/pitch_ref.shift_frames.  Imports without a GPU and
without the library; the constants are restated, not imported."""
import numpy as np

from tests import pitch_ref as pr
from tests import stretch_ref as sr

ONE, MIN_DUR, MAX_DUR, MAX_FRAMES = 65536, 16384, 262144, 8192


def path_curve(path, values, r, fill):
    """path (B, Td), values (B, Tt) integers -> curve (B, Td r) int32"""
    path, values = np.asarray(path), np.asarray(values)
    B, Td = path.shape
    Tt = values.shape[1]
    curve = np.full((B, Td * r), fill, dtype=np.int32)
    for b in range(B):
        for t in range(Td):
            if 0 <= path[b, t] < Tt:
                curve[b, t * r:(t + 1) * r] = values[b, path[b, t]]
    return curve


def clamp_dur(d):
    return np.clip(np.asarray(d, dtype=np.int64), MIN_DUR, MAX_DUR)


def starts(dur_row, Fb):
    """(D (Fb) int64 with D_0 = 0, D_{i+1} = D_i + d_i; d (Fb) int64, clamped) of a row's first Fb durations (None: 65536)"""
    d = np.full(Fb, ONE, dtype=np.int64) if dur_row is None else clamp_dur(dur_row[:Fb])
    D = np.concatenate([[0], np.cumsum(d)[:-1]]).astype(np.int64)
    return D, d


def time_map(dur_row, Fb, Fo):
    """(Fo_b, i, wq) of one row: i and wq int64 arrays over j < Fo_b"""
    if Fb <= 0:
        return 0, np.zeros(0, np.int64), np.zeros(0, np.int64)
    D, d = starts(dur_row, Fb)
    n = int(min(Fo, (int(D[Fb - 1]) >> 16) + 1))
    q = np.arange(n, dtype=np.int64) << 16
    i = np.searchsorted(D, q, side='right') - 1            # the largest i with D_i <= q (D rises strictly)
    assert (i >= 0).all() and (i <= Fb - 1).all()
    wq = ((q - D[i]) << 16) // d[i]
    assert (wq >= 0).all() and (wq < 65536).all()
    return n, i, wq


def stretch_curve(mag_t, frames=None, dur_q=None, frames_per_unit=1, Fo=None):
    """mag_t (B, C, F) float32, dur_q None or (B, F) integers -> (out (B, C, Fo) float32, frames_out (B) int32, src (B, Fo) int32)"""
    mag_t = np.asarray(mag_t)
    assert mag_t.dtype == np.float32 and mag_t.ndim == 3
    B, C, F = mag_t.shape
    Fb = [sr.row_frames(None if frames is None else frames[b], frames_per_unit, F) for b in range(B)]
    maps = [time_map(None if dur_q is None else dur_q[b], Fb[b], MAX_FRAMES if Fo is None else Fo) for b in range(B)]
    if Fo is None:
        Fo = max(1, max(m[0] for m in maps))
    out = np.zeros((B, C, Fo), dtype=np.float32)
    frames_out = np.zeros(B, dtype=np.int32)
    src = np.full((B, Fo), -1, dtype=np.int32)
    for b, (n, i, wq) in enumerate(maps):
        frames_out[b] = n
        if n == 0:
            continue
        src[b, :n] = (i << 16) | wq
        w = wq.astype(np.float32) * np.float32(2.0 ** -16)               # exact
        exact = wq == 0
        assert i.max() <= Fb[b] - 1 and (i[~exact] + 1 <= Fb[b] - 1).all()   # i == F_b - 1 only with wq == 0
        i1 = np.where(exact, i, i + 1)
        row = mag_t[b, :, :Fb[b]]
        a, c = row[:, i], row[:, i1]
        with np.errstate(invalid='ignore', over='ignore'):
            dd = (c - a).astype(np.float32)
            m = (w[None, :] * dd).astype(np.float32)
            y = (a + m).astype(np.float32)
        out[b, :, :n] = np.where(exact[None, :], a, y)
    return out, frames_out, src


def pitch_curve(mag_t, frames=None, step_q=None, frames_per_unit=1, lifter=32, dtype=np.float64):
    """mag_t (B, C, F) float32, step_q None or (B, F) integers -> out (B, C, F) in `dtype`: every frame through
    pitch_ref.shift_frames at its own clamped step; a frame at 65536 is the frame itself; zeros behind F_b"""
    mag_t = np.asarray(mag_t)
    B, C, F = mag_t.shape
    out = np.zeros((B, C, F), dtype=dtype)
    for b in range(B):
        Fb = pr.row_frames(None if frames is None else frames[b], frames_per_unit, F)
        s = np.full(Fb, pr.ONE, dtype=np.int64) if step_q is None else np.array([pr.clamp_step(x) for x in step_q[b][:Fb]], dtype=np.int64)
        for step in np.unique(s):
            cols = np.flatnonzero(s == step)
            out[b][:, cols] = mag_t[b][:, cols] if step == pr.ONE else pr.shift_frames(mag_t[b][:, cols], int(step), lifter, dtype)
    return out


def map_frames(src_row, Fo_b, frame):
    """the output frame of source frame `frame` under a row's time map: searchsorted(src[:Fo_b], frame << 16)"""
    return int(np.searchsorted(np.asarray(src_row[:Fo_b], dtype=np.int64), int(frame) << 16))
