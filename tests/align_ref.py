"""NumPy restatement of taco_alignment_scores (include/taco_hip.h) -- the integers exactly as defined, the two means in float64 --
and of the pixel rule of tacotron_amd.alignment.attention_png.  Plain loops over rows and steps: the yardstick, not a fast path."""
import struct
import zlib

import numpy as np

MAX_JUMP = 3   # lib.MAX_JUMP


def argmax_step(row):
    """(a_t, p_t) of one step: the lowest index of the maximum of the non-NaN elements, 0 when there is none; p_t = row[a_t]"""
    ok = ~np.isnan(row)
    if not ok.any():
        return 0, float(row[0])
    m = row[ok].max()
    a = int(np.flatnonzero(ok & (row == m))[0])
    return a, float(row[a])


def scores(al, text_length, steps=None, max_jump=MAX_JUMP):
    """al (B, Td, Tt) float32 -> (counts (B, 6) int64: n, end, pad_steps, back, skip, covered; means (B, 2) float64: focus, pad_mass)"""
    al = np.asarray(al)
    B, Td, Tt = al.shape
    counts = np.zeros((B, 6), dtype=np.int64)
    means = np.zeros((B, 2), dtype=np.float64)
    for b in range(B):
        L = min(max(int(text_length[b]), 1), Tt)
        n = Td if steps is None else min(max(int(steps[b]), 0), Td)
        a, p, pad = [], [], []
        for t in range(n):
            at, pt = argmax_step(al[b, t])
            a.append(at)
            p.append(pt)
            pad.append(float(al[b, t, L:].astype(np.float64).sum()))
        counts[b, 0] = n
        counts[b, 1] = max(a) if n else 0
        counts[b, 2] = sum(1 for x in a if x >= L)
        counts[b, 3] = sum(1 for t in range(1, n) if a[t] < a[t - 1])
        counts[b, 4] = sum(1 for t in range(1, n) if a[t] > a[t - 1] + int(max_jump))
        counts[b, 5] = len({x for x in a if x < L})
        if n:
            with np.errstate(invalid='ignore'):
                means[b, 0] = np.sum(np.array(p, dtype=np.float64)) / n
                means[b, 1] = np.sum(np.array(pad, dtype=np.float64)) / n
    return counts, means


def means_bound(Td, Tt):
    """|fp32 mean - fp64 mean| for means of at most Td terms in [0, 1], each a sum of at most Tt non-negative fp32 terms: any fp32
    summation order stays inside (Tt + Td) 2^-24 relative to a value of at most 1; the tests allow twice that"""
    return (Tt + Td) * 2.0 ** -23


# ---- the picture ---------------------------------------------------------------------------------------------------------------
HOT = {'r': ((0.0, 0.0416), (0.365079, 1.0), (1.0, 1.0)),
       'g': ((0.0, 0.0), (0.365079, 0.0), (0.746032, 1.0), (1.0, 1.0)),
       'b': ((0.0, 0.0), (0.746032, 0.0), (1.0, 1.0))}


def _piecewise(points, x):
    for (x0, y0), (x1, y1) in zip(points[:-1], points[1:]):
        if x0 <= x <= x1:
            return (y1 - y0) / (x1 - x0) * (x - x0) + y0
    raise ValueError(x)


def hot_table():
    """256 x 3 bytes: each channel at linspace(0, 1, 256) in float64, uint8(v * 255) truncated"""
    xs = np.linspace(0.0, 1.0, 256)
    return np.array([[int(_piecewise(HOT[ch], float(x)) * 255) for ch in 'rgb'] for x in xs], dtype=np.uint8)


def pixels(align, n=None, zoom=4):
    """(n zoom, Tt zoom, 3) uint8: cell (t, s) is hot_table()[clip(int(256 (x - min) / (max - min)), 0, 255)] in float32 arithmetic,
    min / max over the drawn cells that are not NaN; a constant picture and a NaN cell take index 0"""
    a = np.asarray(align, dtype=np.float32)
    n = a.shape[0] if n is None else n
    a = a[:n]
    vals = [x for x in a.reshape(-1) if not np.isnan(x)]
    lo = np.float32(min(vals)) if vals else np.float32(0)
    hi = np.float32(max(vals)) if vals else np.float32(0)
    table = hot_table()
    out = np.zeros((n * zoom, a.shape[1] * zoom, 3), dtype=np.uint8)
    for t in range(n):
        for s in range(a.shape[1]):
            x = a[t, s]
            k = 0
            if hi > lo and not np.isnan(x):
                k = min(max(int(np.float32(np.float32(np.float32(x - lo) / np.float32(hi - lo)) * np.float32(256))), 0), 255)
            out[t * zoom:(t + 1) * zoom, s * zoom:(s + 1) * zoom] = table[k]
    return out


def read_png(path):
    """an 8-bit RGB, non-interlaced PNG whose scanlines all use filter 0 -> (h, w, 3) uint8 (zlib and struct only)"""
    data = open(path, 'rb').read()
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    at, idat, head = 8, b'', None
    while at < len(data):
        size, kind = struct.unpack('>I4s', data[at:at + 8])
        body = data[at + 8:at + 8 + size]
        assert struct.unpack('>I', data[at + 8 + size:at + 12 + size])[0] == zlib.crc32(kind + body) & 0xffffffff
        if kind == b'IHDR':
            head = struct.unpack('>IIBBBBB', body)
        elif kind == b'IDAT':
            idat += body
        at += 12 + size
    w, h, depth, colour, comp, filt, lace = head
    assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(h, 1 + 3 * w)
    assert not raw[:, 0].any()
    return raw[:, 1:].reshape(h, w, 3)
