"""Host side of the alignment monitor: what the per-utterance scores of lib.alignment_scores say about a row (`flags`) and the
attention picture of the reference (data_input.generate_attention_plot, drawn by train.py:92-103 and test.py:60-69) as a PNG
without axes (`attention_png`).  NumPy, zlib and struct only: a picture of Td x Tt cells is host work, the scores are not."""
from __future__ import annotations

import struct
import zlib

import numpy as np

from .lib import ALIGN_COUNTS, ALIGN_MEANS

FLAGS = ('unfinished', 'skips', 'goes back', 'on padding', 'diffuse')

# matplotlib's `hot` map: (x, y) break points of its three piecewise-linear channels
HOT = (((0.0, 0.0416), (0.365079, 1.0), (1.0, 1.0)),
       ((0.0, 0.0), (0.365079, 0.0), (0.746032, 1.0), (1.0, 1.0)),
       ((0.0, 0.0), (0.746032, 0.0), (1.0, 1.0)))


def scores_row(counts, means):
    """the 8 values of one utterance as float64: counts (ALIGN_COUNTS order), then means (ALIGN_MEANS order)"""
    c, m = np.asarray(counts).reshape(-1), np.asarray(means).reshape(-1)
    if c.shape != (len(ALIGN_COUNTS),) or m.shape != (len(ALIGN_MEANS),):
        raise ValueError('scores_row: expected %d counts and %d means, got %s and %s' % (len(ALIGN_COUNTS), len(ALIGN_MEANS), c.shape, m.shape))
    return np.concatenate([c.astype(np.float64), m.astype(np.float64)])


def flags(counts, means, L, end_offset=1, min_covered=0.8, max_skip=2, max_back=2, max_pad_steps=0.1, max_pad_mass=0.1, min_focus=0.3):
    """What is wrong with one row, from its scores: counts (6) and means (2) of lib.alignment_scores, L its text length.
      'unfinished'  end < max(0, L - 1 - end_offset), the stop rule's target, or covered < min_covered L (also a row of 0 steps)
      'skips'       skip > max_skip: the argmax jumped forward by more than max_jump characters that often
      'goes back'   back > max_back
      'on padding'  pad_steps > max_pad_steps n, or pad_mass > max_pad_mass
      'diffuse'     focus < min_focus, or focus is NaN
    Returns the names that apply, in the order of FLAGS; [] for a row that read its text.  Every threshold is a choice of the
    author: none is tuned on a trained model."""
    n, end, pad_steps, back, skip, covered = (int(x) for x in np.asarray(counts).reshape(-1))
    focus, pad_mass = (float(x) for x in np.asarray(means).reshape(-1))
    L = max(1, int(L))
    out = []
    if n == 0 or end < max(0, L - 1 - int(end_offset)) or covered < min_covered * L:
        out.append('unfinished')
    if n == 0:
        return out
    if skip > max_skip:
        out.append('skips')
    if back > max_back:
        out.append('goes back')
    if pad_steps > max_pad_steps * n or not pad_mass <= max_pad_mass:
        out.append('on padding')
    if not focus >= min_focus:   # (a NaN focus is diffuse)
        out.append('diffuse')
    return out


def hot_table():
    """matplotlib's `hot` colour map as 256 RGB bytes: each channel's break points interpolated in float64 at linspace(0, 1, 256),
    the byte uint8(v * 255), truncated"""
    x = np.linspace(0.0, 1.0, 256)
    lut = np.stack([np.interp(x, [p[0] for p in ch], [p[1] for p in ch]) for ch in HOT], axis=1)
    return (lut * 255).astype(np.uint8)


def attention_pixels(align, n=None, zoom=4):
    """The picture of attention_png as a (n zoom, Tt zoom, 3) uint8 array."""
    a = np.asarray(align, dtype=np.float32)
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError('attention_png: align must have shape (Td, Tt), got %s' % (a.shape,))
    n = a.shape[0] if n is None else int(n)
    zoom = int(zoom)
    if not 1 <= n <= a.shape[0]:
        raise ValueError('attention_png: n must be in 1..%d, got %d' % (a.shape[0], n))
    if zoom < 1:
        raise ValueError('attention_png: zoom must be >= 1, got %d' % zoom)
    a = a[:n]
    bad = np.isnan(a)
    lo, hi = (np.float32(a[~bad].min()), np.float32(a[~bad].max())) if not bad.all() else (np.float32(0), np.float32(0))
    index = np.zeros(a.shape, dtype=np.int64)
    if hi > lo:   # float32 throughout, as matplotlib's Normalize keeps a float32 image
        with np.errstate(invalid='ignore'):
            v = (a - lo) / np.float32(hi - lo) * np.float32(256)
        index = np.clip(np.where(bad, 0, v).astype(np.int64), 0, 255)
    rgb = hot_table()[index]
    return np.repeat(np.repeat(rgb, zoom, axis=0), zoom, axis=1)


def _chunk(kind, data):
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data) & 0xffffffff)


def attention_png(path, align, n=None, zoom=4):
    """The reference's attention picture without axes: align (Td, Tt) -> an 8-bit RGB PNG at `path` of n zoom x Tt zoom pixels.
    Rows are the decoder steps 0 .. n - 1 from the top (n None: all Td), columns the Tt characters, each cell zoom x zoom pixels.
    Colour: matplotlib's `hot` map (hot_table) at index clip(int(256 (x - min) / (max - min)), 0, 255), float32 arithmetic, min and
    max over the drawn cells without their NaNs; a constant picture and a NaN cell get index 0.  On a float32 image without NaN
    these are the bytes of matplotlib.colormaps['hot'](Normalize()(a), bytes=True)."""
    px = attention_pixels(align, n, zoom)
    h, w, _ = px.shape
    raw = np.concatenate([np.zeros((h, 1), dtype=np.uint8), px.reshape(h, w * 3)], axis=1).tobytes()   # filter type 0 per scanline
    with open(path, 'wb') as f:
        f.write(b'\x89PNG\r\n\x1a\n' + _chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 2, 0, 0, 0))
                + _chunk(b'IDAT', zlib.compress(raw, 6)) + _chunk(b'IEND', b''))
    return h, w
