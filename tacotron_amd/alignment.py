"""Host side of the alignment monitor: what the per-utterance scores of lib.alignment_scores say about a row (`flags`) and the
attention picture of the reference (data_input.generate_attention_plot, drawn by train.py:92-103 and test.py:60-69) as a PNG
without axes (`attention_png`).  NumPy, zlib and struct only: a picture of Td x Tt cells is host work, the scores are not.

Timings (`char_steps`, `step_samples`, `word_times`): the arithmetic that turns the per-character durations of lib.alignment_path
into seconds of the file a prompt was written to.  RESOLUTION: the r-frame layout (audio.reshape_frames) interleaves the frames of
the 4 decoder steps of a block, so a boundary is exact at multiples of 4 steps and nominal (frame r t) inside a block: the blur is
up to one block, 4 r frames = 150 ms at r = 2 and 16 kHz.  Good enough for subtitles; this is not a phonetic aligner.
Behind a rate that varies inside the utterance (lib.frames_stretch_curve) a boundary goes through the time map `src` of that call:
source frame r t becomes the first output frame at or behind it, which adds a resolution of one output frame (18.75 ms) on top.

Prosody (`word_values`): one value per encoded character from one value per word -- the `values` that lib.path_curve spreads along the
path."""
from __future__ import annotations

import struct
import zlib

import numpy as np

from .lib import ALIGN_COUNTS, ALIGN_MEANS

HOP, SR = 300, 16000   # samples per frame and per second (audio.py)
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


# ---- timings: durations in decoder steps -> seconds of the written file -----------------------------------------------------------
def char_steps(dur):
    """dur (L,) steps per character (lib.alignment_path) -> (start, end): character s is spoken over the steps start[s] .. end[s] - 1;
    cumulative sums, so a skipped character (dur 0) has start == end, the step at which its neighbours meet"""
    d = np.asarray(dur, dtype=np.int64).reshape(-1)
    if (d < 0).any():
        raise ValueError('char_steps: durations must be >= 0, got %s' % (d[d < 0][:4],))
    end = np.cumsum(d)
    return end - d, end


def step_samples(t, r, step_q=None, trim=None, offset=0, total=None, src=None):
    """Decoder step(s) t -> sample position(s) in the written file, float64.  Step t sits at source frame r t and at sample 300 r t;
    with a rate (step_q: the Q16 step of lib.frames_stretch, 65536 the model's own) the frame becomes r t 65536 / step_q.  trim = (s, e)
    of a finished waveform (prompt_NNN_trim.npy): s is subtracted and the result clipped to [0, e - s]; without finishing the result is
    clipped to [0, total], total the 300 (frames - 1) samples the file holds (None: unclipped).  offset: where the piece starts in a
    joined file (--long), added last.  Nominal inside a block of 4 steps: see the module's note on resolution.
    src: the time map of one row of lib.frames_stretch_curve cut to its Fo_b entries ((i << 16) | wq, rising strictly), in place of
    step_q: source frame r t becomes output frame searchsorted(src, (r t) << 16), the first output frame at or behind it (Fo_b
    for a step behind the row's end) -- a resolution of one output frame."""
    if src is not None and step_q is not None:
        raise ValueError('step_samples: give step_q (one rate) or src (a time map), not both')
    frame = np.asarray(t, dtype=np.float64) * int(r)
    if src is not None:
        m = np.asarray(src, dtype=np.int64).reshape(-1)
        if (m < 0).any() or (np.diff(m) <= 0).any():
            raise ValueError('step_samples: src must be the first Fo_b entries of a time map: non-negative and rising strictly')
        frame = np.searchsorted(m, (np.asarray(t, dtype=np.int64) * int(r)) << 16).astype(np.float64)
    if step_q is not None:
        frame = frame * 65536.0 / int(step_q)
    x = frame * HOP
    if trim is not None:
        s, e = int(trim[0]), int(trim[1])
        x = np.clip(x - s, 0, max(0, e - s))
    elif total is not None:
        x = np.clip(x, 0, max(0, int(total)))
    return x + int(offset)


def encoded_chars(line, ivocab):
    """the characters of a raw line that data.load_prompts encodes, in order: those of line.strip() that the vocabulary holds"""
    known = set(ivocab.values())
    return [w for w in line.strip() if w in known]


def word_spans(chars):
    """[(i, j)] of the words of a list of characters: maximal runs of non-space characters, i .. j inclusive"""
    out, i = [], 0
    while i < len(chars):
        if chars[i] == ' ':
            i += 1
            continue
        j = i
        while j + 1 < len(chars) and chars[j + 1] != ' ':
            j += 1
        out.append((i, j))
        i = j + 1
    return out


def word_values(line, ivocab, per_word, base):
    """One value per encoded character of a prompt from one value per word: per_word {word index: value}, words as word_times
    defines them (0-based, maximal runs of encoded non-space characters, punctuation attached).  The characters of a listed word
    take its value; spaces, the words not listed and everything behind the text take `base` (the caller pads with it).
    ValueError for a word index the prompt does not have.  -> (list of len(encoded_chars) values, the number of words)"""
    chars = encoded_chars(line, ivocab)
    spans = word_spans(chars)
    out = [base] * len(chars)
    for w, v in per_word.items():
        if isinstance(w, bool) or int(w) != w or not 0 <= int(w) < len(spans):
            raise ValueError('word_values: word %r: the prompt has the words 0 .. %d' % (w, len(spans) - 1))
        i, j = spans[int(w)]
        out[i:j + 1] = [v] * (j + 1 - i)
    return out, len(spans)


def word_times(line, ivocab, dur, r, step_q=None, trim=None, offset=0, total=None, sr=SR, src=None):
    """[(start_s, end_s, word)] of one prompt (or one piece of a --long prompt): `dur` its per-character steps (lib.alignment_path; entry
    i belongs to encoded character i -- text_length also counts the newline and the dropped characters, so dur may be longer than the
    encoded text and the surplus is ignored; a shorter dur counts as 0 steps for the rest).  A word is a maximal run of encoded
    non-space characters, punctuation attached; it starts with the first step of its first character and ends with the last step of
    its last one (char_steps), mapped to seconds by step_samples(...) / sr.  A word whose characters were all skipped has start == end.
    src: the row's time map behind lib.frames_stretch_curve, cut to Fo_b entries (step_samples), in place of step_q."""
    chars = encoded_chars(line, ivocab)
    d = np.zeros(len(chars), dtype=np.int64)
    given = np.asarray(dur, dtype=np.int64).reshape(-1)[:len(chars)]
    d[:len(given)] = given
    start, end = char_steps(d)
    out = []
    for i, j in word_spans(chars):
        a, b = step_samples([start[i], end[j]], r, step_q, trim, offset, total, src) / float(sr)
        out.append((float(a), float(b), ''.join(chars[i:j + 1])))
    return out


def words_tsv(rows):
    """the text of prompt_NNN_words.tsv: start_s<TAB>end_s<TAB>word, milliseconds kept"""
    return ''.join('%.3f\t%.3f\t%s\n' % row for row in rows)


def path_line(who, counts, mass, L, end_offset=1):
    """(the line --timings prints for one row, whether it is a WARNING): counts (3) and mass of lib.alignment_path, L the text length"""
    n, end, skipped = (int(x) for x in np.asarray(counts).reshape(-1))
    L = max(1, int(L))
    short = end < L - 1 - int(end_offset)
    text = '%s path: mass per step %.3f over %d steps, end %d of %d, %d skipped' % (who, float(mass) / n if n else 0.0, n, end, L - 1, skipped)
    return ('WARNING ' + text + ': the path ends before the text does') if short else text, short
