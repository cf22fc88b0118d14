"""fp64 NumPy restatement of audio.process_audio (audio.py:38-65) -- TEST INFRASTRUCTURE for csrc/features.hip.

Builds on oracle/griffinlim_numpy.stft (librosa's center=True STFT, checked against scipy in tests/test_oracle.py) and
tacotron_amd.audio.reshape_frames (pinned by tests/golden/reshape_frames.npz), and adds librosa.effects.trim (0.6 form), the
drop / zero-pad to max_len, pre-emphasis, the complex mel product and the logs.  PARITY WITH LIBROSA IS UNPINNED: librosa is
not available here; the trim and mel steps restate its published algorithm."""
from __future__ import annotations

import numpy as np

from oracle import griffinlim_numpy as gl
from tacotron_amd.audio import MAXIMUM_AUDIO_LENGTH, mel_basis, reshape_frames

TRIM_FRAME, TRIM_HOP, TOP_DB = 2048, 512, 60.0


def frame_ms(y):
    """librosa.feature.rmse(y, 2048, 512, center=True) ** 2: mean squares of frames of the signal reflect-padded by 1024."""
    yp = np.pad(np.asarray(y, dtype=np.float64), TRIM_FRAME // 2, mode='reflect')
    n = 1 + (len(yp) - TRIM_FRAME) // TRIM_HOP
    return np.array([np.mean(yp[t * TRIM_HOP:t * TRIM_HOP + TRIM_FRAME] ** 2) for t in range(n)])


def trim_bounds(y):
    """librosa.effects.trim(y) (top_db 60, ref max) -> (start, end) in samples."""
    ms = frame_ms(y)
    db = 10 * np.log10(np.maximum(1e-10, ms)) - 10 * np.log10(np.maximum(1e-10, ms.max()))
    nz = np.flatnonzero(db > -TOP_DB)
    if nz.size == 0:
        return 0, 0
    return int(nz[0] * TRIM_HOP), int(min(len(y), (nz[-1] + 1) * TRIM_HOP))


def features(y, max_len=MAXIMUM_AUDIO_LENGTH):
    """-> (log mel (80, F), log |stft| (1025, F), (start, end)) in fp64, chronological, F = 1 + max_len / 300; (None, None,
    (start, end)) when the trimmed wave is longer than max_len."""
    y = np.asarray(y, dtype=np.float64)
    start, end = trim_bounds(y)
    w = y[start:end]
    if len(w) > max_len:
        return None, None, (start, end)
    w = np.pad(w, (0, max_len - len(w)))
    e = np.append(w[0], w[1:] - 0.97 * w[:-1])
    S = gl.stft(e)                                      # (1025, F) complex
    mel = mel_basis().astype(np.float64) @ S            # melspectrogram(S=stft): the complex bins, sr = 22050
    return np.log(np.abs(mel) + 1e-8), np.log(np.abs(S) + 1e-8), (start, end)


def process_audio(y, r, max_len=MAXIMUM_AUDIO_LENGTH):
    """-> (mel (Td, 80 r), stft (Td, 1025 r), (start, end)) in fp64, or (None, None, (start, end)) when dropped."""
    mel, stft, b = features(y, max_len)
    if mel is None:
        return None, None, b
    return reshape_frames(mel, r), reshape_frames(stft, r), b
