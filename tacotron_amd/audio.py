"""r-frame layout of the reference's spectrogram tensors (audio.reshape_frames, audio.py:23-35) -- SURVEY §8f row 1 -- and
the host side of the feature front end (audio.process_audio, audio.py:38-65): the mel filterbank, WAV reading and the batch call
of the HIP feature kernel (csrc/features.hip).

The decoder emits r non-overlapping frames per step; the reference stores frames so that row `4c + j` of the
(steps, r*C) matrix holds frames `4rc + 4i + j` for i = 0..r-1 (C features each).  Written here as plain index
arithmetic (no split/concatenate chains); checked against vectors produced by the reference function itself
(tests/golden/reshape_frames.npz)."""
from __future__ import annotations

import wave as _wave

import numpy as np

MAXIMUM_AUDIO_LENGTH = 108000   # audio.maximum_audio_length (audio.py:13)


def reshape_frames(signal, r, forward=True):
    signal = np.asarray(signal)
    if forward:
        C, T = signal.shape
        nch = T // (4 * r)                                  # only full chunks of 4r frames are kept
        x = signal[:, :nch * 4 * r].reshape(C, nch, r, 4)   # [ch, c, i, j] = signal[ch, 4rc + 4i + j]
        return x.transpose(1, 3, 2, 0).reshape(nch * 4, r * C)   # [4c + j, iC + ch]
    N, RC = signal.shape
    C = RC // r
    nch = N // 4
    x = signal[:nch * 4].reshape(nch, 4, r, C)              # [c, j, i, ch]
    return x.transpose(0, 2, 1, 3).reshape(nch * 4 * r, C)  # row 4rc + 4i + j


def denormalize(output, stft_mean, stft_std):
    """test.py:64 / train.py:94-95: out * stft_std + stft_mean."""
    return output * stft_std + stft_mean


def _hz_to_mel(f):
    """Slaney mel scale (librosa.core.hz_to_mel, htk=False): linear below 1 kHz (200/3 Hz per mel), logarithmic above."""
    f = np.asarray(f, dtype=np.float64)
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, min_log_hz) / min_log_hz) / logstep, f / f_sp)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def mel_basis(sr=22050, n_fft=2048, n_mels=80, fmin=0.0, fmax=None):
    """librosa.filters.mel(sr, n_fft, n_mels) with its defaults htk=False, norm=1, restated after librosa 0.6: triangles between
    n_mels + 2 points equally spaced on the Slaney mel scale from fmin to fmax (default sr / 2), evaluated at the n_fft / 2 + 1
    bin frequencies, each scaled by 2 / (f[i + 2] - f[i]) so that its area in Hz is 1.  Computed in fp64, returned as fp32
    (n_mels, 1 + n_fft / 2).  The reference calls melspectrogram(S=stft, n_mels=80) without sr, so the default 22050 applies
    whatever the corpus rate.  Parity with librosa is UNPINNED (librosa is not a dependency and the reference pins no release)."""
    fmax = float(sr) / 2 if fmax is None else float(fmax)
    fftfreqs = np.linspace(0, float(sr) / 2, 1 + n_fft // 2, endpoint=True)
    mel_f = _mel_to_hz(np.linspace(_hz_to_mel(fmin), _hz_to_mel(fmax), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = np.subtract.outer(mel_f, fftfreqs)
    weights = np.zeros((n_mels, 1 + n_fft // 2))
    for i in range(n_mels):
        lower = -ramps[i] / fdiff[i]
        upper = ramps[i + 2] / fdiff[i + 1]
        weights[i] = np.maximum(0, np.minimum(lower, upper))
    weights *= (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]
    return weights.astype(np.float32)


def load_wav(path, sr):
    """The role of librosa.load(path, mono=True, sr=sr) (audio.py:39) for PCM WAV files, on the standard library's `wave`:
    8-bit (unsigned) and 16 / 24 / 32-bit (signed) samples are scaled like librosa's util.buf_to_float (by 2^-(bits - 1)),
    channels are averaged, the result is fp32.  A file whose rate differs from `sr` is resampled with
    scipy.signal.resample_poly -- a DEVIATION: librosa resampled with resampy's 'kaiser_best' filter.  Among the reference's corpora
    only VCTK (48 kHz files read at sr=24000, preprocess.py:217) is resampled."""
    with _wave.open(str(path), 'rb') as f:
        ch, width, rate, n = f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()
        raw = f.readframes(n)
    if width == 1:
        x = (np.frombuffer(raw, np.uint8).astype(np.float32) - 128.0) / 128.0
    elif width == 3:
        b = np.frombuffer(raw, np.uint8).reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        v = np.where(v >= 1 << 23, v - (1 << 24), v)
        x = v.astype(np.float32) * np.float32(1.0 / (1 << 23))
    elif width in (2, 4):
        x = np.frombuffer(raw, '<i%d' % width).astype(np.float32) * np.float32(1.0 / (1 << (8 * width - 1)))
    else:
        raise ValueError('%s: %d-byte samples are not PCM 8/16/24/32' % (path, width))
    x = x.reshape(-1, ch).mean(axis=1, dtype=np.float32) if ch > 1 else x
    if rate != sr:
        try:
            from scipy.signal import resample_poly
        except ImportError as e:
            raise ImportError('%s is %d Hz, %d Hz requested: resampling needs scipy (scipy.signal.resample_poly)' %
                              (path, rate, sr)) from e
        g = np.gcd(int(rate), int(sr))
        x = resample_poly(x.astype(np.float64), int(sr) // g, int(rate) // g).astype(np.float32)
    return np.ascontiguousarray(x, dtype=np.float32)


_MEL_DEVICE = {}


def process_audio(waves, lengths, r, max_len=MAXIMUM_AUDIO_LENGTH, dtype=None, out=None, work=None):
    """audio.process_audio (audio.py:38-65) for a batch, on the GPU (csrc/features.hip): trim, drop the utterances longer than
    max_len after trimming, zero-pad the others to max_len, pre-emphasis, STFT, complex mel, log, r-frame layout.
    waves: (B, L) fp32 device tensor (row b valid up to lengths[b]) or a list of 1-D arrays; lengths: host ints (None with a list:
    the arrays' lengths).  Returns device tensors (mel (B, Td, 80 r), stft (B, Td, 1025 r), kept (B) int32, bounds (B, 2) int32
    trim [start, end)), mel / stft in `dtype` (default float16, what preprocess.py stores; or float32).  Dropped rows are zero.
    out / work: the caller's own (mel, stft, kept, bounds) buffers and workspace, as lib.audio_features takes them."""
    import torch

    from . import lib
    dtype = torch.float16 if dtype is None else dtype
    if not isinstance(waves, torch.Tensor):
        lengths = [len(w) for w in waves] if lengths is None else list(lengths)
        host = np.zeros((len(waves), max(1, max(lengths))), dtype=np.float32)
        for i, w in enumerate(waves):
            host[i, :lengths[i]] = np.asarray(w, dtype=np.float32)[:lengths[i]]
        waves = torch.from_numpy(host).to('cuda', non_blocking=False)
    if waves.dtype != torch.float32 or not waves.is_cuda or waves.dim() != 2:
        raise ValueError('process_audio: waves must be a (B, L) float32 device tensor')
    if lengths is None:
        lengths = [waves.shape[1]] * waves.shape[0]
    dev = waves.device
    if dev.index not in _MEL_DEVICE:   # (a blocking upload from pageable memory: complete before any stream uses it)
        _MEL_DEVICE[dev.index] = torch.from_numpy(mel_basis()).to(dev)
    return lib.audio_features(waves.contiguous(), lengths, _MEL_DEVICE[dev.index], r, max_len, dtype, out=out, work=work)
