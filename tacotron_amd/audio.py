"""r-frame layout of the reference's spectrogram tensors (audio.reshape_frames, audio.py:23-35) -- SURVEY §8f row 1 -- and
the host side of the feature front end (audio.process_audio, audio.py:38-65): the mel filterbank, WAV reading (on the host:
load_wav; on the device: read_wav_raw / load_batch_device with resampy's kaiser_best filter as a polyphase table) and the batch
call of the HIP feature kernel (csrc/features.hip).

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


# ---- the device path: raw PCM bytes to the GPU, decode and resampling there (csrc/features.hip, taco_wave_resample) ------------
# resampy's 'kaiser_best' filter design, restated from its documentation: 64 zero crossings, 2^9 table entries per crossing, a Kaiser
# window with this beta, the sinc stretched by this rolloff.  UNVERIFIED offline, like the TF-1.2 semantics of SURVEY §8c: neither
# resampy nor librosa is a dependency, so the four numbers could not be compared with resampy's stored filter; a run next to
# resampy.filters.get_filter('kaiser_best') would falsify them (its half window should equal _kaiser_best_window()).
KAISER_BEST = {'num_zeros': 64, 'precision': 9, 'beta': 14.769656459379492, 'rolloff': 0.9475937167399596}

_KAISER_BEST_WINDOW = []


def _kaiser_best_window():
    """The right half of the interpolation window, fp64, num_zeros * 2^precision + 1 = 32769 entries (resampy.filters.sinc_window)."""
    if not _KAISER_BEST_WINDOW:
        num_table = 1 << KAISER_BEST['precision']
        n = num_table * KAISER_BEST['num_zeros']
        rolloff = KAISER_BEST['rolloff']
        sinc_win = rolloff * np.sinc(rolloff * np.linspace(0, KAISER_BEST['num_zeros'], num=n + 1, endpoint=True))
        _KAISER_BEST_WINDOW.append(np.kaiser(2 * n + 1, KAISER_BEST['beta'])[n:] * sinc_win)
    return _KAISER_BEST_WINDOW[0]


def resample_filter(sr_orig, sr_new):
    """resampy.resample(x, sr_orig, sr_new, filter='kaiser_best') as a polyphase table.  With g = gcd, P = sr_orig / g, Q = sr_new / g
    output t sits at input position t P / Q: nn = (t P) // Q and the fraction (t P) % Q / Q takes only Q values, so resampy's
    interpolated window (win[off + i step] + eta delta[off + i step], step = int(min(1, ratio) 2^precision) -- truncated, resampy's
    rule) is evaluated here once per phase, in fp64.  -> (P, Q, n_left, n_right, table (Q, n_left + n_right) fp64): entries
    [0, n_left) of row p multiply x[nn], x[nn - 1], ..., entries [n_left, n_left + n_right) multiply x[nn + 1], x[nn + 2], ...; a phase
    with fewer taps than the longest is zero-padded.  resampy clips both sums at the ends of the signal, which is the same as x = 0
    outside it."""
    sr_orig, sr_new = int(sr_orig), int(sr_new)
    if sr_orig < 1 or sr_new < 1:
        raise ValueError('resample_filter: rates must be positive, got %d and %d' % (sr_orig, sr_new))
    g = int(np.gcd(sr_orig, sr_new))
    P, Q = sr_orig // g, sr_new // g
    num_table = 1 << KAISER_BEST['precision']
    ratio = float(sr_new) / sr_orig
    win = _kaiser_best_window()
    if ratio < 1:
        win = win * ratio
    delta = np.zeros_like(win)
    delta[:-1] = np.diff(win)
    scale = min(1.0, ratio)
    step = int(scale * num_table)
    wings = []
    for p in range(Q):
        frac = scale * (float(p) / Q)
        row = []
        for fr in (frac, scale - frac):
            f = fr * num_table
            off = int(f)
            idx = off + step * np.arange((len(win) - off) // step)
            row.append(win[idx] + (f - off) * delta[idx])
        wings.append(row)
    n_left, n_right = max(len(w[0]) for w in wings), max(len(w[1]) for w in wings)
    table = np.zeros((Q, n_left + n_right))
    for p, (left, right) in enumerate(wings):
        table[p, :len(left)] = left
        table[p, n_left:n_left + len(right)] = right
    return P, Q, n_left, n_right, table


def resample_lengths(n, sr_orig, sr_new):
    """(n_calc, n_len) of a file of n frames: resampy computes int(n ratio) samples, librosa.resample(fix=True) returns
    int(ceil(n ratio)) -- the at most one sample in between is zero.  ratio is the Python float sr_new / sr_orig, as librosa forms it."""
    ratio = float(sr_new) / sr_orig
    return int(n * ratio), int(np.ceil(n * ratio))


def read_wav_raw(path):
    """A PCM WAV file without decoding it -> (the data chunk's bytes as a uint8 array, channels, bytes per sample, rate, frames)."""
    with _wave.open(str(path), 'rb') as f:
        ch, width, rate, n = f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()
        raw = f.readframes(n)
    if width not in (1, 2, 3, 4):
        raise ValueError('%s: %d-byte samples are not PCM 8/16/24/32' % (path, width))
    raw = np.frombuffer(raw, np.uint8)
    return raw, ch, width, rate, len(raw) // (ch * width)


_TAPS_DEVICE = {}


def load_batch_device(files_or_raw, sr, device='cuda'):
    """librosa.load(path, mono=True, sr=sr) for a batch, from the files' bytes on: decode, mono mix-down and kaiser_best resampling
    on the GPU (lib.wave_resample).  files_or_raw: paths, or what read_wav_raw returned for them.  Rows of one (width, channels,
    rate) share a kernel call (a corpus is uniform: one call).  -> (waves (B, L) fp32 device tensor, lengths): row b holds its
    lengths[b] samples -- at least 1 for a file that is not empty -- and zeros behind; L = max(1, max(lengths))."""
    import torch

    from . import lib
    dev = torch.device(device)
    raws = [r if isinstance(r, tuple) else read_wav_raw(r) for r in files_or_raw]
    if not raws:
        raise ValueError('load_batch_device: no files')
    counts = [resample_lengths(r[4], r[3], sr) for r in raws]
    lengths = [c[1] for c in counts]
    L = max(1, max(lengths))
    groups = {}
    for i, (_, ch, width, rate, _) in enumerate(raws):
        groups.setdefault((width, ch, rate), []).append(i)
    waves = torch.empty(len(raws), L, dtype=torch.float32, device=dev)
    for (width, ch, rate), idx in groups.items():
        key = (rate, int(sr), dev.index if dev.index is not None else torch.cuda.current_device())
        if key not in _TAPS_DEVICE:   # (a blocking upload from pageable memory: complete before any stream uses it)
            P, Q, n_left, n_right, table = resample_filter(rate, sr)
            _TAPS_DEVICE[key] = (P, Q, n_left, n_right, torch.from_numpy(table.astype(np.float32)).to(dev))
        P, Q, n_left, n_right, taps = _TAPS_DEVICE[key]
        fb = width * ch
        host = np.zeros((len(idx), max(1, max(raws[i][4] for i in idx)) * fb), dtype=np.uint8)
        for k, i in enumerate(idx):
            host[k, :raws[i][4] * fb] = raws[i][0][:raws[i][4] * fb]
        pcm = torch.from_numpy(host).to(dev)
        rows = torch.tensor([[raws[i][4], counts[i][0]] for i in idx], dtype=torch.int32).to(dev)
        if len(groups) == 1:
            lib.wave_resample(pcm, rows, taps, width, ch, P, Q, n_left, n_right, out=waves)
        else:
            waves[torch.tensor(idx, device=dev)] = lib.wave_resample(pcm, rows, taps, width, ch, P, Q, n_left, n_right, L=L)
    return waves, lengths


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
