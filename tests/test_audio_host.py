"""Host side of the feature front end (no GPU): audio.mel_basis, audio.load_wav, the corpus listing functions of
tacotron_amd.preprocess, the C ABI's argument checks of taco_audio_features, and the trim of the NumPy reference
(tests/audio_ref.py) on signals with hand-derived bounds."""
import ctypes as C
import math
import wave

import numpy as np
import pytest

from tacotron_amd import audio, preprocess
from tests import audio_ref

SR, NFFT = 22050, 2048
F_SP, LOGSTEP = 200.0 / 3, math.log(6.4) / 27.0


def _mel_to_hz(m):   # Slaney: linear below mel 15 (= 1000 Hz), logarithmic above
    return F_SP * m if m < 15 else 1000.0 * math.exp(LOGSTEP * (m - 15))


def _edges():
    top = 15 + math.log(11025 / 1000.0) / LOGSTEP
    return [_mel_to_hz(top * i / 81) for i in range(82)]


def test_mel_basis_shape_and_edges():
    M = audio.mel_basis()
    assert M.shape == (80, 1025) and M.dtype == np.float32
    f = _edges()
    assert f[0] == 0 and abs(f[-1] - 11025) < 1e-6
    freqs = np.arange(1025) * SR / NFFT
    for i in range(80):
        inside = (freqs > f[i] + 1e-6) & (freqs < f[i + 2] - 1e-6)
        assert np.all(M[i][~inside] == 0), 'row %d nonzero outside (%.2f, %.2f) Hz' % (i, f[i], f[i + 2])
        assert np.all(M[i][inside] > 0)
        peak = freqs[np.argmax(M[i])]   # the apex sits at the middle point, within one bin
        assert abs(peak - f[i + 1]) <= SR / NFFT


def test_mel_basis_hand_entries():
    M = audio.mel_basis().astype(np.float64)
    f = _edges()
    step = f[1]                                    # below 1 kHz the points are equally spaced: f[i] = i * step
    assert abs(f[2] - 2 * step) < 1e-9
    apex = lambda i: int(round(f[i + 1] * NFFT / SR))   # noqa: E731  (the bin nearest the middle point)
    for i, k in ((0, 1), (0, 3), (1, 5), (40, apex(40)), (40, apex(40) + 3), (79, apex(79)), (79, apex(79) - 20)):
        fk = k * SR / NFFT
        w = max(0.0, min((fk - f[i]) / (f[i + 1] - f[i]), (f[i + 2] - fk) / (f[i + 2] - f[i + 1]))) * 2 / (f[i + 2] - f[i])
        assert w > 0
        assert abs(M[i, k] - w) <= 1e-6 * w, (i, k, M[i, k], w)
    # bin 1 of filter 0 (10.77 Hz on the rising edge of the 0 .. 2 step triangle): (10.77 / step) * 2 / (2 step)
    assert abs(M[0, 1] - (SR / NFFT / step) / step) <= 1e-6 * M[0, 1]


def test_mel_basis_unit_area():
    M = audio.mel_basis().astype(np.float64)
    area = M.sum(1) * SR / NFFT
    assert np.all(np.abs(area[1:-1] - 1) < 0.015), area


def _write_wav(path, data, width, rate=16000):
    data = np.asarray(data)
    ch = 1 if data.ndim == 1 else data.shape[1]
    with wave.open(str(path), 'wb') as f:
        f.setnchannels(ch)
        f.setsampwidth(width)
        f.setframerate(rate)
        if width == 3:
            v = data.reshape(-1).astype(np.int32) & 0xFFFFFF
            raw = np.stack([v & 0xFF, (v >> 8) & 0xFF, (v >> 16) & 0xFF], 1).astype(np.uint8).tobytes()
        else:
            raw = data.astype('<i%d' % width).tobytes()
        f.writeframes(raw)


def test_load_wav_pcm16_mono_stereo(tmp_path):
    rng = np.random.default_rng(0)
    x = rng.integers(-32768, 32768, size=1000)
    _write_wav(tmp_path / 'm.wav', x, 2)
    y = audio.load_wav(tmp_path / 'm.wav', 16000)
    assert y.dtype == np.float32 and np.array_equal(y, (x / 32768.0).astype(np.float32))
    s = rng.integers(-32768, 32768, size=(500, 2))
    _write_wav(tmp_path / 's.wav', s, 2)
    y = audio.load_wav(tmp_path / 's.wav', 16000)
    assert y.shape == (500,)
    np.testing.assert_allclose(y, s.mean(1) / 32768.0, rtol=0, atol=1e-7)


def test_load_wav_pcm24(tmp_path):
    x = np.array([0, 1, -1, (1 << 23) - 1, -(1 << 23), 123456, -654321])
    _write_wav(tmp_path / 'a.wav', x, 3)
    y = audio.load_wav(tmp_path / 'a.wav', 16000)
    np.testing.assert_array_equal(y, (x / float(1 << 23)).astype(np.float32))


def test_load_wav_resamples(tmp_path):
    pytest.importorskip('scipy')
    t = np.arange(4800) / 48000.0
    _write_wav(tmp_path / 'r.wav', np.round(8000 * np.sin(2 * np.pi * 440 * t)), 2, rate=48000)
    y = audio.load_wav(tmp_path / 'r.wav', 24000)
    assert y.shape == (2400,)
    ref = 8000 / 32768.0 * np.sin(2 * np.pi * 440 * np.arange(2400) / 24000.0)
    assert np.abs(y[100:-100] - ref[100:-100]).max() < 2e-3


def test_prepare_nancy(tmp_path):
    d = tmp_path / 'nancy'
    d.mkdir()
    (d / 'prompts.data').write_text('( nancy001 "Hello there." )\n( nancy002 "A \\"quoted\\" word!" )\n')
    out = preprocess.prepare_nancy(str(tmp_path))
    assert out['prompts'] == ['Hello there', 'A \\"quoted\\" word']   # rfind('"') - 1 drops the last character
    assert out['audio_files'] == [str(d / 'wavn' / 'nancy001.wav'), str(d / 'wavn' / 'nancy002.wav')]


def test_prepare_arctic(tmp_path):
    d = tmp_path / 'arctic' / 'etc'
    d.mkdir(parents=True)
    (d / 'arctic.data').write_text('( arctic_a0001 "Author of the danger trail, Philip Steels, etc." )\n'
                                   '( arctic_b0002 "Yes." )\n')
    out = preprocess.prepare_arctic(str(tmp_path))
    assert out['prompts'] == ['Author of the danger trail, Philip Steels, etc.', 'Yes.']
    w = tmp_path / 'arctic' / 'wav'
    assert out['audio_files'] == [str(w / 'arctic_a0001.wav'), str(w / 'arctic_b0002.wav')]


def test_prepare_vctk(tmp_path):
    v = tmp_path / 'vctk'
    v.mkdir()
    (v / 'speaker-info.txt').write_text('ID  AGE  GENDER  ACCENTS  REGION\n'
                                        '226  22  M    English    Surrey\n'
                                        '225  23  F    English    Southern  England\n')
    for spk, utts in (('p225', {'p225_002': ' Second. \n', 'p225_001': 'Please call Stella.\n'}), ('p226', {'p226_001': 'Ask her.'})):
        (v / 'txt' / spk).mkdir(parents=True)
        for u, t in utts.items():
            (v / 'txt' / spk / (u + '.txt')).write_text(t)
    out = preprocess.prepare_vctk(str(tmp_path))
    # speaker ids in speaker-info order (226 -> 0, 225 -> 1); utterances per speaker sorted by file name
    assert out['prompts'] == ['Ask her.', 'Please call Stella.', 'Second.']
    assert out['speakers'] == [0, 1, 1]
    assert out['audio_files'] == [str(v / 'wav48' / 'p226' / 'p226_001.wav'), str(v / 'wav48' / 'p225' / 'p225_001.wav'),
                                  str(v / 'wav48' / 'p225' / 'p225_002.wav')]


def test_truncate_npy(tmp_path):
    p = str(tmp_path / 'a.npy')
    m = np.lib.format.open_memmap(p, 'w+', np.float16, (1000, 3, 5))
    m[:] = np.arange(15000, dtype=np.float16).reshape(1000, 3, 5)
    m.flush()
    del m
    preprocess._truncate_npy(p, 7)
    a = np.load(p)
    assert a.shape == (7, 3, 5)
    np.testing.assert_array_equal(a, np.arange(15000, dtype=np.float16).reshape(1000, 3, 5)[:7])


def test_reader_threads(monkeypatch):
    monkeypatch.setenv('OMP_NUM_THREADS', '4')
    assert preprocess._reader_threads() == 4
    monkeypatch.setenv('OMP_NUM_THREADS', '256')
    assert preprocess._reader_threads() == 16


def test_audio_features_workspace_and_validation(built_lib):
    lib = built_lib
    assert lib.audio_features_workspace_bytes(4, 200000) > 4 * (1 + 200000 // 512) * 4
    for B, L in ((0, 100), (3, 0), (-1, 5)):
        with pytest.raises(lib.TacoError):
            lib.audio_features_workspace_bytes(B, L)
    fake = C.c_void_p(256)   # never dereferenced: every case below is rejected before anything is enqueued

    def call(lens, L=2000, max_len=108000, r=2, fp16=1, B=None, null=False):
        arr = (C.c_int32 * len(lens))(*lens)
        return lib._lib.taco_audio_features(None if null else fake, arr, fake, fake, fake, fake, fake, fake,
                                            len(lens) if B is None else B, L, max_len, r, fp16, None)

    cases = [dict(lens=[100], r=0), dict(lens=[100], r=6), dict(lens=[100], max_len=108001), dict(lens=[100], max_len=0),
             dict(lens=[100], max_len=900), dict(lens=[100, 2001]), dict(lens=[0]), dict(lens=[100], fp16=2),
             dict(lens=[100], null=True), dict(lens=[100], B=0), dict(lens=[100], max_len=3000, r=3)]
    for kw in cases:
        rc = call(**kw)
        assert rc == -1, kw   # TACO_EINVAL
        assert 'audio_features' in lib.last_error()


def _tone(n, amp=0.5, f0=220.0, sr=16000):
    return amp * np.sin(2 * np.pi * f0 * np.arange(n) / sr)


def test_reference_trim_bounds():
    # silence of 5 * 512 + 100 samples, 20000 samples of tone, 6000 of silence: the frames whose 2048-sample window (centred on
    # 512 t) touches the tone are within ~25 dB of the maximum; the others are exactly 0 -> -100 dB relative
    lead, body, tail = 5 * 512 + 100, 20000, 6000
    y = np.concatenate([np.zeros(lead), _tone(body), np.zeros(tail)])
    # frame t covers samples [512 t - 1024, 512 t + 1024): first touching frame t with 512 t + 1024 > lead -> t = 4;
    # last: 512 t - 1024 < lead + body -> t = 46 (512 * 46 - 1024 = 22528 < 22660); end = 512 * 47
    assert audio_ref.trim_bounds(y) == (4 * 512, 47 * 512)
    assert audio_ref.trim_bounds(np.zeros(5000)) == (0, 5000)   # all-zero: every frame 0 dB, nothing trimmed
    z = _tone(3000)
    assert audio_ref.trim_bounds(z) == (0, 3000)                 # end clipped to the length
    short = np.concatenate([_tone(600), np.zeros(20000)])
    assert audio_ref.trim_bounds(short) == (0, 512 * 4)          # last touching frame: 512 t - 1024 < 600 -> t = 3


def test_reference_process_audio_shapes():
    mel, stft, b = audio_ref.process_audio(_tone(5000), 2)
    assert mel.shape == (180, 160) and stft.shape == (180, 2050) and b == (0, 5000)
    mel, stft, b = audio_ref.process_audio(_tone(109000), 2)
    assert mel is None and stft is None
