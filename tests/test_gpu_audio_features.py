"""GPU: the feature front end (csrc/features.hip, audio.process_audio, tacotron_amd.preprocess) against the fp64 NumPy
restatement of audio.process_audio (tests/audio_ref.py; PARITY WITH LIBROSA UNPINNED: librosa is not available here).

Features are compared in the linear domain, frame by frame: |exp(gpu) - exp(ref)| <= 1e-5 * max(exp(ref)) over the frame, and
on the bins at least 1e-3 of the frame maximum the log difference is <= 2e-3.  Trim bounds and keep flags are exact (the
signals keep every trim frame far from the -60 dB threshold, checked below).

Outputs and workspace of the feature kernel (and of taco_denorm_unframe / Griffin-Lim in the round trip) are the tests' own
buffers from a guarded arena (tests/poison.py), poisoned before the call -- `ones` for mel / stft (every byte differs from a
written zero, in fp16 too) and for the int32 bounds / kept, NaN for the workspace: afterwards every output element is written
(rows of dropped utterances as zeros) and the guard bands are intact."""
import os
import pickle as pkl
import wave

import numpy as np
import pytest
import torch

from oracle import griffinlim_numpy as gl
from oracle import taco_numpy as on
from tacotron_amd import audio
from tacotron_amd.audio import reshape_frames
from tests import audio_ref
from tests.poison import Guarded

pytestmark = pytest.mark.gpu

MAX_LEN = 108000
LOG_EPS32 = np.float32(np.log(np.float32(1e-8)))


def _voice(n, seed, f0=140.0, sr=16000, amp=1.0):
    """A harmonic tone with a little noise: broadband, and every trim frame inside it within ~10 dB of the loudest."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    y = sum(0.3 / k * np.sin(2 * np.pi * k * f0 * t + rng.uniform(0, 2 * np.pi)) for k in range(1, 21))
    return (amp * (y + 0.02 * rng.standard_normal(n))).astype(np.float32)


def _signals():
    z = lambda n: np.zeros(n, np.float32)   # noqa: E731
    return [
        _voice(40000, 1),                                          # shorter than max_len
        _voice(MAX_LEN, 2),                                        # exactly max_len, nothing to trim
        _voice(120000, 3),                                         # longer than max_len: dropped
        np.concatenate([z(3000), _voice(30000, 4), z(7000)]),      # leading and trailing silence
        z(50000),                                                  # all zero: kept, not trimmed
        _voice(70000, 5, amp=0.1),
        np.concatenate([z(10000), _voice(20000, 6, f0=210.0), z(2000)]),
    ]


_REF = {}


def _ref(i):
    if i not in _REF:
        y = _signals()[i]
        ms = audio_ref.frame_ms(y)
        if ms.max() > 0:   # the designed margin: no trim frame within 5 dB of the -60 dB threshold
            db = 10 * np.log10(np.maximum(1e-10, ms)) - 10 * np.log10(ms.max())
            assert not np.any((db > -65) & (db < -55)), 'signal %d has a trim frame near -60 dB' % i
        _REF[i] = audio_ref.features(y, MAX_LEN)
    return _REF[i]


def _run(idx, r, dtype=torch.float32):
    from tacotron_amd import lib
    sig = _signals()
    waves = [sig[i] for i in idx]
    B, L = len(waves), max(len(w) for w in waves)
    Td = ((1 + MAX_LEN // 300) // (4 * r)) * 4
    G = Guarded({'mel': ((B, Td, 80 * r), dtype, 'ones'), 'stft': ((B, Td, 1025 * r), dtype, 'ones'),
                 'kept': ((B,), torch.int32, 'ones'), 'bounds': ((B, 2), torch.int32, 'ones'),
                 'work': ((lib.audio_features_workspace_bytes(B, L),), torch.uint8, 'qnan')})
    res = audio.process_audio(waves, None, r, MAX_LEN, dtype, out=(G['mel'], G['stft'], G['kept'], G['bounds']), work=G['work'])
    torch.cuda.synchronize()
    G.check('mel', 'stft', 'kept', 'bounds')
    assert all(a.data_ptr() == G[k].data_ptr() for a, k in zip(res, ('mel', 'stft', 'kept', 'bounds')))
    return res


def _check_features(gpu_log, ref_log, what):
    """gpu_log, ref_log: (frames, C) chronological."""
    g, rf = np.exp(gpu_log.astype(np.float64)), np.exp(ref_log)
    fmax = rf.max(axis=1, keepdims=True)
    err = np.abs(g - rf) / fmax
    assert err.max() <= 1e-5, '%s: linear error %.2e of the frame maximum (frame %d)' % (what, err.max(), err.max(1).argmax())
    big = rf >= 1e-3 * fmax
    dl = np.abs(gpu_log.astype(np.float64) - ref_log)[big]
    assert dl.max() <= 2e-3, '%s: log error %.2e on bins >= 1e-3 of the frame maximum' % (what, dl.max())


@pytest.mark.parametrize('r', [1, 2, 3, 4, 5])
@pytest.mark.parametrize('idx', [[3], list(range(7))], ids=['B1', 'B7'])
def test_features_match_reference(built_lib, r, idx):
    mel, stft, kept, bounds = _run(idx, r)
    torch.cuda.synchronize()
    F = 1 + MAX_LEN // 300
    Td = (F // (4 * r)) * 4
    Fk = Td * r
    assert mel.shape == (len(idx), Td, 80 * r) and stft.shape == (len(idx), Td, 1025 * r)
    mel, stft, kept, bounds = (t.cpu().numpy() for t in (mel, stft, kept, bounds))
    for b, i in enumerate(idx):
        ref_mel, ref_stft, (s, e) = _ref(i)
        assert (int(bounds[b, 0]), int(bounds[b, 1])) == (s, e), 'signal %d: trim bounds' % i
        assert kept[b] == (ref_mel is not None), 'signal %d: kept flag' % i
        if ref_mel is None:
            assert not mel[b].any() and not stft[b].any(), 'dropped row %d is not zero' % b
            continue
        g_stft = reshape_frames(stft[b], r, forward=False)   # (Fk, 1025) chronological
        g_mel = reshape_frames(mel[b], r, forward=False)
        assert g_stft.shape == (Fk, 1025)
        _check_features(g_stft, ref_stft[:, :Fk].T, 'signal %d stft r=%d' % (i, r))
        _check_features(g_mel, ref_mel[:, :Fk].T, 'signal %d mel r=%d' % (i, r))
        # frames wholly in the zero padding (their input is exactly zero) are log(1e-8) to 1 ulp
        zero = np.all(ref_stft[:, :Fk] == np.log(1e-8), axis=0)
        if e - s < MAX_LEN - 1200:
            assert zero.any(), 'signal %d: expected padding frames' % i
        for name, g in (('stft', g_stft), ('mel', g_mel)):
            ulp = np.abs(g[zero].view(np.int32).astype(np.int64) - LOG_EPS32.view(np.int32))
            assert ulp.size == 0 or ulp.max() <= 1, 'signal %d %s: padding frames %d ulp from log(1e-8)' % (i, name, ulp.max())


def test_trim_bounds_and_keep_flags(built_lib):
    sig = _signals()
    _, _, kept, bounds = _run(range(7), 2)
    kept, bounds = kept.cpu().numpy(), bounds.cpu().numpy()
    expect = [audio_ref.trim_bounds(y) for y in sig]
    assert [tuple(int(v) for v in b) for b in bounds] == expect
    assert expect[3] == (2048, 34304) and expect[4] == (0, 50000) and expect[1] == (0, MAX_LEN)
    assert kept.tolist() == [1, 1, 0, 1, 1, 1, 1]


def test_fp16_is_rounded_fp32_and_reproducible(built_lib):
    idx = list(range(7))
    m32, s32, _, _ = _run(idx, 2, torch.float32)
    m32b, s32b, _, _ = _run(idx, 2, torch.float32)
    m16, s16, _, _ = _run(idx, 2, torch.float16)
    assert torch.equal(m32, m32b) and torch.equal(s32, s32b), 'two calls differ'
    for a16, a32 in ((m16, m32), (s16, s32)):
        np.testing.assert_array_equal(a16.cpu().numpy().view(np.uint16), a32.cpu().numpy().astype(np.float16).view(np.uint16))


def test_round_trip_through_griffinlim(built_lib):
    lib = built_lib
    r = 2
    _, stft, _, _ = _run([0], r)
    RC = stft.shape[2]
    F = (stft.shape[1] // 4) * 4 * r
    G = Guarded({'mag_t': ((1, 1025, F), torch.float32, 'qnan'), 'wave': ((1, 300 * (F - 1)), torch.float32, 'qnan'),
                 'work': ((lib.griffinlim_workspace_floats(1, F),), torch.float32, 'qnan')})
    mag_t = lib.denorm_unframe(stft.contiguous(), torch.zeros(RC, device='cuda'), torch.ones(RC, device='cuda'), r,
                               want_spec=False, want_mag_t=True, mag_t=G['mag_t'])   # (1, 1025, F) = exp(log |X| + ...)
    torch.cuda.synchronize()
    G.check('mag_t')
    assert mag_t.shape[2] == F
    ph = torch.as_tensor(2 * np.pi * np.random.default_rng(7).random((1, 1025, F)), dtype=torch.float32, device='cuda')
    mag = mag_t[0].double().cpu().numpy()
    w0 = lib.griffinlim(mag_t, ph, 0, out=G['wave'], work=G['work'])[0].double().cpu().numpy()
    G.check('wave')
    G.refill('wave', 'work')
    w50 = lib.griffinlim(mag_t, ph, 50, out=G['wave'], work=G['work'])[0].double().cpu().numpy()
    G.check('wave')
    sc0, sc50 = gl.spectral_convergence(w0, mag), gl.spectral_convergence(w50, mag)
    print('  spectral convergence %.4f -> %.4f after 50 rounds' % (sc0, sc50))
    assert sc50 < 0.5 * sc0


def _write_wav16(path, y, sr=16000):
    with wave.open(str(path), 'wb') as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(sr)
        f.writeframes(np.clip(np.round(y * 32767), -32768, 32767).astype('<i2').tobytes())


def _write_nancy(tmp_path):
    """Six utterances in the Blizzard Nancy layout (prompts.data + wavn/); the third is longer than max_len and is dropped."""
    lines = ['Hello world.', 'The quick brown fox!', 'Too long to keep.', 'Jumps over.', 'A lazy dog?', 'Zebra quartz.']
    lens = [30000, 45000, 130000, 20000, 60000, 36000]
    wav_dir = tmp_path / 'nancy' / 'wavn'
    wav_dir.mkdir(parents=True)
    with open(tmp_path / 'nancy' / 'prompts.data', 'w') as f:
        for i, (text, n) in enumerate(zip(lines, lens)):
            f.write('( nancy%03d "%s" )\n' % (i + 1, text))
            _write_wav16(wav_dir / ('nancy%03d.wav' % (i + 1)), 0.8 * _voice(n, 20 + i, f0=120.0 + 15 * i))
    return lines, wav_dir


def test_preprocess_nancy_end_to_end(built_lib, tmp_path):
    from tacotron_amd import preprocess, train
    from tacotron_amd.config import Config
    from tacotron_amd.data import Vocab
    from tacotron_amd.model import Tacotron

    lines, wav_dir = _write_nancy(tmp_path)
    count = preprocess.main(['nancy', '--data-dir', str(tmp_path)])
    assert count == 5
    out = str(tmp_path / 'nancy')
    meta, data, _, _ = train.load_corpus(out)
    assert data['mel'].shape == (5, 180, 160) and data['stft'].shape == (5, 180, 2050)
    assert np.load(os.path.join(out, 'mels.npy')).dtype == np.float16
    assert np.load(os.path.join(out, 'speech_lens.npy')).tolist() == [180] * 5
    prompts = [t[:-1] for t in lines]               # Nancy's slice drops the character before the closing quote
    v = Vocab()
    enc = [v.encode(p) for p in prompts]            # the vocabulary grows over every prompt, the dropped one included
    assert meta['vocab'] == v.ivocab and meta['r'] == 2 and meta['sr'] == 16000
    with open(os.path.join(out, 'meta.pkl'), 'rb') as f:
        assert pkl.load(f) == meta
    kept_enc = [e for i, e in enumerate(enc) if i != 2]
    assert data['text_length'].tolist() == [len(e) for e in kept_enc]
    for row, e in zip(data['text'], kept_enc):
        assert row[:len(e)].tolist() == e and not row[len(e):].any()
    # the row of utterance 4 equals the kernel's fp16 features of the same samples
    y = audio.load_wav(wav_dir / 'nancy004.wav', 16000)
    _, s16, _, _ = audio.process_audio([y], None, 2)
    np.testing.assert_array_equal(np.load(os.path.join(out, 'stfts.npy'))[2], s16[0].cpu().numpy())
    # one train step on the corpus
    c = Config()
    c.r, c.vocab_size = meta['r'], len(meta['vocab'])
    batch = {'text': torch.from_numpy(data['text']), 'text_length': torch.from_numpy(data['text_length']),
             'mel': torch.from_numpy(np.ascontiguousarray(data['mel'], dtype=np.float32)),
             'stft': torch.from_numpy(np.ascontiguousarray(data['stft'], dtype=np.float32))}
    m = Tacotron(c, batch, train=True, seed=0)
    m.step(1e-3)
    torch.cuda.synchronize()
    loss = float(m.loss)
    print('  loss on the preprocessed corpus: %.4f' % loss)
    assert np.isfinite(loss) and loss > 0


def test_preprocess_r3_corpus_trains_like_the_oracle(built_lib, tmp_path):
    """`preprocess --r 3` -> a corpus of Td = ((1 + 108000 // 300) // 12) * 4 = 120 steps of 3 frames -> one Tacotron step on it
    (decoder.hip: decoder3 has no r = 3 instantiation) gives the fp64 oracle's loss on the same batch and masks."""
    from tacotron_amd import preprocess, train
    from tacotron_amd.config import Config
    from tacotron_amd.model import Tacotron

    _write_nancy(tmp_path)
    assert preprocess.main(['nancy', '--data-dir', str(tmp_path), '--r', '3']) == 5
    meta, data, _, _ = train.load_corpus(str(tmp_path / 'nancy'))
    assert meta['r'] == 3
    assert data['mel'].shape == (5, 120, 240) and data['stft'].shape == (5, 120, 3075)
    c = Config()
    c.r, c.vocab_size = meta['r'], len(meta['vocab'])
    assert c.max_decode_iter == 120
    inp = {'text': data['text'], 'text_length': data['text_length'],
           'mel': np.ascontiguousarray(data['mel'], dtype=np.float32), 'stft': np.ascontiguousarray(data['stft'], dtype=np.float32)}
    m = Tacotron(c, {k: torch.from_numpy(v) for k, v in inp.items()}, train=True, seed=0)
    p64 = {k: v.astype(np.float64) for k, v in m.params.to_dict().items()}
    masks = m.draw_masks()
    m.forward(masks)
    m.backward()
    torch.cuda.synchronize()
    m.check()
    assert built_lib.last_cluster(0) == 8 and built_lib.last_cluster(1) == 8   # decoder.hip
    fm = {k: v.cpu().numpy().astype(np.float64) for k, v in masks.items()}
    s2s, out, _, _ = on.forward(p64, {k: (v.astype(np.float64) if v.dtype == np.float32 else v) for k, v in inp.items()},
                                3, 120, True, fm)
    loss = on.loss_fn(s2s, out, inp['mel'].astype(np.float64), inp['stft'].astype(np.float64))
    print('  r = 3 corpus: loss hip %.6f oracle %.6f' % (float(m.loss), loss))
    assert abs(float(m.loss) - loss) <= 1e-5 * loss
