"""GPU: the pitch through the host layers -- griffinlim.invert_spectrogram(pitch=...) and the driver's `pitch` -- held bit for bit to
the same calls without a pitch (0 semitones) and to lib.frames_pitch in front of the Griffin-Lim entry points, and the acoustic check:
the fundamental of the vocoded waveform moves by the ratio asked for."""
import math
import wave as wavefile

import numpy as np
import pytest
import torch

from tests import pitch_ref as pr

pytestmark = pytest.mark.gpu

R, TD, B = 2, 8, 2
F = (TD // 4) * 4 * R          # 16 frames
LENGTHS = (8, 5)               # decoder steps -> 16 and 10 frames


def dev(x, dtype=torch.float32):
    return torch.as_tensor(np.asarray(x), dtype=dtype).cuda()


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.fixture(scope='module')
def frames():
    """(out, mean, std): a normalised model output (B, Td, 1025 r) and the statistics that de-normalise it, on the device"""
    rng = np.random.default_rng(11)
    out = rng.standard_normal((B, TD, 1025 * R)).astype(np.float32)
    mean = (rng.standard_normal(1025 * R) * 0.3 - 2.0).astype(np.float32)
    std = (0.5 + rng.random(1025 * R)).astype(np.float32)
    return dev(out), dev(mean), dev(std)


@pytest.mark.parametrize('rate', [None, 0.5], ids=['no_rate', 'rate'])
@pytest.mark.parametrize('momentum', [None, 0.99], ids=['plain', 'momentum'])
@pytest.mark.parametrize('with_lengths', [False, True], ids=['full', 'lengths'])
def test_zero_semitones_is_the_call_without_a_pitch(built_lib, frames, with_lengths, momentum, rate):
    from tacotron_amd.griffinlim import invert_spectrogram
    out, mean, std = frames
    kw = dict(n_iter=3, seed=5, lengths=dev(LENGTHS, torch.int32) if with_lengths else None, momentum=momentum, rate=rate,
              want_conv=momentum is not None)
    plain = invert_spectrogram(out, mean, std, R, **kw)
    zero = invert_spectrogram(out, mean, std, R, pitch=0.0, **kw)
    moved = invert_spectrogram(out, mean, std, R, pitch=3.0, **kw)
    torch.cuda.synchronize()
    single = rate is None and momentum is None
    plain, zero, moved = ((x,) if single else tuple(x) for x in (plain, zero, moved))
    assert len(plain) == len(zero) == len(moved) == 1 + (momentum is not None) + (rate is not None)
    for a, b in zip(plain, zero):
        assert a.dtype == b.dtype and same_bits(a, b)
    assert bool(plain[0].abs().max() > 0)
    assert moved[0].shape == plain[0].shape and not same_bits(moved[0], plain[0])     # no return shape changes; the samples do
    if rate is not None:
        assert torch.equal(moved[-1], plain[-1])                                       # frames_out: the duration is the rate's alone


def test_pitch_is_frames_pitch_in_front_of_the_vocoder(built_lib, frames):
    """one pitch per row, as semitones and as step_q on the device; with `rate` the shift runs first"""
    from tacotron_amd.griffinlim import invert_spectrogram
    lib = built_lib
    out, mean, std = frames
    lengths = dev(LENGTHS, torch.int32)
    semis = [4.0, -5.0]
    steps = [lib.pitch_step(x) for x in semis]
    assert steps == [52016, 87480]
    mag = lib.denorm_unframe(out, mean, std, R, want_spec=False, want_mag_t=True)
    shifted = lib.frames_pitch(mag, lengths, steps, frames_per_unit=R, lifter=24)
    assert not shifted[1, :, 10:].any() and bool((shifted[1, :, :10] > 0).all())
    want = lib.griffinlim_rows(shifted, lengths, seed=7, n_iter=2, frames_per_unit=R)
    got = invert_spectrogram(out, mean, std, R, n_iter=2, seed=7, lengths=lengths, pitch=semis, lifter=24)
    assert same_bits(got, want)
    got = invert_spectrogram(out, mean, std, R, n_iter=2, seed=7, lengths=lengths, pitch=dev(steps, torch.int32), lifter=24)
    assert same_bits(got, want)
    # without lengths: all F frames, and the phases of the path without lengths
    full = lib.frames_pitch(mag, None, steps, lifter=24)
    g = torch.Generator(device='cpu').manual_seed(7)
    phase0 = (2.0 * math.pi * torch.rand(mag.shape, generator=g)).cuda()
    assert same_bits(invert_spectrogram(out, mean, std, R, n_iter=2, seed=7, pitch=semis, lifter=24), lib.griffinlim(full, phase0, 2))
    # with a rate: the stretch of the shifted frames
    stretched, n = lib.frames_stretch(shifted, lengths, 32768, frames_per_unit=R, Fo=lib.stretch_capacity(F, 32768))
    want = lib.griffinlim_rows(stretched, n, seed=7, n_iter=2)
    got, n2 = invert_spectrogram(out, mean, std, R, n_iter=2, seed=7, lengths=lengths, pitch=semis, lifter=24, rate=0.5)
    assert same_bits(got, want) and n2.tolist() == n.tolist() == [31, 19]
    for bad in (dict(pitch=12.5), dict(pitch=[1.0]), dict(pitch=1.0, lifter=0), dict(pitch=1.0, lifter=65)):
        with pytest.raises(ValueError):
            invert_spectrogram(out, mean, std, R, n_iter=2, **bad)


# ---- the driver --------------------------------------------------------------------------------------------------------------------
RULE = dict(end_offset=200, hold=1, min_steps=5)   # target 0: every row stops after step 4 -> len_b = 8
PROMPTS = ['hello world.\n', 'a somewhat longer prompt, with punctuation!\n']
LONG = ('the first sentence of this prompt is long enough to fill a good part of one piece on its own, and it ends here. '
        'the second one has no full stop for a long while, only a comma after a run of words that goes on and on and on, '
        'and then more words that follow the comma until the line has well over three hundred characters in it.\n')


def _cfg(tmp_path):
    from tacotron_amd.config import Config
    c = Config()
    c.data_path = str(tmp_path / 'no_data') + '/'
    c.max_decode_iter = 16
    return c


def _wav(path):
    with wavefile.open(str(path)) as f:
        assert f.getframerate() == 16000 and f.getsampwidth() == 2 and f.getnchannels() == 1
        return f.getnframes(), f.readframes(f.getnframes())


def _read(path):
    with open(path, 'rb') as f:
        return f.read()


def test_driver_writes_the_pitch_file_and_leaves_the_rest(built_lib, tmp_path, monkeypatch):
    """test() with one pitch per prompt, a stop rule and a rate: prompt_NNN_pitch.npy = (step_q, lifter); every other file has the
    name and size of the run without a pitch, the model's own files and the rate file its bytes; the prompt at 0 semitones also its
    audio, the shifted prompt other audio; and pitch 0 for all is the run without a pitch, byte for byte"""
    from tacotron_amd import test as drv
    lib = built_lib
    seen = []
    real = lib.frames_pitch

    def spy(mag_t, frames=None, step_q=None, **k):
        seen.append((tuple(mag_t.shape), None if frames is None else frames.cpu().tolist(), step_q.cpu().tolist(), dict(k)))
        return real(mag_t, frames, step_q, **k)

    monkeypatch.setattr(lib, 'frames_pitch', spy)
    rule = lib.TacoStopRule(**RULE)
    r = _cfg(tmp_path).r
    common = dict(n_iter=2, stop=rule, rate=0.8)
    plain, shifted, zero = tmp_path / 'plain', tmp_path / 'shifted', tmp_path / 'zero'
    assert drv.test(_cfg(tmp_path), PROMPTS, out_dir=str(plain), **common) == 2
    assert not seen
    assert drv.test(_cfg(tmp_path), PROMPTS, out_dir=str(shifted), pitch=[0.0, 3.0], lifter=40, **common) == 2
    assert seen == [((2, 1025, 16 * r), [8, 8], [65536, lib.pitch_step(3.0)], dict(frames_per_unit=r, lifter=40))]
    assert drv.test(_cfg(tmp_path), PROMPTS, out_dir=str(zero), pitch=0, **common) == 2
    assert seen[1][2] == [65536, 65536] and seen[1][3]['lifter'] == 32
    names = sorted(p.name for p in plain.iterdir())
    assert names == sorted('prompt_%03d%s' % (i, s) for i in range(2) for s in ('.wav', '_spec.npy', '_align.npy', '_len.npy', '_rate.npy'))
    for run in (shifted, zero):
        assert sorted(p.name for p in run.iterdir()) == sorted(names + ['prompt_%03d_pitch.npy' % i for i in range(2)])
    for i in range(2):
        got = np.load(shifted / ('prompt_%03d_pitch.npy' % i))
        assert got.dtype == np.int32 and got.tolist() == [lib.pitch_step((0.0, 3.0)[i]), 40]
        assert np.load(zero / ('prompt_%03d_pitch.npy' % i)).tolist() == [65536, 32]
        for kind in ('spec', 'align', 'len', 'rate'):
            name = 'prompt_%03d_%s.npy' % (i, kind)
            assert _read(shifted / name) == _read(plain / name) == _read(zero / name), name
        name = 'prompt_%03d.wav' % i
        n, data = _wav(plain / name)
        assert n > 0 and any(data) and _wav(shifted / name)[0] == n
        assert _read(zero / name) == _read(plain / name)
        assert (_wav(shifted / name)[1] == data) == (i == 0)
    with pytest.raises(ValueError, match='pitch'):
        drv.test(_cfg(tmp_path), PROMPTS, out_dir=str(tmp_path / 'x'), n_iter=2, pitch=1.0, vocode=False)
    with pytest.raises(ValueError, match='pitch'):
        drv.test(_cfg(tmp_path), PROMPTS, out_dir=str(tmp_path / 'x'), n_iter=2, pitch=[1.0])


def test_driver_pieces_inherit_their_prompts_pitch(built_lib, tmp_path, monkeypatch):
    """with `long` every piece of a prompt is shifted by the prompt's pitch and writes it; without a stretch the vocoder sees all
    frames unless it is given the lengths"""
    from tacotron_amd import data, test as drv
    lib = built_lib
    K = len(data.split_prompt(LONG))
    assert K >= 3
    seen = []
    real = lib.frames_pitch

    def spy(mag_t, frames=None, step_q=None, **k):
        seen.append((None if frames is None else frames.cpu().tolist(), step_q.cpu().tolist()))
        return real(mag_t, frames, step_q, **k)

    monkeypatch.setattr(lib, 'frames_pitch', spy)
    rule = lib.TacoStopRule(**RULE)
    out = tmp_path / 'long'
    up, down = lib.pitch_step(4), lib.pitch_step(-2.5)
    assert drv.test(_cfg(tmp_path), [PROMPTS[0], LONG], out_dir=str(out), n_iter=2, stop=rule, long=True, pitch=[4, -2.5]) == 2
    assert seen == [(None, [up] + [down] * K)]
    assert np.load(out / 'prompt_000_pitch.npy').tolist() == [up, 32]
    for k in range(K):
        assert np.load(out / ('prompt_001_k%02d_pitch.npy' % k)).tolist() == [down, 32]
    assert not (out / 'prompt_001_pitch.npy').exists() and _wav(out / 'prompt_001.wav')[0] > 0
    del seen[:]
    assert drv.test(_cfg(tmp_path), PROMPTS, out_dir=str(tmp_path / 'rows'), n_iter=2, stop=rule, vocode_lengths=True, pitch=-12) == 2
    assert seen == [([8, 8], [131072, 131072])]


# ---- the acoustic check --------------------------------------------------------------------------------------------------------------
def test_the_fundamental_moves_by_four_semitones(built_lib):
    """a comb of 12.8 bins (100 Hz at 16 kHz) under a smooth envelope, F = 24, through frames_pitch at +4 semitones and Griffin-Lim
    with seeded phases: the largest normalised autocorrelation between 60 and 400 Hz sits at lag 160 unshifted and at 127 = 160 /
    2^(4/12) shifted, +-2 lags (the lag quantisation, about 3 % on the ratio).  tests/test_frames_pitch_host.py confirms the same
    window on the float64 restatement and the NumPy Griffin-Lim."""
    lib = built_lib
    mag = dev(pr.comb(1025, 24)[0][None])
    g = torch.Generator(device='cpu').manual_seed(0)
    phase0 = (2.0 * math.pi * torch.rand(mag.shape, generator=g)).cuda()
    shifted = lib.frames_pitch(mag, step_q=lib.pitch_step(4))
    plain = pr.f0_lag(lib.griffinlim(mag, phase0, 30)[0].cpu().numpy())
    moved = pr.f0_lag(lib.griffinlim(shifted, phase0, 30)[0].cpu().numpy())
    print('  lag / peak unshifted %s, shifted %s' % (plain, moved))
    assert abs(plain[0] - 160) <= 2 and abs(moved[0] - 127) <= 2
    assert min(plain[1], moved[1]) > 0.5
