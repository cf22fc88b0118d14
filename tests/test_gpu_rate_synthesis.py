"""GPU: the speaking rate through the host layers -- griffinlim.invert_spectrogram(rate=...) and the driver's `rate` -- held to the
NumPy restatement of the stretch (tests/stretch_ref.py) and to the Griffin-Lim entry points run on its output, bit for bit."""
import wave as wavefile

import numpy as np
import pytest
import torch

from tests import stretch_ref as sr

pytestmark = pytest.mark.gpu

R, TD, B = 2, 8, 2
F = (TD // 4) * 4 * R          # 16 frames
LENGTHS = (8, 5)               # decoder steps -> 16 and 10 frames


def dev(x, dtype=torch.float32):
    return torch.as_tensor(np.asarray(x), dtype=dtype).cuda()


@pytest.fixture(scope='module')
def frames():
    """(out, mean, std): a normalised model output (B, Td, 1025 r) and the statistics that de-normalise it, on the device"""
    rng = np.random.default_rng(11)
    out = rng.standard_normal((B, TD, 1025 * R)).astype(np.float32)
    mean = (rng.standard_normal(1025 * R) * 0.3 - 2.0).astype(np.float32)
    std = (0.5 + rng.random(1025 * R)).astype(np.float32)
    return dev(out), dev(mean), dev(std)


def stretched_ref(lib, frames, lengths, steps, Fo):
    """the restatement's stretch of the magnitudes the library de-normalises, uploaded, and its frames_out"""
    out, mean, std = frames
    mag = lib.denorm_unframe(out, mean, std, R, want_spec=False, want_mag_t=True).cpu().numpy()
    want, n = sr.stretch(mag, lengths, steps, R if lengths is not None else 1, Fo)
    return dev(want), n


def test_rate_one_is_the_call_without_a_rate(built_lib, frames):
    from tacotron_amd.griffinlim import invert_spectrogram
    out, mean, std = frames
    lengths = dev(LENGTHS, torch.int32)
    for momentum in (None, 0.99):
        plain = invert_spectrogram(out, mean, std, R, n_iter=3, seed=5, lengths=lengths, momentum=momentum)
        wave, n = invert_spectrogram(out, mean, std, R, n_iter=3, seed=5, lengths=lengths, momentum=momentum, rate=1.0)
        torch.cuda.synchronize()
        assert n.tolist() == [16, 10] and wave.shape == plain.shape == (B, 300 * (F - 1))
        assert torch.equal(wave.view(torch.int32), plain.view(torch.int32)) and bool(wave.abs().max() > 0)


@pytest.mark.parametrize('momentum', [None, 0.99], ids=['plain', 'momentum'])
def test_half_rate_is_griffinlim_on_the_restated_stretch(built_lib, frames, momentum):
    from tacotron_amd.griffinlim import invert_spectrogram
    lib = built_lib
    out, mean, std = frames
    lengths = dev(LENGTHS, torch.int32)
    Fo = lib.stretch_capacity(F, 32768)
    assert Fo == 31
    ref_mag, ref_n = stretched_ref(lib, frames, LENGTHS, (32768, 32768), Fo)
    assert ref_n.tolist() == [31, 19]
    given = torch.full((B,), -1, dtype=torch.int32, device='cuda')
    if momentum is None:
        wave, n = invert_spectrogram(out, mean, std, R, n_iter=3, seed=7, lengths=lengths, rate=0.5, frames_out=given)
        want = lib.griffinlim_rows(ref_mag, dev(ref_n, torch.int32), seed=7, n_iter=3)
    else:
        wave, conv, n = invert_spectrogram(out, mean, std, R, n_iter=3, seed=7, lengths=lengths, rate=0.5, frames_out=given,
                                           momentum=momentum, want_conv=True)
        want, want_conv = lib.griffinlim_fast(ref_mag, dev(ref_n, torch.int32), seed=7, n_iter=3, momentum=momentum, want_conv=True)
        assert torch.equal(conv.view(torch.int32), want_conv.view(torch.int32))
    torch.cuda.synchronize()
    assert n.data_ptr() == given.data_ptr() and n.tolist() == [31, 19]
    assert wave.shape == (B, 300 * (Fo - 1)) and torch.equal(wave.view(torch.int32), want.view(torch.int32))
    w = wave.cpu().numpy()
    for b, nb in enumerate(ref_n):
        assert not w[b, 300 * (nb - 1):].view(np.uint32).any() and np.abs(w[b, :300 * (nb - 1)]).max() > 0


def test_rates_per_row_device_steps_and_all_frames(built_lib, frames):
    from tacotron_amd.griffinlim import invert_spectrogram
    lib = built_lib
    out, mean, std = frames
    lengths = dev(LENGTHS, torch.int32)
    # one rate per row: the capacity is that of the slowest
    ref_mag, ref_n = stretched_ref(lib, frames, LENGTHS, (32768, 131072), 31)
    wave, n = invert_spectrogram(out, mean, std, R, n_iter=2, seed=1, lengths=lengths, rate=[0.5, 2.0])
    assert n.tolist() == ref_n.tolist() == [31, 5]
    assert torch.equal(wave, lib.griffinlim_rows(ref_mag, dev(ref_n, torch.int32), seed=1, n_iter=2))
    # step_q on the device: the host knows no rate, the capacity is that of rate 0.25
    ref_mag, ref_n = stretched_ref(lib, frames, LENGTHS, (32768, 131072), 61)
    wave, n = invert_spectrogram(out, mean, std, R, n_iter=2, seed=1, lengths=lengths, rate=dev([32768, 131072], torch.int32))
    assert wave.shape == (B, 300 * 60) and n.tolist() == [31, 5]
    assert torch.equal(wave, lib.griffinlim_rows(ref_mag, dev(ref_n, torch.int32), seed=1, n_iter=2))
    # lengths None: all F frames are the source; a fast rate leaves the 5 frames Griffin-Lim needs at least
    ref_mag, ref_n = stretched_ref(lib, frames, None, (262144, 262144), 5)
    wave, n = invert_spectrogram(out, mean, std, R, n_iter=2, seed=1, rate=4.0)
    assert wave.shape == (B, 300 * 4) and n.tolist() == ref_n.tolist() == [4, 4]
    assert torch.equal(wave, lib.griffinlim_rows(ref_mag, dev(ref_n, torch.int32), seed=1, n_iter=2))
    for bad in (dict(rate=0.1), dict(rate=[0.5]), dict(frames_out=torch.zeros(B, dtype=torch.int32, device='cuda'))):
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


def test_driver_writes_the_stretched_audio(built_lib, tmp_path, monkeypatch):
    """test() with rate 0.5 and a stop rule: the wav holds 300 (Fo_b - 1) samples of the stretched waveform, _rate.npy (32768, Fo_b), and
    the model's own files are those of a run without a rate, which writes exactly the files it wrote before"""
    from tacotron_amd import test as drv
    lib = built_lib
    r = _cfg(tmp_path).r
    Fb = 8 * r
    Fob = lib.stretch_frames(Fb, 32768)
    assert Fob == 2 * Fb - 1
    seen = []
    real = lib.griffinlim_rows

    def spy(*a, **k):
        w = real(*a, **k)
        seen.append((a[0].shape, a[1].cpu().numpy(), w.cpu().numpy()))
        return w

    monkeypatch.setattr(lib, 'griffinlim_rows', spy)
    rule = lib.TacoStopRule(**RULE)
    slow, plain = tmp_path / 'slow', tmp_path / 'plain'
    assert drv.test(_cfg(tmp_path), PROMPTS, out_dir=str(slow), n_iter=2, stop=rule, rate=0.5) == 2
    assert len(seen) == 1 and seen[0][0] == (2, 1025, lib.stretch_capacity(16 * r, 32768)) and seen[0][1].tolist() == [Fob] * 2
    monkeypatch.setattr(lib, 'griffinlim_rows', real)
    assert drv.test(_cfg(tmp_path), PROMPTS, out_dir=str(plain), n_iter=2, stop=rule) == 2
    names = sorted(p.name for p in plain.iterdir())
    assert names == sorted('prompt_%03d%s' % (i, s) for i in range(2) for s in ('.wav', '_spec.npy', '_align.npy', '_len.npy'))
    assert sorted(p.name for p in slow.iterdir()) == sorted(names + ['prompt_%03d_rate.npy' % i for i in range(2)])
    for i in range(2):
        rate = np.load(slow / ('prompt_%03d_rate.npy' % i))
        assert rate.dtype == np.int32 and rate.tolist() == [32768, Fob]
        n, data = _wav(slow / ('prompt_%03d.wav' % i))
        assert n == 300 * (Fob - 1) and _wav(plain / ('prompt_%03d.wav' % i))[0] == 300 * (Fb - 1)
        drv.write_wav(str(tmp_path / 'again.wav'), seen[0][2][i, :n])
        assert _wav(tmp_path / 'again.wav')[1] == data and any(data)
        for kind in ('spec', 'align', 'len'):
            name = 'prompt_%03d_%s.npy' % (i, kind)
            assert open(slow / name, 'rb').read() == open(plain / name, 'rb').read(), name
    with pytest.raises(ValueError, match='rate'):
        drv.test(_cfg(tmp_path), PROMPTS, out_dir=str(tmp_path / 'x'), n_iter=2, rate=0.5, vocode=False)
    with pytest.raises(ValueError, match='rate'):
        drv.test(_cfg(tmp_path), PROMPTS, out_dir=str(tmp_path / 'x'), n_iter=2, rate=[0.5])


def test_driver_finishes_over_the_stretched_lengths(built_lib, tmp_path, monkeypatch):
    """with de-emphasis the row's samples come from the stretch's frames_out on the device: taco_wave_finish is handed 300 (Fo_b - 1)
    per row and the wav holds the device's PCM16 over them; one rate per prompt, and no stop rule for the second run"""
    from tacotron_amd import test as drv
    lib = built_lib
    r = _cfg(tmp_path).r
    seen = []
    real = lib.wave_finish

    def spy(*a, **k):
        res = real(*a, **k)
        seen.append((a[0].shape, a[1].cpu().numpy(), res[1].cpu().numpy(), res[2].cpu().numpy()))
        return res

    monkeypatch.setattr(lib, 'wave_finish', spy)
    rule = lib.TacoStopRule(**RULE)
    rates = [0.5, 1.25]
    steps = [lib.stretch_step(x) for x in rates]
    for sub, stop, Fb in (('stop', rule, 8 * r), ('full', None, 16 * r)):
        del seen[:]
        out = tmp_path / sub
        assert drv.test(_cfg(tmp_path), PROMPTS, out_dir=str(out), n_iter=2, stop=stop, rate=rates, deemphasis=0.97) == 2
        Fob = [lib.stretch_frames(Fb, q) for q in steps]
        assert len(seen) == 1 and seen[0][0] == (2, 300 * (lib.stretch_capacity(16 * r, steps[0]) - 1))
        assert seen[0][1].tolist() == [300 * (n - 1) for n in Fob]
        for i in range(2):
            n = 300 * (Fob[i] - 1)
            assert np.load(out / ('prompt_%03d_rate.npy' % i)).tolist() == [steps[i], Fob[i]]
            assert np.load(out / ('prompt_%03d_trim.npy' % i)).tolist() == [0, n] == seen[0][3][i].tolist()
            got, data = _wav(out / ('prompt_%03d.wav' % i))
            assert got == n and data == seen[0][2][i, :n].astype('<i2').tobytes() and any(data)


def test_driver_joins_pieces_of_their_stretched_lengths(built_lib, tmp_path, monkeypatch):
    """with `long` a prompt's pieces inherit its rate, and the lengths flow from frames_out through taco_wave_finish's bounds into
    taco_wave_join: every piece of the slowed prompt is 300 (Fo_b - 1) samples long in the join"""
    from tacotron_amd import data, test as drv
    lib = built_lib
    r = _cfg(tmp_path).r
    kinds = [k for _, k in data.split_prompt(LONG)]
    K = len(kinds)
    assert K >= 3
    seen = []
    real = lib.wave_join

    def spy(pieces, bounds, first, gap, *a, **k):
        res = real(pieces, bounds, first, gap, *a, **k)
        seen.append((pieces.shape, bounds.cpu().numpy(), list(first), list(gap), res[3].cpu().numpy()))
        return res

    monkeypatch.setattr(lib, 'wave_join', spy)
    rule = lib.TacoStopRule(**RULE)
    out = tmp_path / 'long'
    assert drv.test(_cfg(tmp_path), [PROMPTS[0], LONG], out_dir=str(out), n_iter=2, stop=rule, long=True, rate=[1.0, 0.5]) == 2
    n1, n2 = 300 * (8 * r - 1), 300 * (lib.stretch_frames(8 * r, 32768) - 1)
    assert len(seen) == 1
    shape, bounds, first, gap, total = seen[0]
    assert shape == (1 + K, 300 * (lib.stretch_capacity(16 * r, 32768) - 1)) and first == [0, 1, 1 + K]
    assert bounds.tolist() == [[0, n1]] + [[0, n2]] * K
    assert total.tolist() == [n1, K * n2 + sum(gap[1:-1])]
    assert _wav(out / 'prompt_000.wav')[0] == n1 and _wav(out / 'prompt_001.wav')[0] == total[1]
    assert np.load(out / 'prompt_000_rate.npy').tolist() == [65536, 8 * r]
    table = np.load(out / 'prompt_001_pieces.npy')
    assert table[:, 1].tolist() == [n2] * K
    for k in range(K):
        assert np.load(out / ('prompt_001_k%02d_rate.npy' % k)).tolist() == [32768, lib.stretch_frames(8 * r, 32768)]
        assert np.load(out / ('prompt_001_k%02d_len.npy' % k)) == 8
