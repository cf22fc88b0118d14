"""GPU: prosody inside an utterance through the host layers -- griffinlim.invert_spectrogram(rate_curve=, pitch_curve=) and the
driver's `prosody` -- held to the NumPy restatement of the stretch curve (tests/curve_ref.py) and to the Griffin-Lim entry points run
on its output, bit for bit."""
import wave as wavefile

import numpy as np
import pytest
import torch

from tests import curve_ref as cr

pytestmark = pytest.mark.gpu

R, TD, B = 2, 8, 2
F = (TD // 4) * 4 * R          # 16 frames
LENGTHS = (8, 5)               # decoder steps -> 16 and 10 frames


def dev(x, dtype=torch.float32):
    return torch.as_tensor(np.asarray(x), dtype=dtype).cuda()


@pytest.fixture(scope='module')
def frames():
    rng = np.random.default_rng(11)
    out = rng.standard_normal((B, TD, 1025 * R)).astype(np.float32)
    mean = (rng.standard_normal(1025 * R) * 0.3 - 2.0).astype(np.float32)
    std = (0.5 + rng.random(1025 * R)).astype(np.float32)
    return dev(out), dev(mean), dev(std)


@pytest.fixture(scope='module')
def curves():
    """(dur_q (B, F) in [16384, 262144], step_q (B, F): 65536 and three shifts) on the host"""
    rng = np.random.default_rng(12)
    return rng.integers(16384, 262145, (B, F)), rng.choice(np.array([65536, 50000, 80000, 65536, 40000]), (B, F))


@pytest.mark.parametrize('momentum', [None, 0.99], ids=['plain', 'momentum'])
def test_rate_curve_is_griffinlim_on_the_restated_stretch(built_lib, frames, curves, momentum):
    from tacotron_amd.griffinlim import invert_spectrogram
    lib = built_lib
    out, mean, std = frames
    lengths = dev(LENGTHS, torch.int32)
    Fo = lib.stretch_curve_capacity(F, 262144)
    assert Fo == 61
    mag = lib.denorm_unframe(out, mean, std, R, want_spec=False, want_mag_t=True).cpu().numpy()
    ref, ref_n, ref_src = cr.stretch_curve(mag, LENGTHS, curves[0], R, Fo)
    given = torch.full((B,), -1, dtype=torch.int32, device='cuda')
    kw = dict(n_iter=3, seed=7, lengths=lengths, rate_curve=dev(curves[0], torch.int32), frames_out=given)
    if momentum is None:
        wave, n, src = invert_spectrogram(out, mean, std, R, **kw)
        want = lib.griffinlim_rows(dev(ref), dev(ref_n, torch.int32), seed=7, n_iter=3)
    else:
        wave, conv, n, src = invert_spectrogram(out, mean, std, R, momentum=momentum, want_conv=True, **kw)
        want, want_conv = lib.griffinlim_fast(dev(ref), dev(ref_n, torch.int32), seed=7, n_iter=3, momentum=momentum, want_conv=True)
        assert torch.equal(conv.view(torch.int32), want_conv.view(torch.int32))
    torch.cuda.synchronize()
    assert n.data_ptr() == given.data_ptr() and n.tolist() == ref_n.tolist() and np.array_equal(src.cpu().numpy(), ref_src)
    assert wave.shape == (B, 300 * (Fo - 1)) and torch.equal(wave.view(torch.int32), want.view(torch.int32))
    w = wave.cpu().numpy()
    for b, nb in enumerate(ref_n):
        assert not w[b, 300 * (nb - 1):].view(np.uint32).any() and np.abs(w[b, :300 * (nb - 1)]).max() > 0


def test_both_curves_pitch_first_then_the_stretch(built_lib, frames, curves):
    """the pitch curve runs on the unstretched frames; the stretch restatement on its output gives the vocoder's input.  dur_q_max
    is the caller's statement: 131072 halves the capacity, and the device clamps nothing it was not told"""
    from tacotron_amd.griffinlim import invert_spectrogram
    lib = built_lib
    out, mean, std = frames
    lengths = dev(LENGTHS, torch.int32)
    dur = np.minimum(curves[0], 131072)
    mag = lib.denorm_unframe(out, mean, std, R, want_spec=False, want_mag_t=True)
    pitched = lib.frames_pitch_curve(mag, lengths, dev(curves[1], torch.int32), frames_per_unit=R, lifter=32).cpu().numpy()
    assert np.abs(pitched[0, :, 0] / mag.cpu().numpy()[0, :, 0] - 1.0).max() > 0 or curves[1][0, 0] == 65536
    Fo = lib.stretch_curve_capacity(F, 131072)
    assert Fo == 31
    ref, ref_n, ref_src = cr.stretch_curve(pitched, LENGTHS, dur, R, Fo)
    wave, n, src = invert_spectrogram(out, mean, std, R, n_iter=2, seed=3, lengths=lengths, rate_curve=dev(dur, torch.int32),
                                      pitch_curve=dev(curves[1], torch.int32), dur_q_max=131072)
    assert n.tolist() == ref_n.tolist() and np.array_equal(src.cpu().numpy(), ref_src) and wave.shape == (B, 300 * (Fo - 1))
    assert torch.equal(wave, lib.griffinlim_rows(dev(ref), dev(ref_n, torch.int32), seed=3, n_iter=2))


def test_neutral_curves_give_the_bits_of_rate_one_and_pitch_zero(built_lib, frames):
    from tacotron_amd.griffinlim import invert_spectrogram
    out, mean, std = frames
    lengths = dev(LENGTHS, torch.int32)
    one = torch.full((B, F), 65536, dtype=torch.int32, device='cuda')
    for kw in (dict(lengths=lengths), dict()):
        want, want_n = invert_spectrogram(out, mean, std, R, n_iter=2, seed=4, rate=1.0, pitch=0, **kw)
        wave, n, src = invert_spectrogram(out, mean, std, R, n_iter=2, seed=4, rate_curve=one, pitch_curve=one, dur_q_max=65536, **kw)
        assert n.tolist() == want_n.tolist() and torch.equal(wave.view(torch.int32), want.view(torch.int32)) and bool(wave.abs().max() > 0)
        for b, nb in enumerate(n.tolist()):
            assert src[b, :nb].tolist() == [i << 16 for i in range(nb)] and (src[b, nb:] == -1).all()
    for bad in (dict(rate=1.0, rate_curve=one), dict(pitch=0, pitch_curve=one), dict(src=torch.zeros(B, F, dtype=torch.int32, device='cuda')),
                dict(rate_curve=one[:, :5].contiguous()), dict(rate_curve=one, dur_q_max=5)):
        with pytest.raises(ValueError):
            invert_spectrogram(out, mean, std, R, n_iter=2, **bad)


# ---- the driver --------------------------------------------------------------------------------------------------------------------
RULE = dict(end_offset=200, hold=1, min_steps=5)   # target 0: every row stops after step 4 -> len_b = 8
PROMPTS = ['hello world.\n', 'a somewhat longer prompt, with punctuation!\n']
ROWS = [(0, 1, 0.5, None), (1, 0, None, 3.0), (1, 2, 2.0, -2.0), (1, 4, 0.25, None)]


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


def _ivocab():
    ivocab = {i + 1: ch for i, ch in enumerate("abcdefghijklmnopqrstuvwxyz '.,?!-")}
    ivocab[0] = '<pad>'
    return ivocab


def test_driver_writes_the_audio_behind_the_curves(built_lib, tmp_path, monkeypatch):
    """test() with a prosody table, a stop rule and timings: the wav holds 300 (Fo_b - 1) samples of the Griffin-Lim run over the
    stretch curve's frames_out, _prosody.npy the per-character table, the word rows go through the time map, and the model's own files
    are those of a run without prosody, which writes exactly the files it wrote before"""
    from tacotron_amd import alignment, test as drv
    lib = built_lib
    r = _cfg(tmp_path).r
    Fb = 8 * r
    calls, voc = [], []
    real_curve, real_gl = lib.frames_stretch_curve, lib.griffinlim_rows

    def spy_curve(mag_t, frames, dur_q, **k):
        res = real_curve(mag_t, frames, dur_q, **k)
        calls.append((frames.cpu().numpy(), dur_q.cpu().numpy(), k['frames_per_unit'], res[1].cpu().numpy(), res[2].cpu().numpy()))
        return res

    def spy_gl(*a, **k):
        w = real_gl(*a, **k)
        voc.append((a[0].shape, a[1].cpu().numpy(), w.cpu().numpy()))
        return w

    monkeypatch.setattr(lib, 'frames_stretch_curve', spy_curve)
    monkeypatch.setattr(lib, 'griffinlim_rows', spy_gl)
    rule = lib.TacoStopRule(**RULE)
    shaped, plain = tmp_path / 'shaped', tmp_path / 'plain'
    assert drv.test(_cfg(tmp_path), PROMPTS, out_dir=str(shaped), n_iter=2, stop=rule, prosody=ROWS, timings=True) == 2
    assert len(calls) == 1 and len(voc) == 1
    lens, dur_curve, per_unit, fout, src = calls[0]
    Fo = lib.stretch_curve_capacity(16 * r, 262144)
    assert lens.tolist() == [8, 8] and per_unit == r and dur_curve.shape == (2, 16 * r) and src.shape == (2, Fo)
    assert voc[0][0] == (2, 1025, Fo) and voc[0][1].tolist() == fout.tolist()
    table = drv.prosody_table(ROWS, PROMPTS, _ivocab())
    for b in range(2):                                          # the curve holds the table's values along the path, and the map is its
        n, i, wq = cr.time_map(dur_curve[b], Fb, Fo)            # restatement
        assert n == fout[b] and np.array_equal(src[b, :n], (i << 16) | wq) and (src[b, n:] == -1).all()
        assert set(dur_curve[b, :Fb].tolist()) <= set(table[b][:, 0].tolist()) | {65536}
    monkeypatch.setattr(lib, 'frames_stretch_curve', real_curve)
    monkeypatch.setattr(lib, 'griffinlim_rows', real_gl)
    assert drv.test(_cfg(tmp_path), PROMPTS, out_dir=str(plain), n_iter=2, stop=rule, timings=True) == 2
    names = sorted(p.name for p in plain.iterdir())
    assert names == sorted('prompt_%03d%s' % (i, s) for i in range(2)
                           for s in ('.wav', '_spec.npy', '_align.npy', '_len.npy', '_dur.npy', '_words.tsv'))
    assert sorted(p.name for p in shaped.iterdir()) == sorted(names + ['prompt_%03d_prosody.npy' % i for i in range(2)])
    for i in range(2):
        got = np.load(shaped / ('prompt_%03d_prosody.npy' % i))
        assert got.dtype == np.int32 and np.array_equal(got, table[i]) and got.shape == (len(PROMPTS[i].strip()), 2)
        n, data = _wav(shaped / ('prompt_%03d.wav' % i))
        assert n == 300 * (fout[i] - 1) and _wav(plain / ('prompt_%03d.wav' % i))[0] == 300 * (Fb - 1)
        drv.write_wav(str(tmp_path / 'again.wav'), voc[0][2][i, :n])
        assert _wav(tmp_path / 'again.wav')[1] == data and any(data)
        for kind in ('spec', 'align', 'len', 'dur'):
            name = 'prompt_%03d_%s.npy' % (i, kind)
            assert open(shaped / name, 'rb').read() == open(plain / name, 'rb').read(), name
        dur = np.load(shaped / ('prompt_%03d_dur.npy' % i))
        want = alignment.word_times(PROMPTS[i], _ivocab(), dur, r, total=n, src=src[i, :fout[i]])
        rows = [line.split('\t') for line in open(shaped / ('prompt_%03d_words.tsv' % i)).read().splitlines()]
        assert [w for _, _, w in rows] == PROMPTS[i].split() == [w for _, _, w in want]
        times = [float(x) for row in rows for x in row[:2]]
        assert times == sorted(times) and times[-1] <= n / 16000.0 + 1e-9
        assert times == [round(x, 3) for row in want for x in row[:2]]
    assert table[0][:5, 0].tolist() == [65536] * 5 and table[0][6:, 0].tolist() == [131072] * 6       # 'world.' at rate 0.5
    assert table[1][0, 1] == lib.pitch_step(3.0) and table[1][1, 1] == 65536


def test_driver_f0_momentum_and_trim_behind_the_curves(built_lib, tmp_path, monkeypatch, capsys):
    """the options that read the stretched length: _f0.npy holds Fo_b rows and the line is the drift line without a figure asked
    for, _conv.npy comes from the fast rounds over frames_out, and the word rows stay inside the trimmed file"""
    from tacotron_amd import test as drv
    lib = built_lib
    fouts = []
    real_curve = lib.frames_stretch_curve

    def spy_curve(*x, **k):
        res = real_curve(*x, **k)
        fouts.append(res[1].cpu().numpy())
        return res

    monkeypatch.setattr(lib, 'frames_stretch_curve', spy_curve)
    out = tmp_path / 'all'
    assert drv.test(_cfg(tmp_path), PROMPTS, out_dir=str(out), n_iter=2, stop=lib.TacoStopRule(**RULE), prosody=ROWS, f0=True, timings=True,
                    gl_momentum=0.99, trim_db=60.0) == 2
    printed = capsys.readouterr().out
    assert len(fouts) == 1
    for i in range(2):
        n = int(fouts[0][i])
        f0 = np.load(out / ('prompt_%03d_f0.npy' % i))
        assert f0.shape == (n, 2) and f0.dtype == np.float32
        assert np.load(out / ('prompt_%03d_conv.npy' % i)).shape == (3,)
        s, e = np.load(out / ('prompt_%03d_trim.npy' % i)).tolist()
        assert 0 <= s <= e <= 300 * (n - 1) and _wav(out / ('prompt_%03d.wav' % i))[0] == e - s
        rows = [line.split('\t') for line in open(out / ('prompt_%03d_words.tsv' % i)).read().splitlines()]
        times = [float(x) for row in rows for x in row[:2]]
        assert times == sorted(times) and times[0] >= 0.0 and times[-1] <= (e - s) / 16000.0 + 1e-9
        assert 'prompt %d prosody: mean log-F0 moved' % i in printed
    assert 'asked' not in printed


def test_driver_neutral_table_is_rate_one_and_finishing_takes_frames_out(built_lib, tmp_path, monkeypatch):
    """a table that asks for nothing gives the audio of rate 1.0; with de-emphasis taco_wave_finish is handed 300 (Fo_b - 1) per row"""
    from tacotron_amd import test as drv
    lib = built_lib
    r = _cfg(tmp_path).r
    rule = lib.TacoStopRule(**RULE)
    a, b = tmp_path / 'neutral', tmp_path / 'one'
    assert drv.test(_cfg(tmp_path), PROMPTS, out_dir=str(a), n_iter=2, stop=rule, prosody=[(0, 0, None, None)]) == 2
    assert drv.test(_cfg(tmp_path), PROMPTS, out_dir=str(b), n_iter=2, stop=rule, rate=1.0) == 2
    for i in range(2):
        assert _wav(a / ('prompt_%03d.wav' % i)) == _wav(b / ('prompt_%03d.wav' % i)) and _wav(a / ('prompt_%03d.wav' % i))[0] == 300 * (8 * r - 1)
    seen, fouts = [], []
    real, real_curve = lib.wave_finish, lib.frames_stretch_curve

    def spy(*x, **k):
        res = real(*x, **k)
        seen.append((x[0].shape, x[1].cpu().numpy(), res[1].cpu().numpy(), res[2].cpu().numpy()))
        return res

    def spy_curve(*x, **k):
        res = real_curve(*x, **k)
        fouts.append(res[1].cpu().numpy())
        return res

    monkeypatch.setattr(lib, 'wave_finish', spy)
    monkeypatch.setattr(lib, 'frames_stretch_curve', spy_curve)
    out = tmp_path / 'finished'
    assert drv.test(_cfg(tmp_path), PROMPTS, out_dir=str(out), n_iter=2, stop=rule, prosody=ROWS, rate=0.8, pitch=-1.0, deemphasis=0.97) == 2
    assert len(seen) == 1 and len(fouts) == 1 and seen[0][0] == (2, 300 * (lib.stretch_curve_capacity(16 * r, 262144) - 1))
    assert seen[0][1].tolist() == [300 * (int(n) - 1) for n in fouts[0]]
    for i in range(2):
        n = 300 * (int(fouts[0][i]) - 1)
        assert np.load(out / ('prompt_%03d_trim.npy' % i)).tolist() == [0, n] == seen[0][3][i].tolist()
        got, data = _wav(out / ('prompt_%03d.wav' % i))
        assert got == n and data == seen[0][2][i, :n].astype('<i2').tobytes() and any(data)
        table = np.load(out / ('prompt_%03d_prosody.npy' % i))
        assert lib.stretch_dur(0.8) in table[:, 0] and (table[:, 1] != 65536).all()   # --rate / --pitch are the base of the table
    assert not (out / 'prompt_000_rate.npy').exists() and not (out / 'prompt_000_pitch.npy').exists()
