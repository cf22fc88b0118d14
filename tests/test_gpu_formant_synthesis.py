"""GPU: the formant shift through the host layers -- griffinlim.invert_spectrogram(formant=...) and the driver's --formant
(Config.formant) -- held bit for bit to the same calls without it (formant 0 / None), to lib.frames_formant behind lib.frames_sharpen
and in front of lib.frames_pitch / lib.frames_stretch and the vocoder's entry points, and the F0 tracker's word that the pitch did
not move."""
import wave as wavefile

import numpy as np
import pytest
import torch

from tests import f0_ref
from tests import formant_ref as fr
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


@pytest.mark.parametrize('rate,pitch', [(None, None), (0.5, 2.0)], ids=['alone', 'rate_pitch'])
@pytest.mark.parametrize('with_lengths', [False, True], ids=['full', 'lengths'])
def test_formant_zero_is_the_call_without_it(built_lib, frames, with_lengths, rate, pitch):
    from tacotron_amd.griffinlim import invert_spectrogram
    out, mean, std = frames
    kw = dict(n_iter=3, seed=5, lengths=dev(LENGTHS, torch.int32) if with_lengths else None, rate=rate, pitch=pitch)
    plain = invert_spectrogram(out, mean, std, R, **kw)
    none = invert_spectrogram(out, mean, std, R, formant=None, formant_lifter=16, **kw)
    zero = invert_spectrogram(out, mean, std, R, formant=0.0, **kw)
    izero = invert_spectrogram(out, mean, std, R, formant=0, **kw)
    moved = invert_spectrogram(out, mean, std, R, formant=2.0, **kw)
    torch.cuda.synchronize()
    plain, none, zero, izero, moved = ((x,) if rate is None else tuple(x) for x in (plain, none, zero, izero, moved))
    assert len(plain) == len(zero) == len(moved) == 1 + (rate is not None)
    for other in (none, zero, izero):
        for a, b in zip(plain, other):
            assert a.dtype == b.dtype and same_bits(a, b)
    assert bool(plain[0].abs().max() > 0)
    assert moved[0].shape == plain[0].shape and not same_bits(moved[0], plain[0])     # no return shape changes; the samples do
    if rate is not None:
        assert torch.equal(moved[-1], plain[-1])                                       # frames_out: the duration is the rate's alone


def test_formant_is_frames_formant_between_sharpen_and_pitch(built_lib, frames):
    """behind the post-filter and the 'model' track, in front of the pitch and the stretch; the 'formant' track behind it"""
    from tacotron_amd.griffinlim import invert_spectrogram, vocode
    lib = built_lib
    out, mean, std = frames
    lengths = dev(LENGTHS, torch.int32)
    step = lib.formant_step(2.0)
    mag = lib.denorm_unframe(out, mean, std, R, want_spec=False, want_mag_t=True)
    moved = lib.frames_formant(mag, lengths, step, R, 24)
    assert not moved[1, :, 10:].any() and bool((moved[1, :, :10] > 0).all())
    want = lib.griffinlim_rows(moved, lengths, seed=7, n_iter=2, frames_per_unit=R)
    assert same_bits(invert_spectrogram(out, mean, std, R, n_iter=2, seed=7, lengths=lengths, formant=2.0, formant_lifter=24), want)
    # a host sequence and a device tensor of step_q values are the same call
    per_row = [2.0, -3.0]
    a = invert_spectrogram(out, mean, std, R, n_iter=2, seed=7, lengths=lengths, formant=per_row)
    b = invert_spectrogram(out, mean, std, R, n_iter=2, seed=7, lengths=lengths, formant=dev([lib.formant_step(x) for x in per_row], torch.int32))
    want = lib.griffinlim_rows(lib.frames_formant(mag, lengths, [lib.formant_step(x) for x in per_row], R), lengths, seed=7, n_iter=2,
                               frames_per_unit=R)
    assert same_bits(a, want) and same_bits(b, want)
    # with the post-filter, a pitch and a rate: sharpen, formant, pitch, stretch
    sharp = lib.frames_sharpen(mag, 0.4, 24, lengths, R)
    moved = lib.frames_formant(sharp, lengths, step, R, 20)
    shifted = lib.frames_pitch(moved, lengths, [lib.pitch_step(3.0)] * B, frames_per_unit=R, lifter=32)
    stretched, n = lib.frames_stretch(shifted, lengths, 32768, frames_per_unit=R, Fo=lib.stretch_capacity(F, 32768))
    want = lib.griffinlim_rows(stretched, n, seed=7, n_iter=2)
    v = vocode(out, mean, std, R, n_iter=2, seed=7, lengths=lengths, sharpen=0.4, sharpen_lifter=24, formant=2.0, formant_lifter=20,
               pitch=3.0, rate=0.5, f0=True)
    assert same_bits(v.waveform, want) and v.frames_out.tolist() == n.tolist()
    # 'model' is measured in front of the stage (on the sharpened frames), 'formant' behind it, 'pitched' behind the pitch
    w, g, lag_min, lag_max = lib.f0_tables(C=1025)
    tab = dict(weight=dev(w), gain=dev(g), lag_min=lag_min, lag_max=lag_max)
    p_model, p_formant, p_pitched = (lib.frames_f0(x, lengths, R, **tab)[0] for x in (sharp, moved, shifted))
    assert same_bits(v.tracks['model'][0], p_model) and same_bits(v.tracks['formant'][0], p_formant)
    assert same_bits(v.tracks['pitched'][0], p_pitched)
    assert same_bits(v.tracks['formant_stats'], lib.f0_stats(p_formant, p_model, lengths, R))
    assert same_bits(v.tracks['pitch_stats'], lib.f0_stats(p_pitched, p_formant, lengths, R))   # against the track in front of the pitch
    assert same_bits(v.tracks['vocoder'][0], lib.frames_f0(stretched, n, 1, **tab)[0])
    # without a formant every track and statistic is what it was
    v0 = vocode(out, mean, std, R, n_iter=2, seed=7, lengths=lengths, sharpen=0.4, sharpen_lifter=24, pitch=3.0, rate=0.5, f0=True)
    assert 'formant' not in v0.tracks and 'formant_stats' not in v0.tracks
    p_plain = lib.frames_f0(lib.frames_pitch(sharp, lengths, [lib.pitch_step(3.0)] * B, frames_per_unit=R, lifter=32), lengths, R, **tab)[0]
    assert same_bits(v0.tracks['pitch_stats'], lib.f0_stats(p_plain, p_model, lengths, R))
    # alone with f0: the last stage is the vocoder's, and its summary is the track's own
    v = vocode(out, mean, std, R, n_iter=0, seed=7, formant=-4.0, phase_init='estimate', f0=True)
    full = lib.frames_formant(mag, None, lib.formant_step(-4.0))
    assert same_bits(v.waveform, lib.griffinlim(full, lib.phase_estimate(full), 0))
    p_full = lib.frames_f0(full, None, 1, **tab)[0]
    assert same_bits(v.tracks['vocoder'][0], p_full) and same_bits(v.tracks['vocoder_stats'], lib.f0_stats(p_full))
    for bad in (dict(formant=12.5), dict(formant=float('nan')), dict(formant=2.0, formant_lifter=0), dict(formant=2.0, formant_lifter=65),
                dict(formant=[1.0, 2.0, 3.0])):
        with pytest.raises(ValueError):
            invert_spectrogram(out, mean, std, R, n_iter=2, **bad)


def test_the_pitch_does_not_move(built_lib):
    """on the comb (harmonics every 12.8 bins: a period of 160 samples) the device's frames_f0 period behind a +-3 semitone formant
    shift is the period in front of it.  Allowed per frame, in lags: what the restatements (formant_ref, then f0_ref.track, float64)
    give for the same frames, plus what the two device tracks may differ from their restatements by -- an error e of each of the three
    autocorrelation values around the peak moves the parabola's vertex 0.5 (ym - yp) / (ym - 2 y0 + yp) by at most 3 e / |ym - 2 y0 + yp|
    (|vertex| <= 0.5), with e = F0_ACF_ATOL for the tracker plus 6 FORMANT_RTOL for the shifted magnitudes (a relative error r of a
    magnitude is 2 r of a power, at most 4 r of a normalised autocorrelation value, and those stay below 1.5)."""
    lib = built_lib
    m, _ = pr.comb(C=1025, F=8, spacing=12.8)
    x = m[None]
    w, g, lag_min, lag_max = f0_ref.tables()
    tab = dict(weight=w, gain=g, lag_min=lag_min, lag_max=lag_max)
    dtab = dict(weight=dev(w), gain=dev(g), lag_min=lag_min, lag_max=lag_max)
    e = f0_ref.F0_ACF_ATOL + 6.0 * fr.FORMANT_RTOL

    def vertex_slack(mags, period):
        y = f0_ref.acf(mags, **tab)[0]
        at = np.rint(period).astype(int) - lag_min + 1
        cols = np.arange(y.shape[1])
        return 3.0 * e / np.abs(y[at - 1, cols] - 2.0 * y[at, cols] + y[at + 1, cols])

    p_in = f0_ref.track(x, **tab)[0][0]
    assert np.abs(p_in - 160.0).max() < 0.1
    d_in = lib.frames_f0(dev(x), **dtab)[0][0].cpu().numpy().astype(np.float64)
    for semitones in (-3.0, 3.0):
        step = fr.formant_step(semitones)
        ref = fr.formant(x, None, [step], 1, 32).astype(np.float32)
        p_out = f0_ref.track(ref, **tab)[0][0]
        drift = np.abs(p_out - p_in)
        assert drift.max() < 0.05                                                       # the definition keeps the pitch: 0.5 cent
        allowed = drift + vertex_slack(x, p_in) + vertex_slack(ref, p_out)
        moved = lib.frames_formant(dev(x), None, step)
        d_out = lib.frames_f0(moved, **dtab)[0][0].cpu().numpy().astype(np.float64)
        print('  %+g semitones: restated drift %s lags, device %s, allowed %s' % (semitones, drift, np.abs(d_out - d_in), allowed))
        assert (d_in > 0).all() and (d_out > 0).all() and (np.abs(d_out - d_in) <= allowed).all()
        assert allowed.max() < 0.2
        # and the envelope did move: the magnitudes are not the source's
        assert float((moved[0].cpu() / torch.from_numpy(m) - 1.0).abs().max()) > 0.1


# ---- the driver --------------------------------------------------------------------------------------------------------------------
RULE = dict(end_offset=200, hold=1, min_steps=5)   # target 0: every row stops after step 4 -> len_b = 8
PROMPTS = ['hello world.\n', 'a somewhat longer prompt, with punctuation!\n']
LONG = ('the first sentence of this prompt is long enough to fill a good part of one piece on its own, and it ends here. '
        'the second one has no full stop for a long while, only a comma after a run of words that goes on and on and on, '
        'and then more words that follow the comma until the line has well over three hundred characters in it.\n')


def _cfg(tmp_path, formant=None, lifter=32, sharpen=None):
    from tacotron_amd.config import Config
    c = Config()
    c.data_path = str(tmp_path / 'no_data') + '/'
    c.max_decode_iter = 16
    c.formant, c.formant_lifter, c.sharpen = formant, lifter, sharpen
    return c


def _wav(path):
    with wavefile.open(str(path)) as f:
        assert f.getframerate() == 16000 and f.getsampwidth() == 2 and f.getnchannels() == 1
        return f.getnframes(), f.readframes(f.getnframes())


def _read(path):
    with open(path, 'rb') as f:
        return f.read()


def _spies(lib, monkeypatch):
    seen = []
    for name in ('frames_sharpen', 'frames_formant', 'frames_pitch', 'frames_stretch'):
        def spy(mag_t, *a, _real=getattr(lib, name), _name=name, **k):
            seen.append((_name, tuple(mag_t.shape), a, k))
            return _real(mag_t, *a, **k)
        monkeypatch.setattr(lib, name, spy)
    return seen


def test_driver_writes_the_formant_file_and_leaves_the_rest(built_lib, tmp_path, monkeypatch):
    """test() with Config.formant = 2: prompt_NNN_formant.npy = (step_q, lifter) and another wav; every other file has the name, size
    and -- the model's own files -- the bytes of the run without it; formant 0 is the run without it, byte for byte, file for file"""
    from tacotron_amd import test as drv
    lib = built_lib
    seen = _spies(lib, monkeypatch)
    rule = lib.TacoStopRule(**RULE)
    r = _cfg(tmp_path).r
    plain, moved, zero = tmp_path / 'plain', tmp_path / 'moved', tmp_path / 'zero'
    assert drv.test(_cfg(tmp_path), PROMPTS, out_dir=str(plain), n_iter=2, stop=rule) == 2
    assert not seen
    assert drv.test(_cfg(tmp_path, 2.0, 24), PROMPTS, out_dir=str(moved), n_iter=2, stop=rule) == 2
    assert [(s[0], s[1]) for s in seen] == [('frames_formant', (2, 1025, 16 * r))]
    counts, step_q = seen[0][2]
    assert counts is None and step_q.tolist() == [lib.formant_step(2.0)] * 2                 # (no lengths: all frames, as the vocoder)
    assert seen[0][3] == dict(frames_per_unit=1, lifter=24)
    del seen[:]
    assert drv.test(_cfg(tmp_path, 0.0), PROMPTS, out_dir=str(zero), n_iter=2, stop=rule) == 2
    assert not seen
    names = sorted(p.name for p in plain.iterdir())
    assert names == sorted('prompt_%03d%s' % (i, s) for i in range(2) for s in ('.wav', '_spec.npy', '_align.npy', '_len.npy'))
    assert sorted(p.name for p in zero.iterdir()) == names
    assert sorted(p.name for p in moved.iterdir()) == sorted(names + ['prompt_%03d_formant.npy' % i for i in range(2)])
    for name in names:
        assert _read(zero / name) == _read(plain / name), name
        if name.endswith('.npy'):
            assert _read(moved / name) == _read(plain / name), name
        else:
            assert _wav(moved / name)[0] == _wav(plain / name)[0] > 0 and _wav(moved / name)[1] != _wav(plain / name)[1]
    for i in range(2):
        got = np.load(moved / ('prompt_%03d_formant.npy' % i))
        assert got.dtype == np.int32 and got.tolist() == [lib.formant_step(2.0), 24]
    with pytest.raises(ValueError, match='formant'):
        drv.test(_cfg(tmp_path, 2.0), PROMPTS, out_dir=str(tmp_path / 'x'), n_iter=2, vocode=False)
    with pytest.raises(ValueError, match='formant'):
        drv.test(_cfg(tmp_path, -12.5), PROMPTS, out_dir=str(tmp_path / 'x'), n_iter=2)
    with pytest.raises(ValueError, match='formant_lifter'):
        drv.test(_cfg(tmp_path, 2.0, 65), PROMPTS, out_dir=str(tmp_path / 'x'), n_iter=2)


def test_driver_combines_with_stop_sharpen_pitch_rate_f0_and_long(built_lib, tmp_path, monkeypatch, capsys):
    """--stop --sharpen --pitch --rate --f0 --formant: sharpen, formant, pitch, stretch, each over the row's own frames; the other
    files are those of the run without it; one formant line per prompt; with `long` every piece is shifted and writes its own
    _formant.npy"""
    from tacotron_amd import test as drv
    lib = built_lib
    seen = _spies(lib, monkeypatch)
    rule = lib.TacoStopRule(**RULE)
    r = _cfg(tmp_path).r
    common = dict(n_iter=2, stop=rule, pitch=3.0, rate=0.8, f0=True)
    plain, moved = tmp_path / 'plain', tmp_path / 'moved'
    assert drv.test(_cfg(tmp_path, sharpen=0.4), PROMPTS, out_dir=str(plain), **common) == 2
    assert [s[0] for s in seen] == ['frames_sharpen', 'frames_pitch', 'frames_stretch']
    plain_out = capsys.readouterr().out
    assert ' formant asked ' not in plain_out
    del seen[:]
    assert drv.test(_cfg(tmp_path, -3.0, sharpen=0.4), PROMPTS, out_dir=str(moved), **common) == 2
    assert [s[0] for s in seen] == ['frames_sharpen', 'frames_formant', 'frames_pitch', 'frames_stretch']
    counts, step_q = seen[1][2]
    assert (counts.tolist(), step_q.tolist(), seen[1][3]) == ([8, 8], [lib.formant_step(-3.0)] * 2, dict(frames_per_unit=r, lifter=32))
    lines = [line for line in capsys.readouterr().out.splitlines() if ' formant asked ' in line]
    assert len(lines) == 2 and all(line.startswith('prompt %d formant asked -3.00 semitones, F0 moved ' % i) and
                                   line.endswith(' voiced frames') and ' cents over ' in line for i, line in enumerate(lines))
    names = sorted(p.name for p in plain.iterdir())
    assert sorted(p.name for p in moved.iterdir()) == sorted(names + ['prompt_%03d_formant.npy' % i for i in range(2)])
    for name in names:
        if name.endswith('_f0.npy'):
            assert np.load(moved / name).shape == np.load(plain / name).shape             # the track is the shifted frames'
        elif name.endswith('.npy'):
            assert _read(moved / name) == _read(plain / name), name
        else:
            assert _wav(moved / name)[0] == _wav(plain / name)[0] > 0 and _wav(moved / name)[1] != _wav(plain / name)[1]
    del seen[:]
    out = tmp_path / 'long'
    assert drv.test(_cfg(tmp_path, 2.0), [PROMPTS[0], LONG], out_dir=str(out), n_iter=2, stop=rule, long=True) == 2
    K = len(list(out.glob('prompt_001_k*_spec.npy')))
    assert K >= 2 and [s[0] for s in seen] == ['frames_formant'] and seen[0][1][0] == 1 + K      # one batch: every piece a row
    assert np.load(out / 'prompt_000_formant.npy').tolist() == [lib.formant_step(2.0), 32]
    for k in range(K):
        assert np.load(out / ('prompt_001_k%02d_formant.npy' % k)).tolist() == [lib.formant_step(2.0), 32]
    assert not (out / 'prompt_001_formant.npy').exists() and _wav(out / 'prompt_001.wav')[0] > 0


def test_driver_combines_with_prosody(built_lib, tmp_path, monkeypatch):
    """--prosody: the formant is a per-row constant in front of the curves"""
    from tacotron_amd import test as drv
    lib = built_lib
    seen = []
    for name in ('frames_formant', 'frames_pitch_curve', 'frames_stretch_curve'):
        def spy(mag_t, *a, _real=getattr(lib, name), _name=name, **k):
            seen.append(_name)
            return _real(mag_t, *a, **k)
        monkeypatch.setattr(lib, name, spy)
    rule = lib.TacoStopRule(**RULE)
    table = [(0, 0, 0.8, 2.0), (1, 1, None, -1.0)]
    assert drv.test(_cfg(tmp_path, 2.0), PROMPTS, out_dir=str(tmp_path / 'p'), n_iter=2, stop=rule, prosody=table) == 2
    assert seen == ['frames_formant', 'frames_pitch_curve', 'frames_stretch_curve']
    for i in range(2):
        assert np.load(tmp_path / 'p' / ('prompt_%03d_formant.npy' % i)).tolist() == [lib.formant_step(2.0), 32]
        assert (tmp_path / 'p' / ('prompt_%03d_prosody.npy' % i)).exists()
