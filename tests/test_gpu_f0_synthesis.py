"""GPU: the F0 tracker through the host layers -- griffinlim.invert_spectrogram(f0=...), the driver's `f0` and evaluate's -- held to
lib.frames_f0 / lib.f0_stats on the same frames, and bit for bit to the same calls without it: measuring changes nothing else."""

import numpy as np
import pytest
import torch

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


@pytest.mark.parametrize('pitch', [None, 3.0], ids=['no_pitch', 'pitch'])
@pytest.mark.parametrize('rate', [None, 0.5], ids=['no_rate', 'rate'])
@pytest.mark.parametrize('momentum', [None, 0.99], ids=['plain', 'momentum'])
@pytest.mark.parametrize('with_lengths', [False, True], ids=['full', 'lengths'])
def test_f0_adds_the_tracks_and_changes_nothing(built_lib, frames, with_lengths, momentum, rate, pitch):
    from tacotron_amd.griffinlim import invert_spectrogram
    lib = built_lib
    out, mean, std = frames
    lengths = dev(LENGTHS, torch.int32) if with_lengths else None
    kw = dict(n_iter=2, seed=5, lengths=lengths, momentum=momentum, rate=rate, want_conv=momentum is not None, pitch=pitch)
    plain = invert_spectrogram(out, mean, std, R, **kw)
    got = invert_spectrogram(out, mean, std, R, f0=dict(threshold=0.0), **kw)
    torch.cuda.synchronize()
    plain = tuple(plain) if isinstance(plain, tuple) else (plain,)
    assert isinstance(got, tuple) and len(got) == len(plain) + 1 and isinstance(got[-1], dict)
    for a, b in zip(plain, got):
        assert a.dtype == b.dtype and same_bits(a, b)
    tracks = got[-1]
    per = R if with_lengths else 1
    mag = lib.denorm_unframe(out, mean, std, R, want_spec=False, want_mag_t=True)
    w, g, lo, hi = lib.f0_tables()
    opt = dict(weight=dev(w), gain=dev(g), lag_min=lo, lag_max=hi, threshold=0.0)
    want = lib.frames_f0(mag, lengths, per, **opt)
    assert all(same_bits(a, b) for a, b in zip(tracks['model'], want))
    assert same_bits(tracks['model_stats'], lib.f0_stats(want[0], None, lengths, per))
    last = mag
    if pitch is not None:
        last = lib.frames_pitch(mag, lengths, lib.pitch_step(pitch), frames_per_unit=per)
        moved = lib.frames_f0(last, lengths, per, **opt)
        assert all(same_bits(a, b) for a, b in zip(tracks['pitched'], moved))
        assert same_bits(tracks['pitch_stats'], lib.f0_stats(moved[0], want[0], lengths, per))
    else:
        assert 'pitched' not in tracks and 'pitch_stats' not in tracks
    if rate is not None:
        stretched, n = lib.frames_stretch(last, lengths, lib.stretch_step(rate), frames_per_unit=per, Fo=max(5, lib.stretch_capacity(F, 32768)))
        voc = lib.frames_f0(stretched, n, 1, **opt)
        assert all(same_bits(a, b) for a, b in zip(tracks['vocoder'], voc)) and tracks['vocoder'][0].shape[1] == stretched.shape[2]
        assert same_bits(tracks['vocoder_stats'], lib.f0_stats(voc[0], None, n, 1))
    else:
        assert tracks['vocoder'] is tracks['pitched' if pitch is not None else 'model']
    if with_lengths:
        assert not tracks['model'][0][1, 10:].any()
    with pytest.raises(ValueError, match='f0'):
        invert_spectrogram(out, mean, std, R, n_iter=2, f0=dict(smoothing=3))


def test_default_tables_are_the_production_ones(built_lib, frames):
    from tacotron_amd.griffinlim import invert_spectrogram
    lib = built_lib
    out, mean, std = frames
    _, tracks = invert_spectrogram(out, mean, std, R, n_iter=1, f0=True)
    w, g, lo, hi = lib.f0_tables()
    mag = lib.denorm_unframe(out, mean, std, R, want_spec=False, want_mag_t=True)
    assert all(same_bits(a, b) for a, b in zip(tracks['model'], lib.frames_f0(mag, weight=w, gain=g, lag_min=lo, lag_max=hi)))


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


def _read(path):
    with open(path, 'rb') as f:
        return f.read()


def test_driver_writes_the_f0_file_and_leaves_the_rest(built_lib, tmp_path, capsys):
    """test() with a stop rule and a pitch (`test.py --stop --pitch 3 --f0` on synthetic parameters): prompt_NNN_f0.npy holds one
    (period, strength) row per frame the vocoder was given, one line per prompt gives asked and measured semitones, and every other
    file has the bytes of the run without f0.  With a rate alone: the stretched frame count, and the line in cents."""
    from tacotron_amd import test as drv
    lib = built_lib
    rule = lib.TacoStopRule(**RULE)
    r = _cfg(tmp_path).r
    plain, tracked = tmp_path / 'plain', tmp_path / 'tracked'
    assert drv.test(_cfg(tmp_path), PROMPTS, out_dir=str(plain), n_iter=2, stop=rule, pitch=3.0) == 2
    capsys.readouterr()
    assert drv.test(_cfg(tmp_path), PROMPTS, out_dir=str(tracked), n_iter=2, stop=rule, pitch=3.0, f0=True) == 2
    out = capsys.readouterr().out
    for i in range(2):
        assert ('prompt %d pitch: asked +3.00, measured ' % i) in out
    names = sorted(p.name for p in plain.iterdir())
    assert sorted(p.name for p in tracked.iterdir()) == sorted(names + ['prompt_%03d_f0.npy' % i for i in range(2)])
    for name in names:
        assert _read(tracked / name) == _read(plain / name), name
    for i in range(2):
        got = np.load(tracked / ('prompt_%03d_f0.npy' % i))
        assert got.dtype == np.float32 and got.shape == (8 * r, 2) and np.isfinite(got).all()
        assert ((got[:, 0] == 0) == (got[:, 1] == 0)).all() and ((got[:, 0] == 0) | ((got[:, 0] >= 39.5) & (got[:, 0] <= 266.5))).all()
    slow = tmp_path / 'slow'
    assert drv.test(_cfg(tmp_path), PROMPTS, out_dir=str(slow), n_iter=2, stop=rule, rate=0.8, f0=(80.0, 300.0)) == 2
    out = capsys.readouterr().out
    assert 'prompt 1 rate 0.800: mean log-F0 moved ' in out and 'pitch: asked' not in out
    for i in range(2):
        got = np.load(slow / ('prompt_%03d_f0.npy' % i))
        assert got.shape == (int(np.load(slow / ('prompt_%03d_rate.npy' % i))[1]), 2)
        assert ((got[:, 0] == 0) | ((got[:, 0] >= 52.5) & (got[:, 0] <= 200.5))).all()
    with pytest.raises(ValueError, match='f0'):
        drv.test(_cfg(tmp_path), PROMPTS, out_dir=str(tmp_path / 'x'), n_iter=2, f0=True, vocode=False)


def test_driver_f0_with_long_prompts(built_lib, tmp_path, capsys):
    """--long: one _f0.npy per piece, and the joined audio is that of the run without f0"""
    from tacotron_amd import test as drv
    rule = built_lib.TacoStopRule(**RULE)
    plain, tracked = tmp_path / 'plain', tmp_path / 'tracked'
    kw = dict(n_iter=2, stop=rule, long=True, pitch=[4, -2.5], rate=1.25)
    assert drv.test(_cfg(tmp_path), [PROMPTS[0], LONG], out_dir=str(plain), **kw) == 2
    capsys.readouterr()
    assert drv.test(_cfg(tmp_path), [PROMPTS[0], LONG], out_dir=str(tracked), f0=True, **kw) == 2
    out = capsys.readouterr().out
    assert 'prompt 0 pitch: asked +4.00, measured ' in out and 'prompt 1 piece 2 pitch: asked -2.50, measured ' in out
    names = sorted(p.name for p in plain.iterdir())
    extra = sorted(set(p.name for p in tracked.iterdir()) - set(names))
    assert extra and all(n.endswith('_f0.npy') for n in extra) and 'prompt_000_f0.npy' in extra and 'prompt_001_k00_f0.npy' in extra
    assert len(extra) == sum(n.endswith('_rate.npy') for n in names)
    for name in names:
        assert _read(tracked / name) == _read(plain / name), name
    for name in extra:
        rate = np.load(tracked / name.replace('_f0.npy', '_rate.npy'))
        assert np.load(tracked / name).shape == (int(rate[1]), 2)


@pytest.mark.parametrize('f0', [None, True], ids=['plain', 'f0'])
def test_driver_long_prompts_in_two_groups(built_lib, tmp_path, capsys, monkeypatch, f0):
    """--long with more pieces than one join call takes (JOIN_GROUP lowered to 2: prompts 0 and 1 make the first group, prompt 2 the
    second): every prompt's files are written, with and without f0, and the f0 lines of the second group carry its own labels"""
    from tacotron_amd import test as drv
    monkeypatch.setattr(drv, 'JOIN_GROUP', 2)
    rule = built_lib.TacoStopRule(**RULE)
    out_dir = tmp_path / 'out'
    kw = dict(f0=True, pitch=2.0) if f0 else {}
    assert drv.test(_cfg(tmp_path), [PROMPTS[0], LONG, PROMPTS[1]], out_dir=str(out_dir), n_iter=2, stop=rule, long=True, **kw) == 3
    out = capsys.readouterr().out
    names = set(p.name for p in out_dir.iterdir())
    assert {'prompt_000.wav', 'prompt_001.wav', 'prompt_002.wav', 'prompt_001_pieces.npy', 'prompt_001_k02_spec.npy', 'prompt_002_spec.npy'} <= names
    assert ('prompt_002_f0.npy' in names) == bool(f0) and ('prompt_001_k00_f0.npy' in names) == bool(f0)
    if f0:
        for who in ('prompt 0', 'prompt 1 piece 0', 'prompt 1 piece 2', 'prompt 2'):
            assert (who + ' pitch: asked +2.00, measured ') in out
    else:
        assert 'pitch: asked' not in out


def test_evaluate_f0(built_lib, tmp_path, capsys):
    """evaluate --f0 on a small corpus on disk: the six columns of the plain run unchanged, six more behind them, the recording's from
    lib.frames_f0 on the stored stft frames"""
    from tacotron_amd import evaluate as ev
    from tacotron_amd.config import Config
    from tests.test_gpu_frame_dtw import write_corpus
    frames, _ = write_corpus(str(tmp_path / 'data'))

    def cfg():
        c = Config()
        c.data_path = str(tmp_path / 'data') + '/'
        c.batch_size, c.max_decode_iter = 3, 12
        return c

    plain, _ = ev.evaluate(cfg(), 5, cepstra=13, out_dir=str(tmp_path / 'plain'))
    capsys.readouterr()
    rows, _ = ev.main(['--holdout', '5', '--cepstra', '13', '--f0', '--out-dir', str(tmp_path / 'f0')], config=cfg())
    out = capsys.readouterr().out
    assert plain.shape == (5, 6) and rows.shape == (5, 12) and np.array_equal(rows[:, :6], plain, equal_nan=True)
    assert np.array_equal(np.load(tmp_path / 'f0' / 'eval_0.npy'), rows, equal_nan=True)
    assert out.count('pitch level') == 3 and 'not aligned' in out
    share = rows[:, [8, 11]]
    assert (np.isnan(share) | ((share >= 0) & (share <= 1))).all() and not np.isnan(share[:, 1]).any()
    voiced = rows[:, 11] > 0
    assert (np.isnan(rows[~voiced, 9])).all() and ((rows[voiced, 9] >= np.log2(16000 / 266.5)) & (rows[voiced, 9] <= np.log2(16000 / 39.5))).all()
