"""GPU: spectral sharpening through the host layers -- griffinlim.invert_spectrogram(sharpen=...), the driver's --sharpen
(Config.sharpen) and evaluate --gv --sharpen -- held bit for bit to the same calls without it (beta 0), to lib.frames_sharpen in front
of the vocoder's entry points, and evaluate's columns to the restatement (tests/sharpen_ref.py) on the magnitudes it traced."""
import wave as wavefile

import numpy as np
import pytest
import torch

from tests import sharpen_ref as sr

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
@pytest.mark.parametrize('with_lengths', [False, True], ids=['full', 'lengths'])
def test_beta_zero_is_the_call_without_sharpening(built_lib, frames, with_lengths, rate):
    from tacotron_amd.griffinlim import invert_spectrogram
    out, mean, std = frames
    kw = dict(n_iter=3, seed=5, lengths=dev(LENGTHS, torch.int32) if with_lengths else None, rate=rate, pitch=2.0)
    plain = invert_spectrogram(out, mean, std, R, **kw)
    zero = invert_spectrogram(out, mean, std, R, sharpen=0.0, **kw)
    sharp = invert_spectrogram(out, mean, std, R, sharpen=0.4, **kw)
    torch.cuda.synchronize()
    plain, zero, sharp = ((x,) if rate is None else tuple(x) for x in (plain, zero, sharp))
    assert len(plain) == len(zero) == len(sharp) == 1 + (rate is not None)
    for a, b in zip(plain, zero):
        assert a.dtype == b.dtype and same_bits(a, b)
    assert bool(plain[0].abs().max() > 0)
    assert sharp[0].shape == plain[0].shape and not same_bits(sharp[0], plain[0])     # no return shape changes; the samples do
    if rate is not None:
        assert torch.equal(sharp[-1], plain[-1])                                       # frames_out: the duration is the rate's alone


def test_sharpen_is_frames_sharpen_in_front_of_everything(built_lib, frames):
    """behind the de-normalisation and in front of the pitch, the stretch and the F0 tracks"""
    from tacotron_amd.griffinlim import invert_spectrogram, vocode
    lib = built_lib
    out, mean, std = frames
    lengths = dev(LENGTHS, torch.int32)
    mag = lib.denorm_unframe(out, mean, std, R, want_spec=False, want_mag_t=True)
    sharp = lib.frames_sharpen(mag, 0.4, 24, lengths, R)
    assert not sharp[1, :, 10:].any() and bool((sharp[1, :, :10] > 0).all())
    want = lib.griffinlim_rows(sharp, lengths, seed=7, n_iter=2, frames_per_unit=R)
    assert same_bits(invert_spectrogram(out, mean, std, R, n_iter=2, seed=7, lengths=lengths, sharpen=0.4, sharpen_lifter=24), want)
    # with a pitch and a rate: sharpen, shift, stretch
    shifted = lib.frames_pitch(sharp, lengths, [lib.pitch_step(3.0)] * B, frames_per_unit=R, lifter=32)
    stretched, n = lib.frames_stretch(shifted, lengths, 32768, frames_per_unit=R, Fo=lib.stretch_capacity(F, 32768))
    want = lib.griffinlim_rows(stretched, n, seed=7, n_iter=2)
    v = vocode(out, mean, std, R, n_iter=2, seed=7, lengths=lengths, sharpen=0.4, sharpen_lifter=24, pitch=3.0, rate=0.5, f0=True)
    assert same_bits(v.waveform, want) and v.frames_out.tolist() == n.tolist()
    # the 'model' track is measured on the sharpened frames
    w, g, lag_min, lag_max = lib.f0_tables(C=1025)
    period = lib.frames_f0(sharp, lengths, R, weight=dev(w), gain=dev(g), lag_min=lag_min, lag_max=lag_max)[0]
    assert same_bits(v.tracks['model'][0], period)
    # without lengths: all F frames
    full = lib.frames_sharpen(mag, -0.5)
    v = vocode(out, mean, std, R, n_iter=0, seed=7, sharpen=-0.5, phase_init='estimate')
    assert same_bits(v.waveform, lib.griffinlim(full, lib.phase_estimate(full), 0))
    for bad in (dict(sharpen=1.5), dict(sharpen=float('nan')), dict(sharpen=0.4, sharpen_lifter=1), dict(sharpen=0.4, sharpen_lifter=65)):
        with pytest.raises(ValueError):
            invert_spectrogram(out, mean, std, R, n_iter=2, **bad)


# ---- the driver --------------------------------------------------------------------------------------------------------------------
RULE = dict(end_offset=200, hold=1, min_steps=5)   # target 0: every row stops after step 4 -> len_b = 8
PROMPTS = ['hello world.\n', 'a somewhat longer prompt, with punctuation!\n']
LONG = ('the first sentence of this prompt is long enough to fill a good part of one piece on its own, and it ends here. '
        'the second one has no full stop for a long while, only a comma after a run of words that goes on and on and on, '
        'and then more words that follow the comma until the line has well over three hundred characters in it.\n')


def _cfg(tmp_path, sharpen=None, lifter=32):
    from tacotron_amd.config import Config
    c = Config()
    c.data_path = str(tmp_path / 'no_data') + '/'
    c.max_decode_iter = 16
    c.sharpen, c.sharpen_lifter = sharpen, lifter
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
    for name in ('frames_sharpen', 'frames_pitch', 'frames_stretch'):
        def spy(mag_t, *a, _real=getattr(lib, name), _name=name, **k):
            seen.append((_name, tuple(mag_t.shape), a, k))
            return _real(mag_t, *a, **k)
        monkeypatch.setattr(lib, name, spy)
    return seen


def test_driver_writes_the_sharpen_file_and_leaves_the_rest(built_lib, tmp_path, monkeypatch):
    """test() with Config.sharpen = 0.4: prompt_NNN_sharpen.npy = (beta, lifter) and another wav; every other file has the name, size
    and -- the model's own files -- the bytes of the run without it; sharpen 0 is the run without it, byte for byte, file for file"""
    from tacotron_amd import test as drv
    lib = built_lib
    seen = _spies(lib, monkeypatch)
    rule = lib.TacoStopRule(**RULE)
    r = _cfg(tmp_path).r
    plain, sharp, zero = tmp_path / 'plain', tmp_path / 'sharp', tmp_path / 'zero'
    assert drv.test(_cfg(tmp_path), PROMPTS, out_dir=str(plain), n_iter=2, stop=rule) == 2
    assert not seen
    assert drv.test(_cfg(tmp_path, 0.4, 24), PROMPTS, out_dir=str(sharp), n_iter=2, stop=rule) == 2
    assert [(s[0], s[1]) for s in seen] == [('frames_sharpen', (2, 1025, 16 * r))]
    assert seen[0][2][:2] == (0.4, 24) and seen[0][2][2] is None                          # (no lengths: all frames, as the vocoder)
    del seen[:]
    assert drv.test(_cfg(tmp_path, 0.0), PROMPTS, out_dir=str(zero), n_iter=2, stop=rule) == 2
    assert not seen
    names = sorted(p.name for p in plain.iterdir())
    assert names == sorted('prompt_%03d%s' % (i, s) for i in range(2) for s in ('.wav', '_spec.npy', '_align.npy', '_len.npy'))
    assert sorted(p.name for p in zero.iterdir()) == names
    assert sorted(p.name for p in sharp.iterdir()) == sorted(names + ['prompt_%03d_sharpen.npy' % i for i in range(2)])
    for name in names:
        assert _read(zero / name) == _read(plain / name), name
        if name.endswith('.npy'):
            assert _read(sharp / name) == _read(plain / name), name
        else:
            assert _wav(sharp / name)[0] == _wav(plain / name)[0] > 0 and _wav(sharp / name)[1] != _wav(plain / name)[1]
    for i in range(2):
        got = np.load(sharp / ('prompt_%03d_sharpen.npy' % i))
        assert got.dtype == np.float64 and got.tolist() == [0.4, 24.0]
    with pytest.raises(ValueError, match='sharpen'):
        drv.test(_cfg(tmp_path, 0.4), PROMPTS, out_dir=str(tmp_path / 'x'), n_iter=2, vocode=False)
    with pytest.raises(ValueError, match='sharpen'):
        drv.test(_cfg(tmp_path, -1.5), PROMPTS, out_dir=str(tmp_path / 'x'), n_iter=2)


def test_driver_combines_with_stop_pitch_and_rate_and_long(built_lib, tmp_path, monkeypatch):
    """--stop --pitch --rate --sharpen: the post-filter runs first, over each row's own frames; the other files are those of the run
    without it; with `long` every piece is sharpened and writes its own _sharpen.npy"""
    from tacotron_amd import test as drv
    lib = built_lib
    seen = _spies(lib, monkeypatch)
    rule = lib.TacoStopRule(**RULE)
    r = _cfg(tmp_path).r
    common = dict(n_iter=2, stop=rule, pitch=3.0, rate=0.8)
    plain, sharp = tmp_path / 'plain', tmp_path / 'sharp'
    assert drv.test(_cfg(tmp_path), PROMPTS, out_dir=str(plain), **common) == 2
    assert [s[0] for s in seen] == ['frames_pitch', 'frames_stretch']
    del seen[:]
    assert drv.test(_cfg(tmp_path, -0.5), PROMPTS, out_dir=str(sharp), **common) == 2
    assert [s[0] for s in seen] == ['frames_sharpen', 'frames_pitch', 'frames_stretch']
    beta, lifter, counts, per_unit = seen[0][2]
    assert (beta, lifter, counts.tolist(), per_unit) == (-0.5, 32, [8, 8], r)
    names = sorted(p.name for p in plain.iterdir())
    assert sorted(p.name for p in sharp.iterdir()) == sorted(names + ['prompt_%03d_sharpen.npy' % i for i in range(2)])
    for name in names:
        if name.endswith('.npy'):
            assert _read(sharp / name) == _read(plain / name), name
        else:
            assert _wav(sharp / name)[0] == _wav(plain / name)[0] > 0 and _wav(sharp / name)[1] != _wav(plain / name)[1]
    del seen[:]
    out = tmp_path / 'long'
    assert drv.test(_cfg(tmp_path, 0.4), [PROMPTS[0], LONG], out_dir=str(out), n_iter=2, stop=rule, long=True) == 2
    K = len(list(out.glob('prompt_001_k*_spec.npy')))
    assert K >= 2 and [s[0] for s in seen] == ['frames_sharpen'] and seen[0][1][0] == 1 + K      # one batch: every piece a row
    assert np.load(out / 'prompt_000_sharpen.npy').tolist() == [0.4, 32.0]
    for k in range(K):
        assert np.load(out / ('prompt_001_k%02d_sharpen.npy' % k)).tolist() == [0.4, 32.0]
    assert not (out / 'prompt_001_sharpen.npy').exists() and _wav(out / 'prompt_001.wav')[0] > 0


# ---- evaluate ------------------------------------------------------------------------------------------------------------------------
def test_evaluate_gv_columns_and_lines(built_lib, tmp_path, capsys):
    """evaluate(gv=True, sharpen=0.4) on the synthetic pool: the two GV columns behind the columns of the run without it, which stay
    what they were, the added lines, and the columns against the restatement on the traced magnitudes.  The bound on a ratio is the
    restatement's own: 4 times the float32 restatement's error of a variance on these very magnitudes (the convention of
    sharpen_ref.CEPSTATS_RTOL), predicted plus recorded; the sharpened magnitudes themselves are held to SHARPEN_RTOL."""
    from tacotron_amd import evaluate as ev
    from tacotron_amd.config import Config

    def cfg():
        c = Config()
        c.data_path = str(tmp_path / 'no_data') + '/'
        c.batch_size, c.max_decode_iter = 3, 12
        return c

    plain, loss = ev.evaluate(cfg(), 5, out_dir=str(tmp_path / 'plain'), f0=True)
    plain_out = capsys.readouterr().out.splitlines()
    only, _ = ev.evaluate(cfg(), 5, out_dir=str(tmp_path / 'gv'), f0=True, gv=True)
    only_out = capsys.readouterr().out.splitlines()
    solo, _ = ev.evaluate(cfg(), 5, out_dir=str(tmp_path / 'solo'), gv=True, gv_lifter=32)       # without --f0: the same magnitudes
    capsys.readouterr()
    assert solo.shape == (5, 7) and np.array_equal(solo[:, 6].view(np.uint64), only[:, 12].view(np.uint64))
    trace = []
    rows, loss2 = ev.main(['--holdout', '5', '--f0', '--gv', '--sharpen', '0.4', '--out-dir', str(tmp_path / 'both')], config=cfg())
    out = capsys.readouterr().out.splitlines()
    again, _ = ev.evaluate(cfg(), 5, out_dir=str(tmp_path / 'both'), f0=True, gv=True, sharpen=0.4, trace=trace)
    capsys.readouterr()
    Q = 32
    assert plain.shape == (5, 12) and only.shape == (5, 13) and rows.shape == (5, 14) and loss2 == loss
    assert np.array_equal(rows[:, :12].view(np.uint64), plain.view(np.uint64)) and np.array_equal(only[:, :12].view(np.uint64), plain.view(np.uint64))
    assert np.array_equal(rows[:, 12].view(np.uint64), only[:, 12].view(np.uint64)) and np.array_equal(again.view(np.uint64), rows.view(np.uint64))
    assert np.array_equal(np.load(tmp_path / 'both' / 'eval_0.npy'), rows, equal_nan=True)
    added = [line for line in out if 'GV ratio' in line]
    assert len(added) == 3 and added[0].startswith('batch 0 GV ratio') and added[1].startswith('batch 1 GV ratio')
    assert added[2].startswith('held out: GV ratio') and all(', with --sharpen 0.40: ' in line for line in added) and out.index(added[2]) == len(out) - 2
    assert [line for line in out if line not in added] == plain_out                          # nothing else changed
    assert [line for line in only_out if 'GV ratio' not in line] == plain_out and sum('GV ratio' in line for line in only_out) == 3
    assert not any('--sharpen' in line for line in only_out)
    want, k = [], 0
    for t, valid in zip(trace, (3, 2)):
        pm, rm = t['pred_mags'], t['rec_mags']
        npred, nrec = np.minimum(t['lengths'].astype(np.int64) * 2, pm.shape[2]), t['nb']
        assert pm.shape[1] == rm.shape[1] == 1025 and np.array_equal(npred, np.minimum(t['na'], pm.shape[2]))
        sharp = sr.sharpen(pm, 0.4, npred, 1, 32)
        err = sr.rel_err(t['sharp_mags'], sharp)
        print('  batch: sharpened magnitudes within %.3g of the restatement (bound %.3g)' % (err, sr.SHARPEN_RTOL))
        assert err <= sr.SHARPEN_RTOL
        sums = {name: sr.cepstats(m, n, 1, Q) for name, m, n in (('pred', pm, npred), ('rec', rm, nrec), ('sharp', t['sharp_mags'], npred))}
        tol = 0.0
        for name, m, n in (('pred', pm, npred), ('rec', rm, nrec), ('sharp', t['sharp_mags'], npred)):
            s32, n32 = sr.cepstats(m, n, 1, Q, dtype=np.float32)
            e = sr.var_err(s32, n32, *sums[name])
            print('  batch: %s: float32 restatement error of a variance %.3g' % (name, e))
            tol = max(tol, 4.0 * e)
        for col, name in ((12, 'pred'), (13, 'sharp')):
            ref = sr.gv_ratio(sums[name][0], sums[name][1], sums['rec'][0], sums['rec'][1])[:valid]
            got = rows[k:k + valid, col]
            print('  batch: column %d %s, restatement %s (bound %.3g)' % (col, got, ref, 2.0 * tol))
            assert np.array_equal(np.isnan(got), np.isnan(ref))
            ok = ~np.isnan(ref)
            assert (np.abs(got[ok] / ref[ok] - 1.0) <= 2.0 * tol).all()
        k += valid
    assert k == 5
