"""GPU: the smoothed pitch track through the host layers -- griffinlim.invert_spectrogram(f0={'smooth': ...}), the driver's `f0_smooth`
and evaluate's -- held to lib.frames_f0 / lib.f0_viterbi / lib.f0_stats on the same frames, and bit for bit to the same calls without
it: smoothing changes the tracks it is asked to smooth and nothing else."""
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


@pytest.mark.parametrize('pitch, rate', [(None, None), (3.0, 0.5)], ids=['plain', 'pitch_rate'])
@pytest.mark.parametrize('with_lengths', [False, True], ids=['full', 'lengths'])
@pytest.mark.parametrize('smooth', [True, dict(candidates=2, jump_cost=0.5, switch_cost=0.25, threshold=0.1)], ids=['defaults', 'own'])
def test_smooth_adds_its_tracks_and_changes_nothing_else(built_lib, frames, smooth, with_lengths, pitch, rate):
    from tacotron_amd.griffinlim import invert_spectrogram
    lib = built_lib
    out, mean, std = frames
    lengths = dev(LENGTHS, torch.int32) if with_lengths else None
    kw = dict(n_iter=2, seed=5, lengths=lengths, rate=rate, pitch=pitch)
    raw = invert_spectrogram(out, mean, std, R, f0=dict(threshold=0.0), **kw)
    got = invert_spectrogram(out, mean, std, R, f0=dict(threshold=0.0, smooth=smooth), **kw)
    torch.cuda.synchronize()
    assert len(got) == len(raw) and all(same_bits(a, b) for a, b in zip(raw[:-1], got[:-1]))   # the waveform (and frames_out)
    tracks, plain = got[-1], raw[-1]
    per = R if with_lengths else 1
    w, g, lo, hi = lib.f0_tables()
    opt = dict(weight=dev(w), gain=dev(g), lag_min=lo, lag_max=hi, threshold=0.0)
    bias, lg, jump, switch = lib.f0_viterbi_tables()
    vopt = dict(lag_min=lo, lag_max=hi, bias=dev(bias), lg=dev(lg), threshold=0.0, jump_cost=jump, switch_cost=switch)
    if smooth is not True:
        vopt.update(smooth)
    mag = lib.denorm_unframe(out, mean, std, R, want_spec=False, want_mag_t=True)
    stages = [('model', mag, lengths, per)]
    if pitch is not None:
        last = lib.frames_pitch(mag, lengths, lib.pitch_step(pitch), frames_per_unit=per)
        stages.append(('pitched', last, lengths, per))
        stretched, n = lib.frames_stretch(last, lengths, lib.stretch_step(rate), frames_per_unit=per, Fo=max(5, lib.stretch_capacity(F, 32768)))
        stages.append(('vocoder', stretched, n, 1))
    for name, x, counts, unit in stages:
        p, s, acf = lib.frames_f0(x, counts, unit, want_acf=True, **opt)
        want = lib.f0_viterbi(acf, counts, unit, **vopt)
        assert all(same_bits(a, b) for a, b in zip(tracks[name], want[:2])), name
        assert torch.equal(tracks[name + '_counts'], want[2]), name
        assert same_bits(tracks[name + '_raw'][0], p) and same_bits(tracks[name + '_raw'][1], s), name
        assert all(same_bits(a, b) for a, b in zip(tracks[name + '_raw'], plain[name])), name     # the bits of the run without 'smooth'
        assert same_bits(tracks[name + '_stats'], lib.f0_stats(want[0], None, counts, unit)), name
    if pitch is not None:
        assert same_bits(tracks['pitch_stats'], lib.f0_stats(tracks['pitched'][0], tracks['model'][0], lengths, per))
    else:
        assert tracks['vocoder'] is tracks['model'] and tracks['vocoder_counts'] is tracks['model_counts']
        assert tracks['vocoder_raw'] is tracks['model_raw']
    assert not any(k.endswith('_raw') or k.endswith('_counts') for k in plain)
    frames_b = tracks['model_counts'][:, 0].tolist()
    assert frames_b == ([16, 10] if with_lengths else [16, 16])
    with pytest.raises(ValueError, match='smooth'):
        invert_spectrogram(out, mean, std, R, n_iter=1, f0=dict(smooth=dict(ratio=0.9)))


# ---- the synthesis driver ------------------------------------------------------------------------------------------------------------
RULE = dict(end_offset=200, hold=1, min_steps=5)   # target 0: every row stops after step 4 -> len_b = 8
PROMPTS = ['hello world.\n', 'a somewhat longer prompt, with punctuation!\n']


def _cfg(tmp_path):
    from tacotron_amd.config import Config
    c = Config()
    c.data_path = str(tmp_path / 'no_data') + '/'
    c.max_decode_iter = 16
    return c


def _read(path):
    with open(path, 'rb') as f:
        return f.read()


def test_driver_smooths_the_f0_file_and_leaves_the_rest(built_lib, tmp_path, capsys):
    """test() with `f0_smooth`: every file but _f0.npy has the bytes of the `f0` run, _f0.npy keeps its shape, and every prompt's line
    names the frames the smoothing moved; with K = 1 and the same threshold nothing can move"""
    from tacotron_amd import test as drv
    lib = built_lib
    rule = lib.TacoStopRule(**RULE)
    r = _cfg(tmp_path).r
    raw, smooth, plain = tmp_path / 'raw', tmp_path / 'smooth', tmp_path / 'plain'
    assert drv.test(_cfg(tmp_path), PROMPTS, out_dir=str(raw), n_iter=2, stop=rule, pitch=3.0, f0=True) == 2
    capsys.readouterr()
    assert drv.test(_cfg(tmp_path), PROMPTS, out_dir=str(smooth), n_iter=2, stop=rule, pitch=3.0, f0=True, f0_smooth=True) == 2
    out = capsys.readouterr().out
    names = sorted(p.name for p in raw.iterdir())
    assert sorted(p.name for p in smooth.iterdir()) == names
    for name in names:
        if not name.endswith('_f0.npy'):
            assert _read(smooth / name) == _read(raw / name), name
    for i in range(2):
        line = [x for x in out.splitlines() if x.startswith('prompt %d pitch: asked +3.00, measured ' % i)]
        assert len(line) == 1 and line[0].endswith(' of %d frames' % (8 * r)) and ', smoothing moved ' in line[0]
        got = np.load(smooth / ('prompt_%03d_f0.npy' % i))
        assert got.dtype == np.float32 and got.shape == (8 * r, 2) and np.isfinite(got).all()
        assert ((got[:, 0] == 0) == (got[:, 1] == 0)).all() and ((got[:, 0] == 0) | ((got[:, 0] >= 39.5) & (got[:, 0] <= 266.5))).all()
    assert drv.test(_cfg(tmp_path), PROMPTS, out_dir=str(plain), n_iter=2, stop=rule, f0=True, f0_smooth=3) == 2
    out = capsys.readouterr().out
    assert all(('prompt %d f0: smoothing moved ' % i) in out for i in range(2)) and 'pitch: asked' not in out
    for bad in (dict(f0_smooth=True), dict(f0=True, f0_smooth=0), dict(f0=True, f0_smooth=16), dict(f0=True, f0_smooth=2.5)):
        with pytest.raises(ValueError, match='f0_smooth'):
            drv.test(_cfg(tmp_path), PROMPTS, out_dir=str(tmp_path / 'x'), n_iter=2, **bad)
    a = drv.parse_args(['--f0-smooth', '--f0-candidates', '6'])
    assert a.f0 is True and a.f0_smooth == 6 and drv.parse_args(['--f0-smooth']).f0_smooth is True and drv.parse_args(['--f0']).f0_smooth is None
    for bad in (['--f0-candidates', '3'], ['--f0-smooth', '--f0-candidates', '16'], ['--f0', '--f0-candidates', '3']):
        with pytest.raises(SystemExit):
            drv.parse_args(bad)


# ---- evaluate ------------------------------------------------------------------------------------------------------------------------
def test_evaluate_f0_smooth(built_lib, tmp_path, capsys):
    """evaluate --f0-smooth --f0-aligned on the small corpus on disk: SMOOTH_COLUMNS behind every other column; the columns that do not
    come from a pitch track have the bits of the run without it; the per-frame tracks underneath are those of that run, and the F0
    columns are lib.f0_stats of the smoothed ones"""
    from tacotron_amd import evaluate as ev
    from tacotron_amd.config import Config
    from tests.test_gpu_frame_dtw import write_corpus
    lib = built_lib
    write_corpus(str(tmp_path / 'data'))

    def cfg():
        c = Config()
        c.data_path = str(tmp_path / 'data') + '/'
        c.batch_size, c.max_decode_iter = 3, 12
        return c

    before, after = [], []
    plain, _ = ev.evaluate(cfg(), 5, cepstra=13, out_dir=str(tmp_path / 'plain'), f0_aligned=True, trace=before)
    out = capsys.readouterr().out
    assert 'smoothing' not in out and plain.shape == (5, 17)
    rows, _ = ev.evaluate(cfg(), 5, cepstra=13, out_dir=str(tmp_path / 'smooth'), f0_aligned=True, f0_smooth=True, trace=after)
    out = capsys.readouterr().out
    assert ev.SMOOTH_COLUMNS == ('f0_moved', 'rec_f0_moved') and rows.shape == (5, 19)
    assert np.array_equal(np.load(tmp_path / 'smooth' / 'eval_0.npy'), rows, equal_nan=True)
    assert np.array_equal(rows[:, :6].view(np.uint64), plain[:, :6].view(np.uint64))           # index, na, nb, steps, cost, mcd
    assert out.count('smoothing moved') == 3 and out.count('pitch level') == 3 and out.count('along the warping path') == 3
    share = rows[:, 17:]
    assert (np.isnan(share) | ((share >= 0) & (share <= 1))).all() and not np.isnan(share[:, 1]).any()
    w, g, lo, hi = lib.f0_tables()
    for a, b in zip(before, after):
        # the per-frame tracks are what the run without smoothing tracked ...
        assert np.array_equal(b['period_raw'].view(np.uint32), a['period'].view(np.uint32))
        assert np.array_equal(b['rec_period_raw'].view(np.uint32), a['rec_period'].view(np.uint32))
        # ... and the smoothed ones keep to the lags and to the rows' own frames
        for key, n in (('period', np.minimum(b['na'], b['period'].shape[1])), ('rec_period', b['nb'])):
            p = b[key]
            assert ((p == 0) | ((p >= lo - 0.5) & (p <= hi + 0.5))).all()
            assert all(not p[i, int(n[i]):].any() for i in range(len(n)))
    # the F0 columns are the statistics of the smoothed tracks
    got = np.concatenate([lib.f0_stats(dev(b['rec_period']), None, dev(b['nb'], torch.int32), 1).cpu().numpy() for b in after])[[0, 1, 2, 3, 4]]
    want = ev.f0_columns(got, rows[:, 2])
    assert np.array_equal(rows[:, 9:12], want, equal_nan=True)
    r2, _ = ev.main(['--holdout', '5', '--cepstra', '13', '--f0-smooth', '--out-dir', str(tmp_path / 'cli')], config=cfg())
    assert r2.shape == (5, 14) and np.array_equal(r2[:, 12:], rows[:, 17:], equal_nan=True) and np.array_equal(r2[:, :12], rows[:, :12], equal_nan=True)
