"""GPU: the intonation range through the host layers -- griffinlim.vocode(intonation=...) and the driver's --pitch-range
(Config.pitch_range) -- held bit for bit to the same calls made by hand and to the calls without it (None, 1.0), and the closed loop:
the deviation of log2 F0 the tracker measures behind the stage against the one in front of it, compared with what the float64
restatement chain (tests/f0_ref.py, tests/f0_range_ref.py, tests/pitch_ref.py) gives on the same frames."""
import wave as wavefile

import numpy as np
import pytest
import torch

from tests import f0_range_ref as rr
from tests import f0_ref
from tests import pitch_ref as pr

pytestmark = pytest.mark.gpu

R, TD, B = 2, 16, 2
F = (TD // 4) * 4 * R          # 32 frames
LENGTHS = (16, 12)             # decoder steps -> 32 and 24 frames
GAP = slice(9, 13)             # frames without a pitch


def dev(x, dtype=torch.float32):
    return torch.as_tensor(np.asarray(x), dtype=dtype).cuda()


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def contour(n, phase, centre, amp):
    """n periods in samples: a slow sinusoid of log2(period), one and a quarter cycles over the row"""
    return 2.0 ** (centre + amp * np.sin(2.0 * np.pi * (1.25 * np.arange(n) / n + phase)))


def voiced_frames(C, periods, seed, gap=GAP, fill=1e-6):
    """(C, n) float32 magnitudes: frame f a harmonic comb (pitch_ref.comb) of period periods[f] samples at N = 2 (C - 1), the frames
    of `gap` flat at `fill`: no harmonics, so no interior maximum of the autocorrelation and no pitch (seeded noise frames would
    be tracked as voiced at arbitrary periods)"""
    N = 2 * (C - 1)
    x = np.stack([pr.comb(C, 1, spacing=N / p, seed=seed + f)[0][:, 0] for f, p in enumerate(periods)], axis=1)
    x[:, gap] = fill
    return x.astype(np.float32)


@pytest.fixture(scope='module')
def frames(built_lib):
    """(out, mean, std, mag): a model output (B, Td, 1025 r) whose de-normalised frames are combs along a sinusoidal F0 contour
    around 125 Hz with an unvoiced gap, in whatever order the r-frame layout wants them (read off lib.denorm_unframe on a tagged
    input), the neutral statistics, and the magnitudes (B, 1025, F) themselves"""
    lib = built_lib
    C = 1025
    mag = np.stack([voiced_frames(C, contour(F, 0.1 + 0.3 * b, 7.0, 0.3), seed=40 * b) for b in range(B)])      # (B, C, F)
    tags = torch.arange(TD * R * C, dtype=torch.float32).view(1, TD, R * C).cuda()
    mean, std = torch.zeros(R * C, device='cuda'), torch.ones(R * C, device='cuda')
    src = lib.denorm_unframe(tags, mean, std, R)[0].cpu().numpy().astype(np.int64)                               # (F, C): flat source index
    out = np.zeros((B, TD * R * C), dtype=np.float32)
    out[:, src.ravel()] = np.log(mag).transpose(0, 2, 1).reshape(B, -1)
    out = dev(out.reshape(B, TD, R * C))
    got = lib.denorm_unframe(out, mean, std, R, want_spec=False, want_mag_t=True)
    assert np.allclose(got.cpu().numpy(), mag, rtol=1e-5)
    return out, mean, std, got


def test_intonation_is_the_calls_made_by_hand(built_lib, frames):
    """vocode(intonation=1.5, f0=True): the 'model' track, lib.f0_range_curve on it, lib.frames_pitch_curve, the 'pitched' track, and
    range_stats from the two summaries; the waveform is that of vocode(pitch_curve=<the curve made by hand>)"""
    from tacotron_amd.griffinlim import invert_spectrogram, vocode
    lib = built_lib
    out, mean, std, mag = frames
    lengths = dev(LENGTHS, torch.int32)
    w, g, lag_min, lag_max = lib.f0_tables(C=1025)
    tab = dict(weight=dev(w), gain=dev(g), lag_min=lag_min, lag_max=lag_max)
    period = lib.frames_f0(mag, lengths, R, **tab)[0]
    assert int((period[0] > 0).sum()) == F - 4 and int((period[1] > 0).sum()) == 24 - 4      # the combs are tracked, the gap is not
    curve, stats = lib.f0_range_curve(period, lengths, R, [lib.range_scale(1.5)] * B, None, 2, 0.5, want_stats=True)
    assert bool((curve != lib.PITCH_ONE).any())
    moved = lib.frames_pitch_curve(mag, lengths, curve, frames_per_unit=R, lifter=32)
    behind = lib.frames_f0(moved, lengths, R, **tab)[0]
    s_in, s_out = lib.f0_stats(period, None, lengths, R), lib.f0_stats(behind, None, lengths, R)
    assert same_bits(stats, s_in)
    kw = dict(n_iter=2, seed=3, lengths=lengths)
    v = vocode(out, mean, std, R, intonation=1.5, f0=True, **kw)
    by_hand = vocode(out, mean, std, R, pitch_curve=curve, **kw)
    assert same_bits(v.waveform, by_hand.waveform) and same_bits(v.waveform, lib.griffinlim_rows(moved, lengths, seed=3, n_iter=2, frames_per_unit=R))
    assert same_bits(v.tracks['model'][0], period) and same_bits(v.tracks['pitched'][0], behind)
    assert same_bits(v.tracks['model_stats'], s_in) and same_bits(v.tracks['pitched_stats'], s_out)
    want = torch.stack([s_out[:, 0], s_in[:, 2], s_out[:, 2], torch.where(s_in[:, 2] > 0, s_out[:, 2] / s_in[:, 2], torch.zeros_like(s_in[:, 2]))], dim=1)
    assert v.tracks['range_stats'].shape == (B, 4) and same_bits(v.tracks['range_stats'], want)
    # the stage ran with the k it was given: the ratio it reports is the float64 chain's on these frames (1.483 and 1.476 -- not
    # 1.5: the gap's line and the smoothing take their share) to 0.02, a hundred times what the closed-loop test below allows; this
    # one is about the plumbing, that one about the numbers
    ratio = v.tracks['range_stats'][:, 3].cpu().numpy()
    wt, gn, lo, hi = f0_ref.tables()
    for b in range(B):
        a_in, a_out = restated_loop(mag[b:b + 1, :, :LENGTHS[b] * R].cpu().numpy(), 1.5, (lo, hi), 32, wt, gn)
        print('  row %d: asked x1.5, measured x%.4f over %d frames, restated x%.4f over %d' % (b, ratio[b], s_out[b, 0], a_out[2] / a_in[2], a_out[0]))
        assert abs(ratio[b] - a_out[2] / a_in[2]) <= 0.02 and int(s_out[b, 0]) == int(a_out[0])
    # without f0 the frames are tracked once with the default tables: the same waveform, the same return shape
    plain = invert_spectrogram(out, mean, std, R, intonation=1.5, **kw)
    assert torch.is_tensor(plain) and same_bits(plain, v.waveform)
    # a host sequence, a device tensor of scale_q and the stats buffer
    seq = [0.5, 1.5]
    buf = torch.empty(B, 3, device='cuda')
    a = vocode(out, mean, std, R, intonation=seq, intonation_smooth=1, intonation_limit=0.25, intonation_stats=buf, **kw)
    b = vocode(out, mean, std, R, intonation=dev([lib.range_scale(k) for k in seq], torch.int32), intonation_smooth=1, intonation_limit=0.25, **kw)
    c2 = lib.f0_range_curve(period, lengths, R, [lib.range_scale(k) for k in seq], None, 1, 0.25)
    assert same_bits(a.waveform, b.waveform) and same_bits(buf, s_in)
    assert same_bits(a.waveform, vocode(out, mean, std, R, pitch_curve=c2, **kw).waveform)
    # composed with a pitch (broadcast on the device) and with a pitch curve; under 'smooth' the Viterbi track is the one scaled
    base = dev([[lib.pitch_step(2.0)] * F, [lib.pitch_step(-1.0)] * F], torch.int32)
    c3 = lib.f0_range_curve(period, lengths, R, [lib.range_scale(1.5)] * B, base, 2, 0.5)
    want3 = vocode(out, mean, std, R, pitch_curve=c3, **kw).waveform
    assert same_bits(vocode(out, mean, std, R, intonation=1.5, pitch=[2.0, -1.0], **kw).waveform, want3)
    assert same_bits(vocode(out, mean, std, R, intonation=1.5, pitch_curve=base, **kw).waveform, want3)
    vs = vocode(out, mean, std, R, intonation=1.5, f0=dict(smooth=True), **kw)
    c4 = lib.f0_range_curve(vs.tracks['model'][0], lengths, R, [lib.range_scale(1.5)] * B, None, 2, 0.5)
    assert same_bits(vs.waveform, vocode(out, mean, std, R, pitch_curve=c4, **kw).waveform)
    for bad in (dict(intonation=4.5), dict(intonation=-0.1), dict(intonation=float('nan')), dict(intonation=[1.0, 2.0, 3.0]),
                dict(intonation=1.5, intonation_smooth=9), dict(intonation=1.5, intonation_limit=0.0), dict(intonation_stats=buf)):
        with pytest.raises(ValueError):
            vocode(out, mean, std, R, **bad, **kw)


@pytest.mark.parametrize('with_lengths', [False, True], ids=['full', 'lengths'])
def test_none_and_one_are_the_call_without_it(built_lib, frames, with_lengths):
    """intonation None and a plain 1.0 touch nothing, bit for bit, with every other option on"""
    from tacotron_amd.griffinlim import vocode
    out, mean, std, _ = frames
    kw = dict(n_iter=2, seed=5, lengths=dev(LENGTHS, torch.int32) if with_lengths else None, rate=0.8, pitch=2.0, sharpen=0.3, formant=1.0,
              f0=dict(smooth=True), momentum=0.5, want_conv=True, phase_init='estimate')
    plain = vocode(out, mean, std, R, **kw)
    for k in (None, 1.0, 1):
        v = vocode(out, mean, std, R, intonation=k, intonation_smooth=4, intonation_limit=0.25, **kw)
        assert same_bits(v.waveform, plain.waveform) and same_bits(v.conv, plain.conv) and torch.equal(v.frames_out, plain.frames_out)
        assert sorted(v.tracks) == sorted(plain.tracks) and 'range_stats' not in v.tracks
        for name in plain.tracks:
            for x, y in zip(*((t if isinstance(t, tuple) else (t,)) for t in (v.tracks[name], plain.tracks[name]))):
                assert same_bits(x, y), name
    moved = vocode(out, mean, std, R, intonation=1.5, **kw)
    assert not same_bits(moved.waveform, plain.waveform) and 'range_stats' in moved.tracks


# ---- the closed loop at a small bin count ------------------------------------------------------------------------------------------
CL_C, CL_F, CL_Q, CL_LAGS = 129, 48, 12, (24, 110)
CL_GAP = slice(20, 25)


def closed_loop_frames():
    """(1, 129, 48) magnitudes: combs whose period follows a sinusoid of log2 around 2^5.7 = 52 samples (N = 256) with 0.25 octaves of
    amplitude, and five frames of exact zeros (the tracker's r0 > 0 fails: unvoiced in every precision)"""
    return voiced_frames(CL_C, contour(CL_F, 0.2, 5.7, 0.25), seed=7, gap=CL_GAP, fill=0.0)[None]


def restated_loop(x, k, lags=None, Q=None, weight=None, gain=None):
    """the float64 chain on the frames x (1, C, n): f0_ref.track, f0_range_ref.curve, pitch_ref.shift_frames frame by frame,
    f0_ref.track -> (f0_ref.stats in front, behind)"""
    lag_min, lag_max = lags or CL_LAGS
    period = f0_ref.track(x, None, 1, weight, gain, lag_min, lag_max)[0].astype(np.float32)
    step = rr.curve(period, None, 1, (int(round(65536 * k)),), None, rr.SMOOTH, rr.LIMIT)[0]
    moved = np.stack([x[0, :, f] if step[0, f] == rr.ONE else pr.shift_frames(x[0, :, f:f + 1], step[0, f], Q or CL_Q)[:, 0]
                      for f in range(x.shape[2])], axis=1).astype(np.float32)[None]
    behind = f0_ref.track(moved, None, 1, weight, gain, lag_min, lag_max)[0].astype(np.float32)
    return f0_ref.stats(period)[0], f0_ref.stats(behind)[0]


@pytest.fixture(scope='module')
def restated():
    x = closed_loop_frames()
    return x, {k: restated_loop(x, k) for k in (0.0, 0.5, 1.5)}


@pytest.mark.parametrize('k', [0.5, 1.5, 0.0])
def test_the_measured_range_is_the_restated_one(built_lib, restated, k):
    """frames_f0 -> f0_range_curve -> frames_pitch_curve -> frames_f0 -> f0_stats on the device against the float64 restatement chain on
    the same frames.  NOT against k: the tracker's resolution (a parabola through three lags) and the lifter decide how close to k
    one gets.  The restatement's ratios of the deviations on these frames (sd in front 0.16036 octaves over 43 voiced frames):
    k = 0.5: 0.5092 (sd behind 0.08166), k = 1.5: 1.4887 (0.23872), k = 0 (flat): 0.0291 (0.00466).  Margin: F0_STATS_ATOL on each deviation, and on the ratio what those two
    allow, (1 + ratio) F0_STATS_ATOL / sd in front."""
    lib = built_lib
    x, want = restated
    (n_in, _, sd_in), (n_out, _, sd_out) = want[k]
    lag_min, lag_max = CL_LAGS
    xd = dev(x)
    period = lib.frames_f0(xd, None, 1, None, None, lag_min, lag_max)[0]
    curve = lib.f0_range_curve(period, scale_q=lib.range_scale(k))
    moved = lib.frames_pitch_curve(xd, None, curve, lifter=CL_Q)
    behind = lib.frames_f0(moved, None, 1, None, None, lag_min, lag_max)[0]
    got_in, got_out = lib.f0_stats(period)[0].cpu().numpy(), lib.f0_stats(behind)[0].cpu().numpy()
    ratio, ratio_want = got_out[2] / got_in[2], sd_out / sd_in
    print('  k = %g: restated sd %.6f -> %.6f (x%.4f) over %d -> %d frames; device %.6f -> %.6f (x%.4f) over %d -> %d'
          % (k, sd_in, sd_out, ratio_want, n_in, n_out, got_in[2], got_out[2], ratio, got_in[0], got_out[0]))
    assert n_in == CL_F - 5 and (got_in[0], got_out[0]) == (n_in, n_out)
    assert abs(got_in[2] - sd_in) <= f0_ref.F0_STATS_ATOL and abs(got_out[2] - sd_out) <= f0_ref.F0_STATS_ATOL
    assert abs(ratio - ratio_want) <= (1.0 + ratio_want) * f0_ref.F0_STATS_ATOL / sd_in


# ---- the driver --------------------------------------------------------------------------------------------------------------------
RULE = dict(end_offset=200, hold=1, min_steps=5)   # target 0: every row stops after step 4 -> len_b = 8
PROMPTS = ['hello world.\n', 'a somewhat longer prompt, with punctuation!\n']
LONG = ('the first sentence of this prompt is long enough to fill a good part of one piece on its own, and it ends here. '
        'the second one has no full stop for a long while, only a comma after a run of words that goes on and on and on, '
        'and then more words that follow the comma until the line has well over three hundred characters in it.\n')


def _cfg(tmp_path, k=None, smooth=2, limit=0.5):
    from tacotron_amd.config import Config
    c = Config()
    c.data_path = str(tmp_path / 'no_data') + '/'
    c.max_decode_iter = 16
    c.pitch_range, c.pitch_range_smooth, c.pitch_range_limit = k, smooth, limit
    return c


def _wav(path):
    with wavefile.open(str(path)) as f:
        assert f.getframerate() == 16000 and f.getsampwidth() == 2 and f.getnchannels() == 1
        return f.getnframes(), f.readframes(f.getnframes())


def _read(path):
    with open(path, 'rb') as f:
        return f.read()


def test_driver_writes_the_range_file_and_the_line(built_lib, tmp_path, monkeypatch, capsys):
    """test() with Config.pitch_range = 1.5 and f0: prompt_NNN_range.npy = (scale_q, W, limit, count, centre, sd in front), one line
    per prompt, lib.f0_range_curve called once per batch over the rows' own frames; every other file has the name of the run without
    it; pitch_range 1 is the run without it, byte for byte, file for file; with `long` every piece has its own centre"""
    from tacotron_amd import test as drv
    lib = built_lib
    seen = []

    def spy(period, *a, _real=lib.f0_range_curve, **k):
        seen.append((tuple(period.shape), a, k))
        return _real(period, *a, **k)
    monkeypatch.setattr(lib, 'f0_range_curve', spy)
    rule = lib.TacoStopRule(**RULE)
    r = _cfg(tmp_path).r
    common = dict(n_iter=2, stop=rule, pitch=2.0, rate=0.8, f0=True)
    plain, moved, one = tmp_path / 'plain', tmp_path / 'moved', tmp_path / 'one'
    assert drv.test(_cfg(tmp_path), PROMPTS, out_dir=str(plain), **common) == 2
    assert not seen and ' range asked ' not in capsys.readouterr().out
    assert drv.test(_cfg(tmp_path, 1.0, 4, 0.25), PROMPTS, out_dir=str(one), **common) == 2
    assert not seen and ' range asked ' not in capsys.readouterr().out
    assert drv.test(_cfg(tmp_path, 1.5, 3, 0.25), PROMPTS, out_dir=str(moved), **common) == 2
    assert len(seen) == 1 and seen[0][0] == (2, 16 * r)
    counts, per_unit, scale_q, base_q, W, limit = seen[0][1]
    assert (counts.tolist(), per_unit, scale_q.tolist(), W, limit) == ([8, 8], r, [98304, 98304], 3, 0.25)
    assert base_q.shape == (2, 16 * r) and bool((base_q == lib.pitch_step(2.0)).all())
    lines = [line for line in capsys.readouterr().out.splitlines() if ' range asked ' in line]
    assert len(lines) == 2 and all(line.startswith('prompt %d range asked x1.50, measured x' % i) and line.endswith(' voiced frames')
                                   and ' semitones) over ' in line for i, line in enumerate(lines))
    names = sorted(p.name for p in plain.iterdir())
    assert sorted(p.name for p in one.iterdir()) == names
    assert sorted(p.name for p in moved.iterdir()) == sorted(names + ['prompt_%03d_range.npy' % i for i in range(2)])
    for name in names:
        assert _read(one / name) == _read(plain / name), name
        if name.endswith('_f0.npy'):
            assert np.load(moved / name).shape == np.load(plain / name).shape
        elif name.endswith('.npy'):
            assert _read(moved / name) == _read(plain / name), name
        else:
            assert _wav(moved / name)[0] == _wav(plain / name)[0] > 0
    for i in range(2):
        got = np.load(moved / ('prompt_%03d_range.npy' % i))
        assert got.dtype == np.float64 and got.shape == (6,) and got[:3].tolist() == [98304.0, 3.0, 0.25]
        assert 0 <= got[3] <= 8 * r and got[5] >= 0.0
    # without f0 the file is written all the same (the stage tracks for itself); with long every piece is a row with its own centre
    del seen[:]
    out = tmp_path / 'long'
    assert drv.test(_cfg(tmp_path, 0.5), [PROMPTS[0], LONG], out_dir=str(out), n_iter=2, stop=rule, long=True) == 2
    K = len(list(out.glob('prompt_001_k*_spec.npy')))
    assert K >= 2 and len(seen) == 1 and seen[0][0][0] == 1 + K
    assert np.load(out / 'prompt_000_range.npy')[:3].tolist() == [32768.0, 2.0, 0.5]
    for k in range(K):
        assert np.load(out / ('prompt_001_k%02d_range.npy' % k))[:3].tolist() == [32768.0, 2.0, 0.5]
    assert not (out / 'prompt_001_range.npy').exists() and _wav(out / 'prompt_001.wav')[0] > 0
    with pytest.raises(ValueError, match='pitch_range'):
        drv.test(_cfg(tmp_path, 1.5), PROMPTS, out_dir=str(tmp_path / 'x'), n_iter=2, vocode=False)
    with pytest.raises(ValueError, match='pitch_range'):
        drv.test(_cfg(tmp_path, 4.5), PROMPTS, out_dir=str(tmp_path / 'x'), n_iter=2)


def test_driver_combines_with_prosody(built_lib, tmp_path, monkeypatch):
    """--prosody: its pitch curve is the base the range curve is composed with, and one lib.frames_pitch_curve call moves the frames"""
    from tacotron_amd import test as drv
    lib = built_lib
    seen = []
    for name in ('f0_range_curve', 'frames_pitch_curve', 'frames_stretch_curve'):
        def spy(x, *a, _real=getattr(lib, name), _name=name, **k):
            seen.append((_name, a))
            return _real(x, *a, **k)
        monkeypatch.setattr(lib, name, spy)
    rule = lib.TacoStopRule(**RULE)
    table = [(0, 0, 0.8, 2.0), (1, 1, None, -1.0)]
    assert drv.test(_cfg(tmp_path, 1.5), PROMPTS, out_dir=str(tmp_path / 'p'), n_iter=2, stop=rule, prosody=table) == 2
    assert [s[0] for s in seen] == ['f0_range_curve', 'frames_pitch_curve', 'frames_stretch_curve']
    base_q = seen[0][1][3]
    assert base_q is not None and bool((base_q != lib.PITCH_ONE).any())
    for i in range(2):
        assert np.load(tmp_path / 'p' / ('prompt_%03d_range.npy' % i))[:3].tolist() == [98304.0, 2.0, 0.5]
        assert (tmp_path / 'p' / ('prompt_%03d_prosody.npy' % i)).exists()
