"""GPU: taco_frames_f0 and taco_f0_stats.  The continuous part -- acf -- against the float64 restatement (tests/f0_ref.py) within
F0_ACF_ATOL, a bound measured on the CPU from the float32 restatement on these same inputs (tests/f0_cases.py), never from the device;
the exact part -- period and strength -- bit for bit against f0_ref.pick applied to the device's OWN acf, on every case and every frame;
and bit for bit where the contract is exact otherwise: zeros behind a row, acf == NULL, position independence, untouched surroundings.
Outputs sit between guard bands and start as poison."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import f0_cases as fc
from tests import f0_ref as fr
from tests import pitch_ref as pr
from tests.poison import Guarded

pytestmark = pytest.mark.gpu


def dev(x, dtype=torch.float32):
    return torch.as_tensor(np.asarray(x), dtype=dtype).cuda()


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def run(lib, c, want_acf=True, shift_in=0, shift_out=0, x=None, frames='case'):
    """one call on case c -> (period, strength, acf | None) as host arrays; the outputs between guard bands, preset to NaN, mag_t and
    the outputs `shift` floats behind a 256-byte boundary; the bands and the floats in front of a shifted output must be intact and
    mag_t unwritten"""
    x = c.x if x is None else x
    frames = c.frames if isinstance(frames, str) else frames
    B, Cw, F = x.shape
    L = c.lag_max - c.lag_min + 3
    G = Guarded({'in': ((x.size + shift_in,), torch.float32, 'qnan'), 'period': ((B * F + shift_out,), torch.float32, 'qnan'),
                 'strength': ((B * F + shift_out,), torch.float32, 'qnan'), 'acf': ((B * L * F + shift_out,), torch.float32, 'qnan')})
    xin = G['in'][shift_in:].view(B, Cw, F)
    xin.copy_(torch.from_numpy(x))
    out = (G['period'][shift_out:].view(B, F), G['strength'][shift_out:].view(B, F), G['acf'][shift_out:].view(B, L, F))
    assert xin.data_ptr() % 256 == 4 * shift_in and all(t.data_ptr() % 256 == 4 * shift_out for t in out)
    got = lib.frames_f0(xin, None if frames is None else dev(frames, torch.int32), c.per_unit, c.weight, c.gain, c.lag_min, c.lag_max,
                        c.ratio, c.threshold, want_acf=want_acf, out=out if want_acf else out[:2])
    torch.cuda.synchronize()
    assert [t.data_ptr() for t in got] == [t.data_ptr() for t in out[:len(got)]]
    G.check()
    for name in ('period', 'strength', 'acf'):
        head = G[name][:shift_out].cpu().numpy()
        assert (bits(head) == 0x7fc00000).all(), 'the floats in front of %s were written' % name
    if not want_acf:
        assert (bits(G['acf'].cpu().numpy()) == 0x7fc00000).all(), 'acf was written although it was not asked for'
    assert torch.equal(xin.cpu().view(torch.int32), torch.from_numpy(x).view(torch.int32)), 'mag_t was written'
    return out[0].cpu().numpy(), out[1].cpu().numpy(), out[2].cpu().numpy() if want_acf else None


def check(lib, c, **kw):
    """the call against the restatements: every element written and finite, exact zeros behind each row, acf within F0_ACF_ATOL of
    float64, period and strength the float32 pick of the device's own acf bit for bit, and the same bits without acf"""
    want = fr.acf(c.x, c.frames, c.per_unit, c.weight, c.gain, c.lag_min, c.lag_max)
    period, strength, acf = run(lib, c, **kw)
    for name, a in (('period', period), ('strength', strength), ('acf', acf)):
        assert np.isfinite(a).all(), '%s holds poison or a NaN from behind a row: %d elements' % (name, int((~np.isfinite(a)).sum()))
    B, _, F = c.x.shape
    for b in range(B):
        Fb = fr.row_frames(None if c.frames is None else c.frames[b], c.per_unit, F)
        assert not bits(period[b, Fb:]).any() and not bits(strength[b, Fb:]).any() and not bits(acf[b, :, Fb:]).any(), \
            'row %d: a bit is set behind frame %d' % (b, Fb)
    err = fc.acf_err(acf, want)
    p_ref, s_ref = fr.pick(acf, c.lag_min, c.ratio, c.threshold)
    voiced = int((period > 0).sum())
    print('  %s: B %d C %d F %d L %d: largest acf error %.3g (bound %.3g), %d voiced frames'
          % ((c.name,) + c.x.shape + (acf.shape[1], err, fr.F0_ACF_ATOL, voiced)))
    assert err <= fr.F0_ACF_ATOL
    wrong = np.flatnonzero(bits(period) != bits(p_ref))
    assert not len(wrong), 'period differs from the float32 pick of the device\'s own acf in %d frames, first %d: %r against %r' \
        % (len(wrong), wrong[0], period.ravel()[wrong[0]], p_ref.ravel()[wrong[0]])
    assert np.array_equal(bits(strength), bits(s_ref)), 'strength differs from the float32 pick of the device\'s own acf'
    p2, s2, _ = run(lib, c, want_acf=False, **kw)
    assert np.array_equal(bits(p2), bits(period)) and np.array_equal(bits(s2), bits(strength)), 'acf == NULL changes the bits'
    return period, strength, acf


CASES = {c.name: c for c in fc.all_cases()}


def test_mixed_batch(built_lib):
    """five rows at the production bin count, lags and tables, one of them empty, NaN in every source column behind a row's end; the
    100 Hz comb of row 4 is tracked at 160 samples"""
    c = CASES['mixed']
    assert c.x.shape == (5, 1025, 23) and c.lag_max - c.lag_min + 3 == 229 and np.isnan(c.x[2, :, 5:]).all()
    period, strength, _ = check(built_lib, c)
    assert not bits(period[1]).any() and np.abs(period[4] - 160.0).max() < 0.15 and strength[4].min() > 0.5


@pytest.mark.parametrize('F', fc.EDGE_F)
@pytest.mark.parametrize('shape', fc.SMALL, ids=lambda s: 'C%d_%d_%d' % s)
def test_small_and_odd_shapes(built_lib, shape, F):
    """a frame tile is 32 frames: F on each side of its edges; mag_t and the outputs 1, 2 and 3 floats behind a 256-byte boundary"""
    c = CASES['small_C%d_%d_%d_F%d' % (shape + (F,))]
    a = check(built_lib, c)
    for si, so in ((1, 3), (2, 1), (3, 2)):
        b = run(built_lib, c, shift_in=si, shift_out=so)
        assert all(np.array_equal(bits(u), bits(v)) for u, v in zip(a, b)), 'the bits depend on the alignment'


def test_unvoiced_frames(built_lib):
    """frames of zeros, of 1e-30 and without an interior maximum: +0 period and strength (and +0 acf for the first two)"""
    c = CASES['silent']
    period, strength, acf = check(built_lib, c)
    assert not bits(period[:3]).any() and not bits(strength[:3]).any() and not bits(acf[:2]).any() and acf[2].any()
    assert (period[3] > 0).all()


@pytest.mark.parametrize('shape', fc.LAG_PATHS, ids=lambda s: 'C%d_%d_%d' % s)
def test_lag_tiles(built_lib, shape):
    """33, 64 and 65 lags: a straddled tile of 32, two full ones, two and a row; 512: the cap, two tiles per wave"""
    check(built_lib, CASES['lags_C%d_%d_%d' % shape])


@pytest.mark.parametrize('r', [2, 3, 5])
def test_frames_per_unit(built_lib, r):
    c = CASES['per_unit_%d' % r]
    assert c.per_unit == r and c.frames[1] * r > c.x.shape[2] and 0 < c.frames[0] * r < c.x.shape[2]
    check(built_lib, c)


def test_frames_product_past_2_31_clamps(built_lib):
    c = CASES['past_2_31']
    assert c.frames[0] * c.per_unit > 2 ** 31 and c.frames[1] * c.per_unit < -2 ** 31
    period, _, acf = check(built_lib, c)                 # the product is formed in 64 bits: all F frames, and none
    assert not bits(acf[1]).any() and acf[0].any(axis=0).all()


def test_a_frame_does_not_depend_on_where_it_is(built_lib):
    """permute the frames of a row, move the row to another batch index, pad F: each frame's bits stay; and twice the same call"""
    lib = built_lib
    c = CASES['replay_first']._replace(frames=None)
    Cw, F = 33, 37
    row = fc.voices(1, Cw, F, c.lag_min, c.lag_max, seed=9)[0]
    one = lambda x, frames=None, **kw: run(lib, c, x=x, frames=frames, **kw)   # noqa: E731
    base = one(row[None])
    assert all(np.array_equal(bits(u), bits(v)) for u, v in zip(one(row[None]), base))            # the same arguments, the same bits
    perm = np.random.default_rng(3).permutation(F)
    got = one(np.ascontiguousarray(row[:, perm])[None])
    assert all(np.array_equal(bits(u), bits(v[..., perm])) for u, v in zip(got, base)), 'a frame changed with its position'
    batch = np.stack([fc.voices(1, Cw, F, 2, 31, seed=10)[0], np.full((Cw, F), np.nan, dtype=np.float32), row])
    got = one(batch, (F, 0, F))
    assert all(np.array_equal(bits(u[2]), bits(v[0])) for u, v in zip(got, base)), 'a row changed with its batch index'
    wide = np.full((1, Cw, 70), np.nan, dtype=np.float32)
    wide[0, :, :F] = row
    got = one(wide, (F,), shift_in=1, shift_out=2)
    assert all(np.array_equal(bits(u[0, ..., :F]), bits(v[0])) and not bits(u[0, ..., F:]).any() for u, v in zip(got, base)), \
        'a frame changed with F'


def test_a_non_finite_bin_spoils_its_own_frame_only(built_lib):
    c = CASES['replay_first']._replace(frames=None)
    base = run(built_lib, c)
    x = c.x.copy()
    x[0, 5, 7], x[1, 0, 33], x[2, 32, 0] = np.nan, np.inf, -np.inf
    got = run(built_lib, c, x=x)
    keep = np.ones(x.shape[::2], dtype=bool)
    keep[0, 7] = keep[1, 33] = keep[2, 0] = False
    for u, v in zip(got, base):
        u, v = (np.moveaxis(a, 1, -1) if a.ndim == 3 else a for a in (u, v))
        assert np.array_equal(bits(u[keep]), bits(v[keep])), 'a non-finite bin reached another frame'


def test_bad_arguments_enqueue_nothing(built_lib):
    """every TACO_EINVAL case returns before a launch: the outputs keep their fill, and the message names the argument"""
    lib = built_lib
    c = CASES['refusal_good']
    B, Cw, F = c.x.shape
    L = c.lag_max - c.lag_min + 3
    assert (Cw, c.lag_min, c.lag_max) == (17, 3, 12)
    x, frames = dev(c.x), dev(c.frames, torch.int32)
    G = Guarded({'period': ((B, F), torch.float32, 7.0), 'strength': ((B, F), torch.float32, 7.0), 'acf': ((B, L, F), torch.float32, 7.0)})
    fn = C.CDLL(lib.LIB_PATH).taco_frames_f0
    fn.restype, fn.argtypes = lib.EXPORTS['taco_frames_f0']
    good = dict(mag_t=lib.ptr(x), frames=lib.ptr(frames), per_unit=1, weight=None, gain=None, lag_min=c.lag_min, lag_max=c.lag_max,
                ratio=c.ratio, threshold=c.threshold, period=lib.ptr(G['period']), strength=lib.ptr(G['strength']), acf=lib.ptr(G['acf']),
                B=B, C=Cw, F=F)
    order = ('mag_t', 'frames', 'per_unit', 'weight', 'gain', 'lag_min', 'lag_max', 'ratio', 'threshold', 'period', 'strength', 'acf',
             'B', 'C', 'F')
    inside = C.c_void_p(x.data_ptr() + 4 * (B * Cw * F - 1))                 # an output begins on the last float of mag_t
    before = {k: C.c_void_p(G[k].data_ptr() + 4 * (G[k].numel() - 1)) for k in ('period', 'strength', 'acf')}   # mag_t on its last float
    nan = float('nan')
    cases = [({'mag_t': None}, 'mag_t'), ({'period': None}, 'period'), ({'strength': None}, 'strength'),
             ({'period': good['mag_t']}, 'period overlaps'), ({'strength': inside}, 'strength overlaps'), ({'acf': inside}, 'acf overlaps'),
             ({'mag_t': before['period']}, 'period overlaps'), ({'mag_t': before['strength']}, 'strength overlaps'),
             ({'mag_t': before['acf']}, 'acf overlaps'),
             ({'B': 0}, 'B='), ({'B': -1}, 'B='), ({'F': 0}, 'F='), ({'F': -1}, 'F='), ({'F': 8193}, 'F='),
             ({'C': 0}, 'C='), ({'C': 5}, 'C='), ({'C': 16}, 'C='), ({'C': 18}, 'C='), ({'C': 2049}, 'C='), ({'C': -17}, 'C='),
             ({'lag_min': 1}, 'lag_min'), ({'lag_min': 13}, 'lag_min'), ({'lag_max': 16}, 'lag_max'), ({'lag_min': -3}, 'lag_min'),
             ({'lag_min': 2, 'lag_max': 600, 'C': 1025}, 'lag_max'),
             ({'ratio': 0.0}, 'ratio'), ({'ratio': -0.5}, 'ratio'), ({'ratio': 1.0001}, 'ratio'), ({'ratio': nan}, 'ratio'),
             ({'threshold': nan}, 'threshold'), ({'per_unit': 0}, 'frames_per_unit'), ({'per_unit': -3}, 'frames_per_unit')]
    everything = {k: torch.ones(G[k].shape, dtype=torch.bool, device='cuda') for k in ('period', 'strength', 'acf')}
    for change, word in cases:
        for nulls in ((), ('frames', 'acf')):
            if set(nulls) & set(change) or (nulls and word == 'acf overlaps'):   # (without acf there is nothing to overlap)
                continue
            a = dict(good)
            a.update({k: None for k in nulls})
            a.update(change)
            lib.griffinlim_workspace_floats(1, 8)   # (a successful call in between: the string below is this refusal's)
            rc = fn(*[a[k] for k in order], lib.stream_ptr())
            torch.cuda.synchronize()
            msg = lib.last_error()
            print('  %r%s: rc %d, %s' % (change, ' frames / acf NULL' if nulls else '', rc, msg))
            assert rc == -1, (change, rc)
            assert 'frames_f0' in msg and word in msg, (change, msg)
            assert all(G.margin_intact(k, everything[k]) for k in everything), 'an output was written although %r is refused' % (change,)
    G.check()
    assert fn(*[good[k] for k in order], lib.stream_ptr()) == 0              # and the good arguments do run
    torch.cuda.synchronize()
    G.check('period', 'strength', 'acf')
    want = fr.acf(c.x, c.frames, 1, None, None, c.lag_min, c.lag_max)
    acf = G['acf'].cpu().numpy()
    assert fc.acf_err(acf, want) <= fr.F0_ACF_ATOL
    p_ref, s_ref = fr.pick(acf, c.lag_min, c.ratio, c.threshold)
    assert np.array_equal(bits(G['period'].cpu().numpy()), bits(p_ref)) and np.array_equal(bits(G['strength'].cpu().numpy()), bits(s_ref))
    sfn = C.CDLL(lib.LIB_PATH).taco_f0_stats
    sfn.restype, sfn.argtypes = lib.EXPORTS['taco_f0_stats']
    S = Guarded({'stats': ((B, 3), torch.float32, 7.0)})
    sgood = dict(period=lib.ptr(G['period']), other=None, frames=lib.ptr(frames), per_unit=1, stats=lib.ptr(S['stats']), B=B, F=F)
    for change, word in (({'period': None}, 'period'), ({'stats': None}, 'stats'), ({'B': 0}, 'B='), ({'F': 0}, 'F='), ({'F': 8193}, 'F='),
                         ({'per_unit': 0}, 'frames_per_unit')):
        a = dict(sgood, **change)
        lib.griffinlim_workspace_floats(1, 8)
        rc = sfn(*[a[k] for k in ('period', 'other', 'frames', 'per_unit', 'stats', 'B', 'F')], lib.stream_ptr())
        torch.cuda.synchronize()
        msg = lib.last_error()
        assert rc == -1 and 'f0_stats' in msg and word in msg, (change, rc, msg)
        assert S.margin_intact('stats', torch.ones(B, 3, dtype=torch.bool, device='cuda'))
    S.check()


def test_graph_replay_follows_the_device_arguments(built_lib):
    """one capture of the one launch (a linear graph); the replay reads frames at replay time"""
    c = CASES['replay_first']
    B, Cw, F = c.x.shape
    L = c.lag_max - c.lag_min + 3
    x = dev(c.x)
    first, second = (CASES['replay_' + name].frames for name in ('first', 'second'))
    frames = dev(first, torch.int32)
    G = Guarded({'period': ((B, F), torch.float32, 'qnan'), 'strength': ((B, F), torch.float32, 'qnan'),
                 'acf': ((B, L, F), torch.float32, 'qnan'), 'stats': ((B, 3), torch.float32, 'qnan')})

    def call():
        built_lib.frames_f0(x, frames, 1, None, None, c.lag_min, c.lag_max, c.ratio, c.threshold, want_acf=True,
                            out=(G['period'], G['strength'], G['acf']))
        built_lib.f0_stats(G['period'], None, frames, 1, out=G['stats'])

    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            call()
    torch.cuda.synchronize()
    for fr_b in (first, second, first):
        frames.copy_(dev(fr_b, torch.int32))
        G.refill('period', 'strength', 'acf', 'stats')
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        G.check('period', 'strength', 'acf', 'stats')
        acf, period = G['acf'].cpu().numpy(), G['period'].cpu().numpy()
        assert fc.acf_err(acf, fr.acf(c.x, fr_b, 1, None, None, c.lag_min, c.lag_max)) <= fr.F0_ACF_ATOL, 'replay with frames %s' % (fr_b,)
        p_ref, s_ref = fr.pick(acf, c.lag_min, c.ratio, c.threshold)
        assert np.array_equal(bits(period), bits(p_ref)) and np.array_equal(bits(G['strength'].cpu().numpy()), bits(s_ref))
        assert fc.stats_err(G['stats'].cpu().numpy(), fr.stats(period, None, fr_b, 1)) <= fr.F0_STATS_ATOL


@pytest.mark.parametrize('name', [c.name for c in fc.stats_cases()])
def test_f0_stats(built_lib, name):
    """rows with no, one and many voiced frames, paired (the other track partly unvoiced) and unpaired, against float64"""
    c = next(c for c in fc.stats_cases() if c.name == name)
    B, F = c.period.shape
    G = Guarded({'stats': ((B, 3), torch.float32, 'qnan')})
    got = built_lib.f0_stats(dev(c.period), None if c.other is None else dev(c.other), None if c.frames is None else dev(c.frames, torch.int32),
                             c.per_unit, out=G['stats'])
    torch.cuda.synchronize()
    G.check('stats')
    want = fr.stats(c.period, c.other, c.frames, c.per_unit)
    err = fc.stats_err(got.cpu().numpy(), want)
    print('  %s: counts %s, largest error of mean and deviation %.3g (bound %.3g)' % (name, want[:, 0], err, fr.F0_STATS_ATOL))
    assert err <= fr.F0_STATS_ATOL
    empty = want[:, 0] == 0
    assert not bits(got.cpu().numpy()[empty]).any()


def test_shift_is_measured_on_the_device(built_lib):
    """end to end at C = 1025, F = 24: the 100 Hz comb through lib.frames_pitch at +4 semitones, both tracked with the production tables
    and compared by the paired statistic on the device: within 0.05 semitones of the step"""
    lib = built_lib
    mag = dev(pr.comb(1025, 24)[0][None])
    step = lib.pitch_step(4)
    moved = lib.frames_pitch(mag, None, step)
    w, g, lo, hi = lib.f0_tables()
    before = lib.frames_f0(mag, weight=w, gain=g, lag_min=lo, lag_max=hi)
    behind = lib.frames_f0(moved, weight=w, gain=g, lag_min=lo, lag_max=hi)
    count, mean, sd = lib.f0_stats(behind[0], before[0]).cpu().numpy()[0]
    asked = 12.0 * np.log2(65536.0 / step)
    print('  asked %+.4f, measured %+.4f semitones over %d frames (deviation %.4f); periods %.3f -> %.3f'
          % (asked, 12.0 * mean, count, 12.0 * sd, float(before[0].mean()), float(behind[0].mean())))
    assert count == 24 and abs(12.0 * mean - asked) <= 0.05
