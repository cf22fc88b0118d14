"""GPU: the three prosody-curve entry points against tests/curve_ref.py.  taco_path_curve and taco_frames_stretch_curve are exact
(integers, and three separately rounded fp32 operations): out, src and frames_out are compared bit for bit.  taco_frames_pitch_curve
is compared bit for bit, frame by frame, with taco_frames_pitch run once per distinct step, and with the float64 restatement within
tests.pitch_ref.PITCH_RTOL (the existing bound, not re-derived).  Outputs sit between guard bands and start as poison."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import curve_ref as cr
from tests import pitch_cases as pc
from tests import pitch_ref as pr
from tests import stretch_ref as sr
from tests.poison import Guarded

pytestmark = pytest.mark.gpu


def dev(x, dtype=torch.float32):
    return torch.as_tensor(np.asarray(x), dtype=dtype).cuda()


def idev(x):
    return None if x is None else dev(x, torch.int32)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def mags(B, Cw, F, seed=0):
    rng = np.random.default_rng(seed)
    return np.exp(rng.standard_normal((B, Cw, F)) * 2.0).astype(np.float32)


def nan_behind(x, frames, per_unit=1):
    x = x.copy()
    for b, f in enumerate(frames):
        x[b, :, sr.row_frames(f, per_unit, x.shape[2]):] = np.nan
    return x


# ---- taco_frames_stretch_curve ---------------------------------------------------------------------------------------------------
def run_stretch(lib, x, frames, dur, Fo, per_unit=1, shift=0):
    """one call -> (out, frames_out, src) as host arrays; the three outputs between guard bands and poisoned, mag_t and out `shift`
    floats behind a 256-byte boundary (src `shift` words behind one)"""
    B, Cw, F = x.shape
    G = Guarded({'in': ((x.size + shift,), torch.float32, 'qnan'), 'out': ((B * Cw * Fo + shift,), torch.float32, 'qnan'),
                 'n': ((B,), torch.int32, 'ones'), 'src': ((B * Fo + shift,), torch.int32, 'qnan')})
    xin = G['in'][shift:].view(B, Cw, F)
    xin.copy_(torch.from_numpy(x))
    out, src = G['out'][shift:].view(B, Cw, Fo), G['src'][shift:].view(B, Fo)
    assert xin.data_ptr() % 16 == (4 * shift) % 16 and out.data_ptr() % 16 == (4 * shift) % 16
    got = lib.frames_stretch_curve(xin, idev(frames), idev(dur), frames_per_unit=per_unit, out=out, frames_out=G['n'], src=src)
    torch.cuda.synchronize()
    assert got[0].data_ptr() == out.data_ptr() and got[1].data_ptr() == G['n'].data_ptr() and got[2].data_ptr() == src.data_ptr()
    G.check('n')
    assert (bits(G['out'][:shift].cpu().numpy()) == 0x7fc00000).all(), 'the floats in front of out were written'
    assert (G['src'][:shift].cpu().numpy() == 0x7fc00000).all(), 'the words in front of src were written'
    assert torch.equal(xin.cpu().view(torch.int32), torch.from_numpy(x).view(torch.int32)), 'mag_t was written'
    return out.cpu().numpy(), G['n'].cpu().numpy(), src.cpu().numpy()


def check_stretch(lib, x, frames, dur, Fo, per_unit=1, **kw):
    want, want_n, want_src = cr.stretch_curve(x, frames, dur, per_unit, Fo)
    got, got_n, got_src = run_stretch(lib, x, frames, dur, Fo, per_unit, **kw)
    print('  B %d C %d F %d Fo %d: frames_out %s' % (x.shape + (Fo, got_n.tolist())))
    assert got_n.tolist() == want_n.tolist()
    bad = got_src != want_src
    assert not bad.any(), '%d elements of src differ, first at %s' % (int(bad.sum()), np.argwhere(bad)[0].tolist())
    assert np.isfinite(got).all(), 'an element of out holds poison or a NaN from behind a row: %d' % int((~np.isfinite(got)).sum())
    bad = bits(got) != bits(want)
    assert not bad.any(), '%d elements differ from the restatement, first at %s' % (int(bad.sum()), np.argwhere(bad)[0].tolist())
    for b, nb in enumerate(got_n):
        assert not bits(got[b, :, nb:]).any() and (got_src[b, nb:] == -1).all()
    return got, got_n, got_src


MIX_F, MIX_FO = 300, 700
MIX_FRAMES = (300, 0, 1, 300, 300, 287)


def mixed_durations(extra=None):
    """the rows of the mixed batch: full at 65536, empty, F_b = 1, all 16384, all 262144 (needs 1197 frames: Fo cuts it), random"""
    rng = np.random.default_rng(11)
    d = np.full((6, MIX_F), 65536, dtype=np.int64)
    d[1] = rng.integers(16384, 262145, MIX_F)
    d[2] = 100000
    d[3] = 16384
    d[4] = 262144
    d[5] = rng.integers(16384, 262145, MIX_F)
    if extra is not None:
        d[0] = extra
    return d


def test_stretch_mixed_batch(built_lib):
    """B = 6, C = 17 (one bin past the 16-bin tile), F = 300, Fo = 700 (three spans of 256): every kind of row, NaN behind each"""
    x = nan_behind(mags(6, 17, MIX_F), MIX_FRAMES)
    got, n, src = check_stretch(built_lib, x, MIX_FRAMES, mixed_durations(), MIX_FO)
    assert n.tolist()[:5] == [300, 0, 1, 75, 700] and 256 < n[5] <= 700
    assert np.array_equal(bits(got[0, :, :300]), bits(x[0]))                       # every duration 65536: a copy
    for b in (0, 2, 3, 4, 5):
        assert (np.diff(src[b, :n[b]].astype(np.int64)) > 0).all()                # the map rises strictly


def test_stretch_out_of_range_durations_are_clamped_on_the_device(built_lib):
    rng = np.random.default_rng(12)
    row = rng.choice(np.array([0, -5, 2 ** 30, 65536, 30000]), MIX_F)
    x = nan_behind(mags(6, 17, MIX_F, seed=1), MIX_FRAMES)
    got, n, src = check_stretch(built_lib, x, MIX_FRAMES, mixed_durations(row), MIX_FO)
    clamped = mixed_durations(np.clip(row, 16384, 262144))
    want, wn, wsrc = run_stretch(built_lib, x, MIX_FRAMES, clamped, MIX_FO)
    assert n.tolist() == wn.tolist() and np.array_equal(src, wsrc) and np.array_equal(bits(got), bits(want))


def test_stretch_real_bin_count(built_lib):
    rng = np.random.default_rng(13)
    x = mags(2, 1025, 40, seed=2)
    check_stretch(built_lib, x, (40, 33), rng.integers(16384, 262145, (2, 40)), 120)


def test_stretch_the_sum_of_durations_needs_the_32nd_bit(built_lib):
    """B = C = 1, F = Fo = 8192, every d = 262144: the scan's total is 2^31"""
    d = np.full((1, 8192), 262144, dtype=np.int64)
    assert int(d.sum()) == 2 ** 31
    x = mags(1, 1, 8192, seed=3)
    _, n, src = check_stretch(built_lib, x, None, d, 8192)
    assert n.tolist() == [8192] and src[0, -1] == ((8191 // 4) << 16) | ((8191 % 4) << 14)


@pytest.mark.parametrize('shift', [1, 2, 3])
def test_stretch_bases_behind_a_16_byte_boundary(built_lib, shift):
    rng = np.random.default_rng(14)
    x = mags(3, 5, 23, seed=4)
    d = rng.integers(16384, 262145, (3, 23))
    a, _, sa = check_stretch(built_lib, x, (23, 20, 23), d, 37, shift=shift)
    b, _, sb = check_stretch(built_lib, x, (23, 20, 23), d, 37)
    assert np.array_equal(bits(a), bits(b)) and np.array_equal(sa, sb)


def test_stretch_frames_in_units(built_lib):
    rng = np.random.default_rng(15)
    d = rng.integers(16384, 262145, (2, 16))
    x = nan_behind(mags(2, 4, 16, seed=5), (4, 100), 2)
    _, n, _ = check_stretch(built_lib, x, (4, 100), d, 40, per_unit=2)
    assert n[0] == min(40, (int(d[0, :7].sum()) >> 16) + 1)
    _, n, _ = check_stretch(built_lib, mags(2, 4, 16, seed=5), (2 ** 30, -2 ** 30), d, 64, per_unit=1000)
    assert n[0] == min(64, (int(d[0, :15].sum()) >> 16) + 1) and n[1] == 0


def test_stretch_null_frames_and_null_durations(built_lib):
    rng = np.random.default_rng(16)
    x = mags(2, 6, 12, seed=6)
    check_stretch(built_lib, x, None, rng.integers(16384, 262145, (2, 12)), 40)
    got, n, src = check_stretch(built_lib, nan_behind(x, (12, 7)), (12, 7), None, 13)
    assert n.tolist() == [12, 7] and np.array_equal(bits(got[0, :, :12]), bits(x[0]))
    assert src[1, :7].tolist() == [i << 16 for i in range(7)]
    check_stretch(built_lib, x, None, None, 16)


def test_stretch_rows_are_the_call_on_each_row_alone(built_lib):
    x = nan_behind(mags(6, 17, MIX_F), MIX_FRAMES)
    d = mixed_durations()
    batch, n, src = run_stretch(built_lib, x, MIX_FRAMES, d, MIX_FO)
    for b, f in enumerate(MIX_FRAMES):
        if f == 0:
            continue
        alone, na, sa = run_stretch(built_lib, np.ascontiguousarray(x[b:b + 1, :, :f]), None, d[b:b + 1, :f], MIX_FO)
        assert na.tolist() == [n[b]] and np.array_equal(sa[0], src[b]) and np.array_equal(bits(alone[0]), bits(batch[b])), b


@pytest.mark.parametrize('dur,step', [(16384, 262144), (32768, 131072), (65536, 65536), (131072, 32768), (262144, 16384)])
def test_stretch_power_of_two_constants_equal_frames_stretch(built_lib, dur, step):
    """a constant duration 65536 / rate is the constant step 65536 * rate: the same Fo_b and the same bits"""
    frames = (300, 7, 1, 0)
    x = nan_behind(mags(4, 3, 300, seed=7), frames)
    Fo = 640
    got, n, _ = run_stretch(built_lib, x, frames, np.full((4, 300), dur), Fo)
    want, wn = built_lib.frames_stretch(dev(x), idev(frames), idev([step] * 4), Fo=Fo)
    assert n.tolist() == wn.cpu().numpy().tolist()
    assert np.array_equal(bits(got), bits(want.cpu().numpy()))


def test_stretch_bad_arguments_enqueue_nothing(built_lib):
    lib = built_lib
    B, Cw, F, Fo = 2, 3, 8, 16
    xh = mags(B, Cw, F, seed=8)
    x = dev(xh)
    dh = np.array([[32768] * F, [100000] * F])
    fr, du = idev([8, 5]), idev(dh)
    G = Guarded({'out': ((B, Cw, Fo), torch.float32, 7.0), 'n': ((B,), torch.int32, 7.0), 'src': ((B, Fo), torch.int32, 7.0)})
    fn = C.CDLL(lib.LIB_PATH).taco_frames_stretch_curve
    fn.restype, fn.argtypes = lib.EXPORTS['taco_frames_stretch_curve']
    good = dict(mag_t=lib.ptr(x), frames=lib.ptr(fr), per_unit=1, dur_q=lib.ptr(du), out=lib.ptr(G['out']), frames_out=lib.ptr(G['n']),
                src=lib.ptr(G['src']), B=B, C=Cw, F=F, Fo=Fo)
    order = ('mag_t', 'frames', 'per_unit', 'dur_q', 'out', 'frames_out', 'src', 'B', 'C', 'F', 'Fo')
    inside = C.c_void_p(x.data_ptr() + 4 * (B * Cw * F - 1))
    before = C.c_void_p(G['out'].data_ptr() + 4 * (B * Cw * Fo - 1))
    cases = [({'mag_t': None}, 'mag_t'), ({'out': None}, 'out'), ({'frames_out': None}, 'frames_out'), ({'src': None}, 'src'),
             ({'out': good['mag_t']}, 'overlap'), ({'out': inside}, 'overlap'), ({'mag_t': before}, 'overlap'), ({'B': 0}, 'B='),
             ({'B': -1}, 'B='), ({'C': 0}, 'C='), ({'C': -7}, 'C='), ({'F': 0}, 'F='), ({'F': -1}, 'F='), ({'F': 8193}, 'F='),
             ({'Fo': 0}, 'Fo='), ({'Fo': -2}, 'Fo='), ({'Fo': 8193}, 'Fo='), ({'per_unit': 0}, 'frames_per_unit'),
             ({'per_unit': -3}, 'frames_per_unit')]
    everything = {k: torch.ones(G[k].shape, dtype=torch.bool, device='cuda') for k in ('out', 'n', 'src')}
    for change, word in cases:
        for nulls in ((), ('frames', 'dur_q')):
            a = dict(good)
            a.update({k: None for k in nulls})
            a.update(change)
            lib.griffinlim_workspace_floats(1, 8)   # (a successful call in between: the string below is this refusal's)
            rc = fn(*[a[k] for k in order], lib.stream_ptr())
            torch.cuda.synchronize()
            msg = lib.last_error()
            assert rc == -1, (change, rc)
            assert 'frames_stretch_curve' in msg and word in msg, (change, msg)
            for name, m in everything.items():
                assert G.margin_intact(name, m), '%s was written although %r is refused' % (name, change)
    G.check()
    assert fn(*[good[k] for k in order], lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    G.check('out', 'n', 'src')
    want, wn, wsrc = cr.stretch_curve(xh, [8, 5], dh, 1, Fo)
    assert np.array_equal(bits(G['out'].cpu().numpy()), bits(want)) and G['n'].cpu().numpy().tolist() == wn.tolist()
    assert np.array_equal(G['src'].cpu().numpy(), wsrc)
    for bad in (dict(dur_q=du[:, :4].contiguous()), dict(dur_q=du.float()), dict(src=torch.empty(B, Fo + 1, dtype=torch.int32, device='cuda'))):
        with pytest.raises(ValueError, match='frames_stretch_curve'):
            lib.frames_stretch_curve(x, fr, **{'dur_q': du, **bad}, Fo=Fo)


def test_stretch_graph_replay_follows_the_device_arguments(built_lib):
    """one capture of the two launches; the replay reads frames and dur_q at replay time"""
    B, Cw, F, Fo = 3, 5, 20, 77
    rng = np.random.default_rng(17)
    xh = mags(B, Cw, F, seed=9)
    x = dev(xh)
    first = ([20, 9, 0], rng.integers(16384, 262145, (B, F)))
    second = ([3, 20, 14], rng.integers(16384, 262145, (B, F)))
    frames, dur = idev(first[0]), idev(first[1])
    G = Guarded({'out': ((B, Cw, Fo), torch.float32, 'qnan'), 'n': ((B,), torch.int32, 'ones'), 'src': ((B, Fo), torch.int32, 'qnan')})
    call = lambda: built_lib.frames_stretch_curve(x, frames, dur, out=G['out'], frames_out=G['n'], src=G['src'])   # noqa: E731
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            call()
    torch.cuda.synchronize()
    for fr, du in (first, second, first):
        frames.copy_(idev(fr))
        dur.copy_(idev(du))
        G.refill('out', 'n', 'src')
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        G.check('out', 'n', 'src')
        want, wn, wsrc = cr.stretch_curve(xh, fr, du, 1, Fo)
        assert G['n'].cpu().numpy().tolist() == wn.tolist() and np.array_equal(G['src'].cpu().numpy(), wsrc)
        assert np.array_equal(bits(G['out'].cpu().numpy()), bits(want)), 'replay with frames %s differs from the restatement' % (fr,)


# ---- taco_frames_pitch_curve -----------------------------------------------------------------------------------------------------
PITCH_STEPS = (40000, 131072, 65537, 32768, 99999, 50000, 77777)


def pitch_batch(Cw, F, seed):
    """(mag_t (4, C, F), frames, step_q (4, F)):
    row 0  full: the first tile all at ONE, behind it a step that changes at every frame
    row 1  cut at F - 3 with NaN behind: every third frame at ONE among shifted ones
    row 2  full: out-of-range steps (0, -5, 2^30) among in-range ones
    row 3  empty, all NaN: the neighbour nobody may read"""
    frames = (F, max(F - 3, 0), F, 0)
    x = nan_behind(mags(4, Cw, F, seed=seed), frames)
    f = np.arange(F)
    steps = np.zeros((4, F), dtype=np.int64)
    steps[0] = np.where(f < 32, 65536, 33000 + 1500 * f)
    steps[1] = np.where(f % 3 == 0, 65536, np.array(PITCH_STEPS)[f % 7])
    steps[2] = np.array([0, 45000, -5, 2 ** 30, 65536, 88888])[f % 6]
    steps[3] = 40000
    return x, frames, steps


def run_pitch(lib, x, frames, steps, Q, shift=0):
    B, Cw, F = x.shape
    G = Guarded({'in': ((x.size + shift,), torch.float32, 'qnan'), 'out': ((x.size + shift,), torch.float32, 'qnan')})
    xin = G['in'][shift:].view(B, Cw, F)
    xin.copy_(torch.from_numpy(x))
    out = G['out'][shift:].view(B, Cw, F)
    got = lib.frames_pitch_curve(xin, idev(frames), idev(steps), lifter=Q, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    G.check()
    assert (bits(G['out'][:shift].cpu().numpy()) == 0x7fc00000).all(), 'the floats in front of out were written'
    assert torch.equal(xin.cpu().view(torch.int32), torch.from_numpy(x).view(torch.int32)), 'mag_t was written'
    return out.cpu().numpy()


def assembled(lib, x, frames, steps, Q):
    """the same frames through taco_frames_pitch, one call per distinct clamped step, put together frame by frame"""
    B, Cw, F = x.shape
    cl = np.clip(steps, pr.MIN_STEP, pr.MAX_STEP)
    xd, fd = dev(x), idev(frames)
    want = np.zeros_like(x)
    for s in np.unique(cl):
        y = lib.frames_pitch(xd, fd, int(s), lifter=Q).cpu().numpy()
        for b in range(B):
            Fb = pr.row_frames(None if frames is None else frames[b], 1, F)
            cols = np.flatnonzero(cl[b, :Fb] == s)
            want[b][:, cols] = y[b][:, cols]
    return want


def check_pitch(lib, x, frames, steps, Q, **kw):
    got = run_pitch(lib, x, frames, steps, Q, **kw)
    B, _, F = x.shape
    assert np.isfinite(got).all(), 'an element of out holds poison or a NaN from elsewhere: %d' % int((~np.isfinite(got)).sum())
    for b in range(B):
        Fb = pr.row_frames(None if frames is None else frames[b], 1, F)
        assert not bits(got[b, :, Fb:]).any(), 'row %d: a bit is set behind frame %d' % (b, Fb)
        if steps is not None:
            one = np.flatnonzero(np.clip(steps[b, :Fb], pr.MIN_STEP, pr.MAX_STEP) == pr.ONE)
            assert np.array_equal(bits(got[b][:, one]), bits(x[b][:, one])), 'row %d: a frame at 65536 is not its input' % b
    want = assembled(lib, x, frames, np.full(x.shape[::2], pr.ONE) if steps is None else steps, Q)
    bad = bits(got) != bits(want)
    assert not bad.any(), '%d elements differ from taco_frames_pitch at the same step, first at %s' % (int(bad.sum()),
                                                                                                      np.argwhere(bad)[0].tolist())
    err = pc.rel_err(got, cr.pitch_curve(x, frames, steps, 1, Q))
    print('  C %d F %d Q %d: largest relative error against fp64 %.3g (bound %.3g)' % (x.shape[1], F, Q, err, pr.PITCH_RTOL))
    assert err <= pr.PITCH_RTOL
    return got


@pytest.mark.parametrize('F', [1, 31, 32, 33, 65])
@pytest.mark.parametrize('CQ', [(17, 1), (17, 8), (129, 32), (129, 33)], ids=lambda cq: 'C%d_Q%d' % cq)
def test_pitch_curve_frame_by_frame(built_lib, CQ, F):
    """both lifter paths (Q <= 32 and above), F on each side of the 32-frame tile's edges"""
    x, frames, steps = pitch_batch(CQ[0], F, seed=100 * CQ[0] + CQ[1] + F)
    a = check_pitch(built_lib, x, frames, steps, CQ[1])
    if F == 33:
        b = check_pitch(built_lib, x, frames, steps, CQ[1], shift=1)
        assert np.array_equal(bits(a), bits(b)), 'the bits depend on the alignment'


def test_pitch_curve_real_bin_count(built_lib):
    x, frames, steps = pitch_batch(1025, 33, seed=5)
    check_pitch(built_lib, x, frames, steps, 64)


def test_pitch_curve_null_steps_and_null_frames(built_lib):
    x, frames, steps = pitch_batch(17, 40, seed=6)
    got = check_pitch(built_lib, x, frames, None, 4)
    assert np.array_equal(bits(got[0]), bits(x[0]))
    check_pitch(built_lib, mags(2, 17, 40, seed=7), None, steps[:2], 4)


def test_pitch_curve_bad_arguments(built_lib):
    lib = built_lib
    B, Cw, F = 2, 17, 8
    x = dev(mags(B, Cw, F, seed=8))
    st = idev(np.full((B, F), 40000))
    G = Guarded({'out': ((B, Cw, F), torch.float32, 7.0)})
    fn = C.CDLL(lib.LIB_PATH).taco_frames_pitch_curve
    fn.restype, fn.argtypes = lib.EXPORTS['taco_frames_pitch_curve']
    good = dict(mag_t=lib.ptr(x), frames=None, per_unit=1, step_q=lib.ptr(st), lifter=4, out=lib.ptr(G['out']), B=B, C=Cw, F=F)
    order = ('mag_t', 'frames', 'per_unit', 'step_q', 'lifter', 'out', 'B', 'C', 'F')
    cases = [({'mag_t': None}, 'mag_t'), ({'out': None}, 'out'), ({'out': good['mag_t']}, 'overlap'), ({'B': 0}, 'B='), ({'C': 18}, 'C='),
             ({'C': 2049}, 'C='), ({'F': 0}, 'F='), ({'F': 8193}, 'F='), ({'lifter': 0}, 'lifter'), ({'lifter': 9}, 'lifter'),
             ({'per_unit': 0}, 'frames_per_unit')]
    whole = torch.ones(G['out'].shape, dtype=torch.bool, device='cuda')
    for change, word in cases:
        a = dict(good)
        a.update(change)
        lib.griffinlim_workspace_floats(1, 8)
        rc = fn(*[a[k] for k in order], lib.stream_ptr())
        torch.cuda.synchronize()
        msg = lib.last_error()
        assert rc == -1 and 'frames_pitch_curve' in msg and word in msg, (change, rc, msg)
        assert G.margin_intact('out', whole), 'out was written although %r is refused' % (change,)
    with pytest.raises(ValueError, match='frames_pitch_curve: step_q'):
        lib.frames_pitch_curve(x, None, st[0].contiguous(), lifter=4)


def test_pitch_curve_graph_replay(built_lib):
    B, Cw, F, Q = 4, 33, 40, 16
    xh, fr1, st1 = pitch_batch(Cw, F, seed=9)
    fr2, st2 = (3, 40, 33, 40), np.roll(st1, 1, axis=0)
    xh = np.where(np.isnan(xh), np.float32(1.5), xh)          # (the second set of lengths reaches what was NaN)
    x, frames, steps = dev(xh), idev(fr1), idev(st1)
    G = Guarded({'out': ((B, Cw, F), torch.float32, 'qnan')})
    call = lambda: built_lib.frames_pitch_curve(x, frames, steps, lifter=Q, out=G['out'])   # noqa: E731
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            call()
    torch.cuda.synchronize()
    for fr, st in ((fr1, st1), (fr2, st2), (fr1, st1)):
        frames.copy_(idev(fr))
        steps.copy_(idev(st))
        G.refill('out')
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        G.check('out')
        want = assembled(built_lib, xh, fr, st, Q)
        assert np.array_equal(bits(G['out'].cpu().numpy()), bits(want)), 'replay with frames %s differs' % (fr,)


# ---- taco_path_curve -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('r', [1, 2, 5])
def test_path_curve(built_lib, r):
    """a -1 tail, an empty row, an index >= Tt and one below -1 give `fill`; more than one workgroup of 256 elements"""
    rng = np.random.default_rng(r)
    B, Td, Tt, fill = 3, 131, 9, -77
    path = np.sort(rng.integers(0, Tt, (B, Td)), axis=1)
    path[0, 100:] = -1
    path[1, :] = -1
    path[2, 5], path[2, 6] = Tt, -2
    values = rng.integers(-2 ** 31, 2 ** 31, (B, Tt))
    G = Guarded({'curve': ((B, Td * r), torch.int32, 'qnan')})
    got = built_lib.path_curve(idev(path), idev(values), r, fill, curve=G['curve'])
    torch.cuda.synchronize()
    G.check('curve')
    want = cr.path_curve(path, values, r, fill)
    assert want[2, 5 * r] == fill and want[2, 6 * r] == fill and (want[1] == fill).all() and (want[0, 100 * r:] == fill).all()
    assert np.array_equal(got.cpu().numpy(), want)


def test_path_curve_bad_arguments(built_lib):
    lib = built_lib
    B, Td, Tt = 2, 6, 4
    path, values = idev(np.zeros((B, Td))), idev(np.ones((B, Tt)))
    G = Guarded({'curve': ((B, Td * 2), torch.int32, 7.0)})
    fn = C.CDLL(lib.LIB_PATH).taco_path_curve
    fn.restype, fn.argtypes = lib.EXPORTS['taco_path_curve']
    good = dict(path=lib.ptr(path), values=lib.ptr(values), r=2, fill=0, curve=lib.ptr(G['curve']), B=B, Td=Td, Tt=Tt)
    order = ('path', 'values', 'r', 'fill', 'curve', 'B', 'Td', 'Tt')
    cases = [({'path': None}, 'path is'), ({'values': None}, 'values'), ({'curve': None}, 'curve is'), ({'B': 0}, 'B='), ({'Td': 0}, 'Td='),
             ({'Tt': -1}, 'Tt='), ({'r': 0}, 'frames_per_step'), ({'Td': 4097}, 'frames_per_step'), ({'Td': 2 ** 30, 'r': 2 ** 30}, 'Td=')]
    whole = torch.ones(G['curve'].shape, dtype=torch.bool, device='cuda')
    for change, word in cases:
        a = dict(good)
        a.update(change)
        lib.griffinlim_workspace_floats(1, 8)
        rc = fn(*[a[k] for k in order], lib.stream_ptr())
        torch.cuda.synchronize()
        msg = lib.last_error()
        assert rc == -1 and 'path_curve' in msg and word in msg, (change, rc, msg)
        assert G.margin_intact('curve', whole), 'curve was written although %r is refused' % (change,)
    assert fn(*[good[k] for k in order], lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    G.check('curve')
    assert (G['curve'].cpu().numpy() == 1).all()
    with pytest.raises(ValueError, match='path_curve'):
        lib.path_curve(path, values, 4096)
