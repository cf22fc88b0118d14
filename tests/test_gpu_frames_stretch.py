"""GPU: taco_frames_stretch against the NumPy float32 restatement (tests/stretch_ref.py), bit for bit in every case -- the definition
is three separately rounded fp32 operations, so there is no tolerance.  Outputs sit between guard bands and start as poison."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import stretch_ref as sr
from tests.poison import Guarded

pytestmark = pytest.mark.gpu


def dev(x, dtype=torch.float32):
    return torch.as_tensor(np.asarray(x), dtype=dtype).cuda()


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def mags(B, Cw, F, seed=0):
    """magnitudes as exp() leaves them: positive, over many binades"""
    rng = np.random.default_rng(seed)
    return np.exp(rng.standard_normal((B, Cw, F)) * 2.0).astype(np.float32)


def nan_behind(x, frames, per_unit=1):
    x = x.copy()
    for b, f in enumerate(frames):
        x[b, :, sr.row_frames(f, per_unit, x.shape[2]):] = np.nan
    return x


def run(lib, x, frames, steps, Fo, per_unit=1, shift_in=0, shift_out=0):
    """one call on x (host array) -> (out, frames_out) as host arrays; out and frames_out between guard bands, preset to NaN / -1,
    mag_t and out `shift` floats behind a 256-byte boundary; the bands and the floats in front of a shifted out must be intact"""
    B, Cw, F = x.shape
    G = Guarded({'in': ((x.size + shift_in,), torch.float32, 'qnan'), 'out': ((B * Cw * Fo + shift_out,), torch.float32, 'qnan'),
                 'n': ((B,), torch.int32, 'ones')})
    xin = G['in'][shift_in:].view(B, Cw, F)
    xin.copy_(torch.from_numpy(x))
    out = G['out'][shift_out:].view(B, Cw, Fo)
    assert xin.data_ptr() % 16 == (4 * shift_in) % 16 and out.data_ptr() % 16 == (4 * shift_out) % 16
    got = lib.frames_stretch(xin, None if frames is None else dev(frames, torch.int32), None if steps is None else dev(steps, torch.int32),
                             frames_per_unit=per_unit, out=out, frames_out=G['n'])
    torch.cuda.synchronize()
    assert got[0].data_ptr() == out.data_ptr() and got[1].data_ptr() == G['n'].data_ptr()
    G.check('n')
    head = G['out'][:shift_out].cpu().numpy()
    assert np.isnan(head).all() and (bits(head) == 0x7fc00000).all(), 'the floats in front of out were written'
    assert torch.equal(xin.cpu().view(torch.int32), torch.from_numpy(x).view(torch.int32)), 'mag_t was written'
    return out.cpu().numpy(), G['n'].cpu().numpy()


def check(lib, x, frames, steps, Fo, per_unit=1, **kw):
    want, want_n = sr.stretch(x, frames, steps, per_unit, Fo)
    got, got_n = run(lib, x, frames, steps, Fo, per_unit, **kw)
    print('  B %d C %d F %d Fo %d: frames_out %s' % (x.shape + (Fo, got_n.tolist())))
    assert got_n.tolist() == want_n.tolist()
    assert np.isfinite(got).all(), 'an element of out holds poison or a NaN from behind a row: %d' % int((~np.isfinite(got)).sum())
    bad = bits(got) != bits(want)
    assert not bad.any(), '%d elements differ from the restatement, first at %s' % (int(bad.sum()), np.argwhere(bad)[0].tolist())
    return got, got_n


MIXED_FRAMES = (23, 0, 5, 13, 23)
MIXED_STEPS = (65536, 65536, 16384, 262144, 77777)


def test_mixed_batch(built_lib):
    """every kind of row in one call, Fo = 89 = the capacity at 4x slower, NaN in every source column behind a row's end"""
    x = nan_behind(mags(5, 7, 23), MIXED_FRAMES)
    got, n = check(built_lib, x, MIXED_FRAMES, MIXED_STEPS, 89)
    assert n.tolist() == [23, 0, 17, 4, 19] and sr.out_frames(23, 16384) == 89
    assert np.array_equal(bits(got[0, :, :23]), bits(x[0]))               # step 65536: a copy
    for b, nb in enumerate(n):
        assert not got[b, :, nb:].any()                                   # exactly 0 behind Fo_b (+0: no bit set)
        assert not bits(got[b, :, nb:]).any()


def test_real_bin_count_on_an_aligned_base(built_lib):
    """C = 1025 is no multiple of the 16-bin tile; Fo % 4 == 0 and a 16-byte aligned base, where a 16-byte store would be possible"""
    x = mags(2, 1025, 24, seed=1)
    _, n = check(built_lib, x, None, (32768, 32768), 48)
    assert n.tolist() == [47, 47]


def test_odd_sizes_and_misaligned_bases_give_the_same_bits(built_lib):
    """F = 23, Fo = 37, mag_t and out one float behind a 16-byte boundary; and the same rows at Fo = 40 on aligned bases"""
    x = mags(3, 5, 23, seed=2)
    steps = (40000, 65536, 131072)
    a, _ = check(built_lib, x, (23, 20, 23), steps, 37, shift_in=1, shift_out=1)
    b, _ = check(built_lib, x, (23, 20, 23), steps, 40)
    assert np.array_equal(bits(a), bits(b[:, :, :37]))
    check(built_lib, x, (23, 20, 23), steps, 40, shift_out=2)           # Fo % 4 == 0 on a base that is not 16-byte aligned
    check(built_lib, x, (23, 20, 23), steps, 40, shift_in=3)


@pytest.mark.parametrize('F,Fo,step', [(300, 1197, 16384), (1197, 300, 262144), (300, 1200, 16384), (260, 260, 65537)],
                         ids=['slow_odd', 'fast', 'slow_mult4', 'span_edge'])
def test_more_than_one_span_of_output_frames(built_lib, F, Fo, step):
    """a workgroup owns 256 output frames: five spans at 4x slower, two at 4x faster, a last span of 4 frames"""
    x = mags(1, 3, F, seed=F)
    _, n = check(built_lib, x, None, (step,), Fo)
    assert n.tolist() == [min(Fo, sr.out_frames(F, step))]


def test_frames_in_units(built_lib):
    """frames_per_unit = 2: 4 units are 8 frames, 100 units clamp to F = 16; a product behind 2^31 clamps too"""
    x = nan_behind(mags(2, 4, 16, seed=3), (4, 100), 2)
    _, n = check(built_lib, x, (4, 100), (32768, 32768), 31, per_unit=2)
    assert n.tolist() == [15, 31]
    x = mags(2, 4, 16, seed=3)
    _, n = check(built_lib, x, (2 ** 30, -2 ** 30), None, 16, per_unit=1000)
    assert n.tolist() == [16, 0]


def test_null_frames_and_null_steps(built_lib):
    x = mags(2, 6, 12, seed=4)
    check(built_lib, x, None, (20000, 99999), 40)
    check(built_lib, nan_behind(x, (12, 7)), (12, 7), None, 13)
    got, n = check(built_lib, x, None, None, 16)                           # both NULL: a plain copy with a zero tail
    assert n.tolist() == [12, 12] and np.array_equal(bits(got[:, :, :12]), bits(x)) and not bits(got[:, :, 12:]).any()


def test_rows_are_the_call_on_each_row_alone(built_lib):
    """row b of the mixed batch equals the B = 1, F = F_b call on a contiguous copy of its first F_b columns"""
    x = nan_behind(mags(5, 7, 23), MIXED_FRAMES)
    batch, n = check(built_lib, x, MIXED_FRAMES, MIXED_STEPS, 89)
    for b, (f, s) in enumerate(zip(MIXED_FRAMES, MIXED_STEPS)):
        if f == 0:
            assert n[b] == 0 and not bits(batch[b]).any()
            continue
        alone, na = run(built_lib, np.ascontiguousarray(x[b:b + 1, :, :f]), None, (s,), 89)
        assert na.tolist() == [n[b]] and np.array_equal(bits(alone[0]), bits(batch[b])), b
    again, _ = run(built_lib, x, MIXED_FRAMES, MIXED_STEPS, 89)
    assert np.array_equal(bits(again), bits(batch))                        # the same arguments, the same bits


def test_fo_smaller_than_a_row_needs(built_lib):
    x = mags(2, 5, 40, seed=5)
    got, n = check(built_lib, x, (40, 3), (16384, 65536), 50)              # row 0 needs 157
    assert n.tolist() == [50, 3]
    got, n = check(built_lib, x, (40, 40), (65536, 65536), 7)
    assert n.tolist() == [7, 7] and np.array_equal(bits(got), bits(x[:, :, :7]))


def test_out_of_range_steps_are_clamped_on_the_device(built_lib):
    x = mags(3, 4, 9, seed=6)
    got, n = check(built_lib, x, None, (0, -5, 2 ** 30), 33)
    want, wn = run(built_lib, x, None, (16384, 16384, 262144), 33)
    assert n.tolist() == wn.tolist() == [33, 33, 3] and np.array_equal(bits(got), bits(want))


def test_bad_arguments_enqueue_nothing(built_lib):
    """every TACO_EINVAL case returns before a launch: out and frames_out keep their fill, and the message names the argument"""
    lib = built_lib
    B, Cw, F, Fo = 2, 3, 8, 16
    x = dev(mags(B, Cw, F, seed=7))
    fr, st = dev([8, 5], torch.int32), dev([32768, 65536], torch.int32)
    G = Guarded({'out': ((B, Cw, Fo), torch.float32, 7.0), 'n': ((B,), torch.int32, 7.0)})
    fn = C.CDLL(lib.LIB_PATH).taco_frames_stretch
    fn.restype, fn.argtypes = lib.EXPORTS['taco_frames_stretch']
    good = dict(mag_t=lib.ptr(x), frames=lib.ptr(fr), per_unit=1, step_q=lib.ptr(st), out=lib.ptr(G['out']), frames_out=lib.ptr(G['n']),
                B=B, C=Cw, F=F, Fo=Fo)
    order = ('mag_t', 'frames', 'per_unit', 'step_q', 'out', 'frames_out', 'B', 'C', 'F', 'Fo')
    inside = C.c_void_p(x.data_ptr() + 4 * (B * Cw * F - 1))              # out begins on the last float of mag_t
    before = C.c_void_p(G['out'].data_ptr() + 4 * (B * Cw * Fo - 1))      # mag_t begins on the last float of out
    cases = [({'mag_t': None}, 'mag_t'), ({'out': None}, 'out'), ({'frames_out': None}, 'frames_out'), ({'out': good['mag_t']}, 'overlap'),
             ({'out': inside}, 'overlap'), ({'mag_t': before}, 'overlap'), ({'B': 0}, 'B='), ({'B': -1}, 'B='), ({'C': 0}, 'C='),
             ({'C': -7}, 'C='), ({'F': 0}, 'F='), ({'F': -1}, 'F='), ({'F': 8193}, 'F='), ({'Fo': 0}, 'Fo='), ({'Fo': -2}, 'Fo='),
             ({'Fo': 8193}, 'Fo='), ({'per_unit': 0}, 'frames_per_unit'), ({'per_unit': -3}, 'frames_per_unit')]
    everything = {k: torch.ones(G[k].shape, dtype=torch.bool, device='cuda') for k in ('out', 'n')}
    for change, word in cases:
        for nulls in ((), ('frames', 'step_q')):
            a = dict(good)
            a.update({k: None for k in nulls})
            a.update(change)
            lib.griffinlim_workspace_floats(1, 8)   # (a successful call in between: the string below is this refusal's)
            rc = fn(*[a[k] for k in order], lib.stream_ptr())
            torch.cuda.synchronize()
            msg = lib.last_error()
            print('  %r%s: rc %d, %s' % (change, ' frames / step_q NULL' if nulls else '', rc, msg))
            assert rc == -1, (change, rc)
            assert 'frames_stretch' in msg and word in msg, (change, msg)
            for name, m in everything.items():
                assert G.margin_intact(name, m), '%s was written although %r is refused' % (name, change)
    G.check()
    assert fn(*[good[k] for k in order], lib.stream_ptr()) == 0           # and the good arguments do run
    torch.cuda.synchronize()
    G.check('out', 'n')
    want, wn = sr.stretch(x.cpu().numpy(), [8, 5], [32768, 65536], 1, Fo)
    assert np.array_equal(bits(G['out'].cpu().numpy()), bits(want)) and G['n'].cpu().numpy().tolist() == wn.tolist() == [15, 5]


def test_graph_replay_follows_the_device_arguments(built_lib):
    """one capture of the one launch (a linear graph); the replay reads frames and step_q at replay time"""
    B, Cw, F, Fo = 3, 5, 20, 77
    xh = mags(B, Cw, F, seed=8)
    x = dev(xh)
    first = ([20, 9, 0], [65536, 16384, 100000])
    second = ([3, 20, 14], [262144, 30000, 65536])
    frames, steps = dev(first[0], torch.int32), dev(first[1], torch.int32)
    G = Guarded({'out': ((B, Cw, Fo), torch.float32, 'qnan'), 'n': ((B,), torch.int32, 'ones')})
    call = lambda: built_lib.frames_stretch(x, frames, steps, out=G['out'], frames_out=G['n'])   # noqa: E731
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            call()
    torch.cuda.synchronize()
    for fr, st in (first, second, first):
        frames.copy_(dev(fr, torch.int32))
        steps.copy_(dev(st, torch.int32))
        G.refill('out', 'n')
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        G.check('out', 'n')
        want, wn = sr.stretch(xh, fr, st, 1, Fo)
        assert G['n'].cpu().numpy().tolist() == wn.tolist()
        assert np.array_equal(bits(G['out'].cpu().numpy()), bits(want)), 'replay with frames %s, steps %s differs from the restatement' % (fr, st)
