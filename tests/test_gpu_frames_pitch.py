"""GPU: taco_frames_pitch against the float64 restatement (tests/pitch_ref.py) within PITCH_RTOL -- a bound measured on the CPU from
the float32 restatement on these same inputs (tests/pitch_cases.py), never from the device -- and bit for bit where the contract is
exact: the copy at step 65536, the zeros behind a row, position independence, repeatability, untouched surroundings.  Outputs sit
between guard bands and start as poison."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import pitch_cases as pc
from tests import pitch_ref as pr
from tests.poison import Guarded

pytestmark = pytest.mark.gpu


def dev(x, dtype=torch.float32):
    return torch.as_tensor(np.asarray(x), dtype=dtype).cuda()


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def run(lib, x, frames, steps, Q, per_unit=1, shift_in=0, shift_out=0):
    """one call on x (host array) -> out as a host array; out between guard bands, preset to NaN, mag_t and out `shift` floats behind
    a 256-byte boundary; the bands and the floats in front of a shifted out must be intact and mag_t unwritten"""
    B, Cw, F = x.shape
    G = Guarded({'in': ((x.size + shift_in,), torch.float32, 'qnan'), 'out': ((x.size + shift_out,), torch.float32, 'qnan')})
    xin = G['in'][shift_in:].view(B, Cw, F)
    xin.copy_(torch.from_numpy(x))
    out = G['out'][shift_out:].view(B, Cw, F)
    assert xin.data_ptr() % 256 == 4 * shift_in and out.data_ptr() % 256 == 4 * shift_out
    got = lib.frames_pitch(xin, None if frames is None else dev(frames, torch.int32), None if steps is None else dev(steps, torch.int32),
                           frames_per_unit=per_unit, lifter=Q, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    G.check()
    head = G['out'][:shift_out].cpu().numpy()
    assert np.isnan(head).all() and (bits(head) == 0x7fc00000).all(), 'the floats in front of out were written'
    assert torch.equal(xin.cpu().view(torch.int32), torch.from_numpy(x).view(torch.int32)), 'mag_t was written'
    return out.cpu().numpy()


def check(lib, name, x, frames, steps, per_unit, Q, **kw):
    """the call against the float64 restatement: finite, exact zeros behind each row, the copy rows bit for bit, the rest within
    PITCH_RTOL"""
    want = pr.shift(x, frames, steps, per_unit, Q)
    got = run(lib, x, frames, steps, Q, per_unit, **kw)
    assert np.isfinite(got).all(), 'an element of out holds poison or a NaN from behind a row: %d' % int((~np.isfinite(got)).sum())
    B, _, F = x.shape
    for b in range(B):
        Fb = pr.row_frames(None if frames is None else frames[b], per_unit, F)
        assert not bits(got[b, :, Fb:]).any(), 'row %d: a bit is set behind frame %d' % (b, Fb)
        if steps is None or pr.clamp_step(steps[b]) == pr.ONE:
            assert np.array_equal(bits(got[b, :, :Fb]), bits(x[b, :, :Fb])), 'row %d at step 65536 is not a copy' % b
    err = pc.rel_err(got, want)
    print('  %s: B %d C %d F %d Q %d: largest relative error %.3g (bound %.3g)' % ((name,) + x.shape + (Q, err, pr.PITCH_RTOL)))
    assert err <= pr.PITCH_RTOL
    return got


CASES = {c[0]: c[1:] for c in pc.all_cases()}


def test_mixed_batch(built_lib):
    """a copied, an empty, an octave-up, an octave-down and an odd-step row in one call at the production bin count, NaN in every
    source column behind a row's end"""
    x, frames, steps, r, Q = CASES['mixed']
    assert x.shape == (5, 1025, 23) and Q == 32 and np.isnan(x[2, :, 5:]).all()
    got = check(built_lib, 'mixed', x, frames, steps, r, Q)
    assert np.array_equal(bits(got[0]), bits(x[0])) and not bits(got[1]).any()
    assert np.abs(got[4, :, :23] / x[4, :, :23] - 1.0).max() > 0.1            # and a shifted row is not the source


@pytest.mark.parametrize('F', pc.EDGE_F)
@pytest.mark.parametrize('CQ', pc.SMALL, ids=lambda cq: 'C%d_Q%d' % cq)
def test_small_and_odd_shapes(built_lib, CQ, F):
    """a frame tile is 32 frames: F on each side of its edges; mag_t and out 1, 2 and 3 floats behind a 256-byte boundary"""
    x, frames, steps, r, Q = CASES['small_C%d_Q%d_F%d' % (CQ + (F,))]
    a = check(built_lib, 'aligned', x, frames, steps, r, Q)
    for si, so in ((1, 3), (2, 1), (3, 2)):
        b = check(built_lib, 'shifted %d/%d' % (si, so), x, frames, steps, r, Q, shift_in=si, shift_out=so)
        assert np.array_equal(bits(a), bits(b)), 'the bits depend on the alignment'


def test_floor(built_lib):
    """frames of all zeros, and frames mixing 0, 1e-30 and 1e4: finite, and the restatement's values"""
    x, frames, steps, r, Q = CASES['floor']
    got = check(built_lib, 'floor', x, frames, steps, r, Q)
    assert np.abs(got[0] / 1e-8 - 1.0).max() < 1e-4                            # log(floor) is all envelope: the floor comes back


@pytest.mark.parametrize('CQ', pc.LIFTER_PATHS, ids=lambda cq: 'C%d_Q%d' % cq)
def test_lifters_on_both_sides_of_32(built_lib, CQ):
    """up to 32 quefrencies are one block of cepstrum rows, 33 to 64 two"""
    check(built_lib, 'lifter', *CASES['lifter_C%d_Q%d' % CQ])


@pytest.mark.parametrize('r', [2, 3, 5])
def test_frames_per_unit(built_lib, r):
    x, frames, steps, per_unit, Q = CASES['per_unit_%d' % r]
    assert per_unit == r and frames[1] * r > x.shape[2] and 0 < frames[0] * r < x.shape[2]
    check(built_lib, 'per_unit', x, frames, steps, per_unit, Q)


def test_frames_product_past_2_31_clamps(built_lib):
    x, frames, steps, per_unit, Q = CASES['past_2_31']
    assert frames[0] * per_unit > 2 ** 31 and frames[1] * per_unit < -2 ** 31
    got = check(built_lib, 'past 2^31', x, frames, steps, per_unit, Q)     # the product is formed in 64 bits: all F frames, and none
    assert not bits(got[1]).any() and got[0].all()


def test_null_frames_null_steps_and_clamped_steps(built_lib):
    x, frames, steps, r, Q = CASES['clamped']
    got = check(built_lib, 'both NULL', x, None, None, r, Q)
    assert np.array_equal(bits(got), bits(x))
    a = check(built_lib, 'steps out of range', x, frames, steps, r, Q)
    b = run(built_lib, x, None, (32768, 32768, 131072), Q)
    assert np.array_equal(bits(a), bits(b))


def test_a_frame_does_not_depend_on_where_it_is(built_lib):
    """permute the frames of a row, move the row to another batch index, pad F: each frame's bits stay; and twice the same call"""
    lib = built_lib
    Cw, F, Q, step = 33, 37, 16, 50000
    row = pc.mags(1, Cw, F, seed=9)[0]
    base = run(lib, row[None], None, (step,), Q)[0]
    assert np.array_equal(bits(run(lib, row[None], None, (step,), Q)[0]), bits(base))          # the same arguments, the same bits
    perm = np.random.default_rng(3).permutation(F)
    got = run(lib, np.ascontiguousarray(row[:, perm])[None], None, (step,), Q)[0]
    assert np.array_equal(bits(got), bits(base[:, perm])), 'a frame changed with its position'
    batch = np.stack([pc.mags(1, Cw, F, seed=10)[0], np.full((Cw, F), np.nan, dtype=np.float32), row])
    got = run(lib, batch, (F, 0, F), (90000, 65536, step), Q)
    assert np.array_equal(bits(got[2]), bits(base)), 'a row changed with its batch index'
    wide = np.full((1, Cw, 70), np.nan, dtype=np.float32)
    wide[0, :, :F] = row
    got = run(lib, wide, (F,), (step,), Q, shift_in=1, shift_out=2)
    assert np.array_equal(bits(got[0, :, :F]), bits(base)) and not bits(got[0, :, F:]).any(), 'a frame changed with F'


def test_bad_arguments_enqueue_nothing(built_lib):
    """every TACO_EINVAL case returns before a launch: out keeps its fill, and the message names the argument"""
    lib = built_lib
    xh, frames, steps, _, Q = CASES['refusal_good']
    B, Cw, F = xh.shape
    assert (Cw, Q) == (17, 4)
    x, fr, st = dev(xh), dev(frames, torch.int32), dev(steps, torch.int32)
    G = Guarded({'out': ((B, Cw, F), torch.float32, 7.0)})
    fn = C.CDLL(lib.LIB_PATH).taco_frames_pitch
    fn.restype, fn.argtypes = lib.EXPORTS['taco_frames_pitch']
    good = dict(mag_t=lib.ptr(x), frames=lib.ptr(fr), per_unit=1, step_q=lib.ptr(st), lifter=Q, out=lib.ptr(G['out']), B=B, C=Cw, F=F)
    order = ('mag_t', 'frames', 'per_unit', 'step_q', 'lifter', 'out', 'B', 'C', 'F')
    inside = C.c_void_p(x.data_ptr() + 4 * (B * Cw * F - 1))              # out begins on the last float of mag_t
    before = C.c_void_p(G['out'].data_ptr() + 4 * (B * Cw * F - 1))       # mag_t begins on the last float of out
    cases = [({'mag_t': None}, 'mag_t'), ({'out': None}, 'out'), ({'out': good['mag_t']}, 'overlap'), ({'out': inside}, 'overlap'),
             ({'mag_t': before}, 'overlap'), ({'B': 0}, 'B='), ({'B': -1}, 'B='), ({'F': 0}, 'F='), ({'F': -1}, 'F='), ({'F': 8193}, 'F='),
             ({'C': 0}, 'C='), ({'C': 5}, 'C='), ({'C': 16}, 'C='), ({'C': 18}, 'C='), ({'C': 2049}, 'C='), ({'C': -17}, 'C='),
             ({'lifter': 0}, 'lifter'), ({'lifter': -1}, 'lifter'), ({'lifter': 9}, 'lifter'), ({'lifter': 65, 'C': 1025}, 'lifter'),
             ({'per_unit': 0}, 'frames_per_unit'), ({'per_unit': -3}, 'frames_per_unit')]
    everything = torch.ones(G['out'].shape, dtype=torch.bool, device='cuda')
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
            assert 'frames_pitch' in msg and word in msg, (change, msg)
            assert G.margin_intact('out', everything), 'out was written although %r is refused' % (change,)
    G.check()
    assert fn(*[good[k] for k in order], lib.stream_ptr()) == 0           # and the good arguments do run
    torch.cuda.synchronize()
    G.check('out')
    want = pr.shift(xh, frames, steps, 1, Q)
    assert pc.rel_err(G['out'].cpu().numpy(), want) <= pr.PITCH_RTOL


def test_graph_replay_follows_the_device_arguments(built_lib):
    """one capture of the one launch (a linear graph); the replay reads frames and step_q at replay time"""
    xh, _, _, _, Q = CASES['replay_first']
    B, Cw, F = xh.shape
    x = dev(xh)
    first, second = (CASES['replay_' + name][1:3] for name in ('first', 'second'))
    frames, steps = dev(first[0], torch.int32), dev(first[1], torch.int32)
    G = Guarded({'out': ((B, Cw, F), torch.float32, 'qnan')})
    call = lambda: built_lib.frames_pitch(x, frames, steps, lifter=Q, out=G['out'])   # noqa: E731
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
        G.refill('out')
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        G.check('out')
        got, want = G['out'].cpu().numpy(), pr.shift(xh, fr, st, 1, Q)
        assert pc.rel_err(got, want) <= pr.PITCH_RTOL, 'replay with frames %s, steps %s' % (fr, st)
        for b in range(B):
            if st[b] == 65536:
                assert np.array_equal(bits(got[b, :, :fr[b]]), bits(xh[b, :, :fr[b]]))
