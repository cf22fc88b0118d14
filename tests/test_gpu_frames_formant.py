"""GPU: taco_frames_formant against the float64 restatement (tests/formant_ref.py) within FORMANT_RTOL -- a bound measured on the CPU
from the float32 restatement on these same inputs (formant_ref.all_cases), never from the device -- the energy identity on the
device's own output, and bit for bit where the contract is exact: the copy at step 65536, the clamp of the step, the zeros behind a
row, position independence, repeatability, untouched surroundings.  Outputs sit between guard bands and start as poison."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import formant_ref as fr
from tests.poison import Guarded

pytestmark = pytest.mark.gpu


def dev(x, dtype=torch.float32):
    return torch.as_tensor(np.asarray(x), dtype=dtype).cuda()


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def run(lib, x, frames, steps, Q, per_unit=1, shift_in=0, shift_out=0):
    """one call on x (host array) -> out as a host array; out between guard bands, preset to NaN, mag_t and out `shift` floats behind
    a 256-byte boundary; the bands and the floats in front of a shifted out must be intact and mag_t unwritten.  frames and steps go
    to the device as they are: the device clamps them"""
    B, Cw, F = x.shape
    G = Guarded({'in': ((x.size + shift_in,), torch.float32, 'qnan'), 'out': ((x.size + shift_out,), torch.float32, 'qnan')})
    xin = G['in'][shift_in:].view(B, Cw, F)
    xin.copy_(torch.from_numpy(x))
    out = G['out'][shift_out:].view(B, Cw, F)
    assert xin.data_ptr() % 256 == 4 * shift_in and out.data_ptr() % 256 == 4 * shift_out
    got = lib.frames_formant(xin, None if frames is None else dev(frames, torch.int32), None if steps is None else dev(steps, torch.int32),
                             per_unit, Q, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    G.check()
    head = G['out'][:shift_out].cpu().numpy()
    assert np.isnan(head).all() and (bits(head) == 0x7fc00000).all(), 'the floats in front of out were written'
    assert torch.equal(xin.cpu().view(torch.int32), torch.from_numpy(x).view(torch.int32)), 'mag_t was written'
    return out.cpu().numpy()


def check(lib, name, x, frames, per_unit, steps, Q, **kw):
    """the call against the float64 restatement: finite, exact zeros behind each row and where the source is zero, within
    FORMANT_RTOL, a row at 65536 its source bit for bit, and the frame's energy (an element's relative error e moves its square by
    2 e: the bound is twice FORMANT_RTOL)"""
    want = fr.formant(x, frames, steps, per_unit, Q)
    got = run(lib, x, frames, steps, Q, per_unit, **kw)
    assert np.isfinite(got).all(), 'an element of out holds poison or a NaN from behind a row: %d' % int((~np.isfinite(got)).sum())
    B, _, F = x.shape
    for b in range(B):
        Fb = fr.row_frames(None if frames is None else frames[b], per_unit, F)
        assert not bits(got[b, :, Fb:]).any(), 'row %d: a bit is set behind frame %d' % (b, Fb)
        m = x[b, :, :Fb]
        assert not bits(got[b, :, :Fb][m == 0]).any(), 'row %d: a zero bin did not stay zero' % b
        if steps is None or fr.clamp_step(steps[b]) == fr.ONE:
            assert np.array_equal(bits(got[b, :, :Fb]), bits(m)), 'row %d at step 65536 is not its source' % b
        elif Fb:
            m64, y = m.astype(np.float64), got[b, :, :Fb].astype(np.float64)
            P0 = (m64 * m64).sum(axis=0)
            live = P0 > 0
            assert np.abs((y * y).sum(axis=0)[live] / P0[live] - 1.0).max(initial=0.0) <= 2.0 * fr.FORMANT_RTOL, 'row %d: the energy' % b
    err = fr.rel_err(got, want)
    print('  %s: B %d C %d F %d Q %d steps %s: largest relative error %.3g (bound %.3g)' % ((name,) + x.shape + (Q, steps, err, fr.FORMANT_RTOL)))
    assert err <= fr.FORMANT_RTOL
    return got


CASES = {c[0]: c[1:] for c in fr.all_cases()}
SHAPES = [(Cw, Q) for Cw, Qs in fr.SHAPES for Q in Qs]


@pytest.mark.parametrize('F', fr.EDGE_F)
@pytest.mark.parametrize('CQ', SHAPES, ids=lambda cq: 'C%d_Q%d' % cq)
def test_mixed_batch_at_small_and_odd_shapes(built_lib, CQ, F):
    """a cut row with NaN behind it, a row of zeros and an empty row of NaN in one call; F on each side of the 32-frame tile's edges,
    Q = 1, the largest, and both lifter paths; mag_t and out 1, 2 and 3 floats behind a 256-byte boundary; a step outside the range
    gives the bits of the clamped step"""
    x, frames, r, steps, Q = CASES['mixed_C%d_Q%d_F%d' % (CQ + (F,))]
    assert frames[2] == 0 and not x[1].any() and np.isnan(x[2]).all()
    a = check(built_lib, 'aligned', x, frames, r, steps, Q)
    assert not bits(a[1]).any() and not bits(a[2]).any()
    live = x[0, :, :frames[0]]
    assert np.abs(a[0, :, :frames[0]] / live - 1.0).max() > 0.01                                 # and a shifted row is not the source
    clamped = tuple(fr.clamp_step(s) for s in steps)
    if clamped != steps:
        assert np.array_equal(bits(run(built_lib, x, frames, clamped, Q, r)), bits(a)), 'a step outside the range is not the clamped one'
    for si, so in ((1, 3), (2, 1), (3, 2)):
        b = check(built_lib, 'shifted %d/%d' % (si, so), x, frames, r, steps, Q, shift_in=si, shift_out=so)
        assert np.array_equal(bits(a), bits(b)), 'the bits depend on the alignment'


def test_production_width(built_lib):
    x, frames, r, steps, Q = CASES['production']
    assert x.shape == (2, 1025, 40) and np.isnan(x[1, :, 37:]).all() and Q == 32
    check(built_lib, 'production', x, frames, r, steps, Q, shift_in=1, shift_out=3)


def test_bins_at_zero_under_the_floor_and_far_above(built_lib):
    x, frames, r, steps, Q = CASES['floor']
    assert {0.0, np.float32(1e-30), np.float32(1e4)} <= set(x[1].ravel().tolist()) and not x[0].any()
    got = check(built_lib, 'floor', x, frames, r, steps, Q)
    assert not bits(got[0]).any()                                                               # P1 == 0: g = 1, zeros stay zeros
    assert np.array_equal(got[4] != 0, x[4] != 0)


def test_a_row_at_one_beside_shifted_rows_is_copied_bit_for_bit(built_lib):
    x, frames, r, steps, Q = CASES['beside_one']
    assert steps[1] == fr.ONE and steps[0] != fr.ONE != steps[2]
    x = x.copy()
    x[1] = np.abs(x[1]) * np.float32(1e-30)          # denormals and tiny values survive a copy, not a log / exp
    got = check(built_lib, 'beside one', x, frames, r, steps, Q, shift_out=1)
    assert np.array_equal(bits(got[1]), bits(x[1]))
    got = run(built_lib, x, None, None, Q)                                                       # step_q NULL: every row
    assert np.array_equal(bits(got), bits(x))


def test_frames_per_unit_and_the_product_past_2_31(built_lib):
    x, frames, r, steps, Q = CASES['per_unit_3']
    assert r == 3 and 0 < frames[0] * r < x.shape[2] < frames[1] * r
    check(built_lib, 'per_unit', x, frames, r, steps, Q)
    x, frames, r, steps, Q = CASES['past_2_31']
    assert frames[0] * r > 2 ** 31 and frames[1] * r < -2 ** 31
    got = check(built_lib, 'past 2^31', x, frames, r, steps, Q)      # the product is formed in 64 bits: all F frames, and none
    assert not bits(got[1]).any() and got[0].all()
    check(built_lib, 'frames NULL', x, None, 1, steps, Q)


def test_a_frame_does_not_depend_on_where_it_is(built_lib):
    """permute the frames of a row, move the row to another batch index, pad F, shift the buffers by one float on either side: each
    frame's bits stay; and twice the same call; and row b of a B-row call is the call on that row alone"""
    lib = built_lib
    Cw, F, Q, s = 33, 37, 16, fr.formant_step(-3)
    row = fr.moving_comb(Cw, F, seed=9)
    base = run(lib, row[None], None, (s,), Q)[0]
    assert np.array_equal(bits(run(lib, row[None], None, (s,), Q)[0]), bits(base))              # the same arguments, the same bits
    for si, so in ((1, 0), (0, 1)):
        assert np.array_equal(bits(run(lib, row[None], None, (s,), Q, shift_in=si, shift_out=so)[0]), bits(base)), 'alignment'
    perm = np.random.default_rng(3).permutation(F)
    got = run(lib, np.ascontiguousarray(row[:, perm])[None], None, (s,), Q)[0]
    assert np.array_equal(bits(got), bits(base[:, perm])), 'a frame changed with its position'
    batch = np.stack([fr.moving_comb(Cw, F, seed=10), np.full((Cw, F), np.nan, dtype=np.float32), row])
    got = run(lib, batch, (F, 0, F), (fr.formant_step(5), 40000, s), Q)
    assert np.array_equal(bits(got[2]), bits(base)), 'a row changed with its batch index'
    wide = np.full((1, Cw, 70), np.nan, dtype=np.float32)
    wide[0, :, :F] = row
    got = run(lib, wide, (F,), (s,), Q, shift_in=1, shift_out=2)
    assert np.array_equal(bits(got[0, :, :F]), bits(base)) and not bits(got[0, :, F:]).any(), 'a frame changed with F'


def test_bad_arguments_enqueue_nothing(built_lib):
    """every TACO_EINVAL case returns before a launch: out keeps its fill, and the message names the argument"""
    lib = built_lib
    xh, frames, _, steps, Q = CASES['refusal_good']
    B, Cw, F = xh.shape
    assert (Cw, Q) == (17, 4)
    x, fr_d, st = dev(xh), dev(frames, torch.int32), dev(steps, torch.int32)
    G = Guarded({'out': ((B, Cw, F), torch.float32, 7.0)})
    fn = C.CDLL(lib.LIB_PATH).taco_frames_formant
    fn.restype, fn.argtypes = lib.EXPORTS['taco_frames_formant']
    good = dict(mag_t=lib.ptr(x), frames=lib.ptr(fr_d), per_unit=1, step_q=lib.ptr(st), lifter=Q, out=lib.ptr(G['out']), B=B, C=Cw, F=F)
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
        for nulls in ((), ('frames',), ('step_q',), ('frames', 'step_q')):
            a = dict(good)
            a.update({k: None for k in nulls})
            a.update(change)
            lib.griffinlim_workspace_floats(1, 8)   # (a successful call in between: the string below is this refusal's)
            rc = fn(*[a[k] for k in order], lib.stream_ptr())
            torch.cuda.synchronize()
            msg = lib.last_error()
            print('  %r%s: rc %d, %s' % (change, ' NULL: %s' % (nulls,) if nulls else '', rc, msg))
            assert rc == -1, (change, rc)
            assert 'frames_formant' in msg and word in msg, (change, msg)
            assert G.margin_intact('out', everything), 'out was written although %r is refused' % (change,)
    G.check()
    assert fn(*[good[k] for k in order], lib.stream_ptr()) == 0           # and the good arguments do run
    torch.cuda.synchronize()
    G.check('out')
    assert fr.rel_err(G['out'].cpu().numpy(), fr.formant(xh, frames, steps, 1, Q)) <= fr.FORMANT_RTOL


def test_graph_replay_follows_the_device_arguments(built_lib):
    """one capture of the one launch; the replay reads frames and step_q at replay time"""
    xh = CASES['replay_first'][0]
    Q = CASES['replay_first'][4]
    B, Cw, F = xh.shape
    x = dev(xh)
    first, second = ((CASES['replay_' + name][1], CASES['replay_' + name][3]) for name in ('first', 'second'))
    assert first != second
    frames, steps = dev(first[0], torch.int32), dev(first[1], torch.int32)
    G = Guarded({'out': ((B, Cw, F), torch.float32, 'qnan')})
    call = lambda: built_lib.frames_formant(x, frames, steps, 1, Q, out=G['out'])   # noqa: E731
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            call()
    torch.cuda.synchronize()
    for fr_h, st_h in (first, second, first):
        frames.copy_(dev(fr_h, torch.int32))
        steps.copy_(dev(st_h, torch.int32))
        G.refill('out')
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        G.check('out')
        got = G['out'].cpu().numpy()
        assert fr.rel_err(got, fr.formant(xh, fr_h, st_h, 1, Q)) <= fr.FORMANT_RTOL, 'replay with frames %s steps %s' % (fr_h, st_h)
        for b in range(B):
            assert not bits(got[b, :, fr_h[b]:]).any()
