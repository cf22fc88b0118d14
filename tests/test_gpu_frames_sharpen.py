"""GPU: taco_frames_sharpen against the float64 restatement (tests/sharpen_ref.py) within SHARPEN_RTOL -- a bound measured on the CPU
from the float32 restatement on these same inputs (sharpen_ref.all_cases), never from the device -- the cepstral and the energy
identity on the device's own output, and bit for bit where the contract is exact: the copy at beta 0, the zeros behind a row,
position independence, repeatability, untouched surroundings.  Outputs sit between guard bands and start as poison."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import sharpen_ref as sr
from tests.poison import Guarded

pytestmark = pytest.mark.gpu


def dev(x, dtype=torch.float32):
    return torch.as_tensor(np.asarray(x), dtype=dtype).cuda()


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def run(lib, x, frames, beta, Q, per_unit=1, shift_in=0, shift_out=0):
    """one call on x (host array) -> out as a host array; out between guard bands, preset to NaN, mag_t and out `shift` floats behind
    a 256-byte boundary; the bands and the floats in front of a shifted out must be intact and mag_t unwritten"""
    B, Cw, F = x.shape
    G = Guarded({'in': ((x.size + shift_in,), torch.float32, 'qnan'), 'out': ((x.size + shift_out,), torch.float32, 'qnan')})
    xin = G['in'][shift_in:].view(B, Cw, F)
    xin.copy_(torch.from_numpy(x))
    out = G['out'][shift_out:].view(B, Cw, F)
    assert xin.data_ptr() % 256 == 4 * shift_in and out.data_ptr() % 256 == 4 * shift_out
    got = lib.frames_sharpen(xin, beta, Q, None if frames is None else dev(frames, torch.int32), per_unit, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    G.check()
    head = G['out'][:shift_out].cpu().numpy()
    assert np.isnan(head).all() and (bits(head) == 0x7fc00000).all(), 'the floats in front of out were written'
    assert torch.equal(xin.cpu().view(torch.int32), torch.from_numpy(x).view(torch.int32)), 'mag_t was written'
    return out.cpu().numpy()


def identities(x, got, frames, per_unit, beta, Q):
    """on the device's output, in float64, for the rows whose live bins all lie above the floor: c'[n] = (1 + beta) c[n] for
    2 <= n <= Q, c'[n] = c[n] for n = 1 and n > Q, and the frame's energy.  A relative error e of an element of out moves its
    logarithm by e and a cepstral coefficient -- a mean of logarithms under weights of at most 1 -- by at most e: the bound is
    SHARPEN_RTOL itself, and twice that for the sum of squares."""
    B, Cw, F = x.shape
    for b in range(B):
        Fb = sr.row_frames(None if frames is None else frames[b], per_unit, F)
        m = x[b, :, :Fb].astype(np.float64)
        if Fb == 0 or not (m > sr.FLOOR).all():
            continue
        y = got[b, :, :Fb].astype(np.float64)
        c, cy = sr.cepstra(m, Cw - 1), sr.cepstra(y, Cw - 1)
        scale = np.ones(Cw)[:, None]
        scale[sr.FIRST:Q + 1] = 1.0 + beta
        assert np.abs(cy[1:] - (scale * c)[1:]).max() <= sr.SHARPEN_RTOL, 'row %d: the cepstral identity' % b
        assert np.abs((y * y).sum(axis=0) / (m * m).sum(axis=0) - 1.0).max() <= 2.0 * sr.SHARPEN_RTOL, 'row %d: the energy' % b


def check(lib, name, x, frames, per_unit, beta, Q, **kw):
    """the call against the float64 restatement: finite, exact zeros behind each row, within SHARPEN_RTOL, and the identities"""
    want = sr.sharpen(x, beta, frames, per_unit, Q)
    got = run(lib, x, frames, beta, Q, per_unit, **kw)
    assert np.isfinite(got).all(), 'an element of out holds poison or a NaN from behind a row: %d' % int((~np.isfinite(got)).sum())
    B, _, F = x.shape
    for b in range(B):
        Fb = sr.row_frames(None if frames is None else frames[b], per_unit, F)
        assert not bits(got[b, :, Fb:]).any(), 'row %d: a bit is set behind frame %d' % (b, Fb)
    err = sr.rel_err(got, want)
    print('  %s: B %d C %d F %d Q %d beta %g: largest relative error %.3g (bound %.3g)' % ((name,) + x.shape + (Q, beta, err, sr.SHARPEN_RTOL)))
    assert err <= sr.SHARPEN_RTOL
    identities(x, got, frames, per_unit, beta, Q)
    return got


CASES = {c[0]: c[1:] for c in sr.all_cases()}
SHAPES = [(Cw, Q) for Cw, Qs in sr.SHAPES for Q in Qs]


@pytest.mark.parametrize('F', sr.EDGE_F)
@pytest.mark.parametrize('CQ', SHAPES, ids=lambda cq: 'C%d_Q%d' % cq)
def test_mixed_batch_at_small_and_odd_shapes(built_lib, CQ, F):
    """a cut row with NaN behind it, a row of zeros and an empty row of NaN in one call; F on each side of the 32-frame tile's edges,
    Q = 2, the largest, and both lifter paths; mag_t and out 1, 2 and 3 floats behind a 256-byte boundary"""
    x, frames, r, beta, Q = CASES['mixed_C%d_Q%d_F%d' % (CQ + (F,))]
    assert frames[2] == 0 and not x[1].any() and np.isnan(x[2]).all()
    a = check(built_lib, 'aligned', x, frames, r, beta, Q)
    assert not bits(a[1]).any() and not bits(a[2]).any()
    if F > 1:
        assert np.abs(a[0, :, :frames[0]] / x[0, :, :frames[0]] - 1.0).max() > 0.01          # and a sharpened row is not the source
    for si, so in ((1, 3), (2, 1), (3, 2)):
        b = check(built_lib, 'shifted %d/%d' % (si, so), x, frames, r, beta, Q, shift_in=si, shift_out=so)
        assert np.array_equal(bits(a), bits(b)), 'the bits depend on the alignment'


def test_production_width(built_lib):
    x, frames, r, beta, Q = CASES['production']
    assert x.shape == (2, 1025, 40) and np.isnan(x[1, :, 37:]).all()
    check(built_lib, 'production', x, frames, r, beta, Q, shift_in=1, shift_out=3)


def test_beta_zero_copies_bit_for_bit(built_lib):
    x, frames, r, _, Q = CASES['mixed_C129_Q33_F65']
    got = run(built_lib, x, frames, 0.0, Q, shift_out=1)
    assert np.array_equal(bits(got[0, :, :frames[0]]), bits(x[0, :, :frames[0]])) and not bits(got[0, :, frames[0]:]).any()
    assert not bits(got[1:]).any()
    x = np.abs(CASES['per_unit_3'][0]) * np.float32(1e-30)          # denormals and tiny values survive a copy, not a log / exp
    got = run(built_lib, x, None, -0.0, 16)
    assert np.array_equal(bits(got), bits(x))


def test_frames_per_unit_and_the_product_past_2_31(built_lib):
    x, frames, r, beta, Q = CASES['per_unit_3']
    assert 0 < frames[0] * r < x.shape[2] < frames[1] * r
    check(built_lib, 'per_unit', x, frames, r, beta, Q)
    x, frames, r, beta, Q = CASES['past_2_31']
    assert frames[0] * r > 2 ** 31 and frames[1] * r < -2 ** 31
    got = check(built_lib, 'past 2^31', x, frames, r, beta, Q)      # the product is formed in 64 bits: all F frames, and none
    assert not bits(got[1]).any() and got[0].all()
    check(built_lib, 'frames NULL', x, None, 1, beta, Q)


def test_a_frame_does_not_depend_on_where_it_is(built_lib):
    """permute the frames of a row, move the row to another batch index, pad F: each frame's bits stay; and twice the same call"""
    lib = built_lib
    Cw, F, Q, beta = 33, 37, 16, 0.55
    row = sr.moving_comb(Cw, F, seed=9)
    base = run(lib, row[None], None, beta, Q)[0]
    assert np.array_equal(bits(run(lib, row[None], None, beta, Q)[0]), bits(base))          # the same arguments, the same bits
    perm = np.random.default_rng(3).permutation(F)
    got = run(lib, np.ascontiguousarray(row[:, perm])[None], None, beta, Q)[0]
    assert np.array_equal(bits(got), bits(base[:, perm])), 'a frame changed with its position'
    batch = np.stack([sr.moving_comb(Cw, F, seed=10), np.full((Cw, F), np.nan, dtype=np.float32), row])
    got = run(lib, batch, (F, 0, F), beta, Q)
    assert np.array_equal(bits(got[2]), bits(base)), 'a row changed with its batch index'
    wide = np.full((1, Cw, 70), np.nan, dtype=np.float32)
    wide[0, :, :F] = row
    got = run(lib, wide, (F,), beta, Q, shift_in=1, shift_out=2)
    assert np.array_equal(bits(got[0, :, :F]), bits(base)) and not bits(got[0, :, F:]).any(), 'a frame changed with F'


def test_bad_arguments_enqueue_nothing(built_lib):
    """every TACO_EINVAL case returns before a launch: out keeps its fill, and the message names the argument"""
    lib = built_lib
    xh, frames, _, beta, Q = CASES['refusal_good']
    B, Cw, F = xh.shape
    assert (Cw, Q) == (17, 4)
    x, fr = dev(xh), dev(frames, torch.int32)
    G = Guarded({'out': ((B, Cw, F), torch.float32, 7.0)})
    fn = C.CDLL(lib.LIB_PATH).taco_frames_sharpen
    fn.restype, fn.argtypes = lib.EXPORTS['taco_frames_sharpen']
    good = dict(mag_t=lib.ptr(x), frames=lib.ptr(fr), per_unit=1, beta=beta, lifter=Q, out=lib.ptr(G['out']), B=B, C=Cw, F=F)
    order = ('mag_t', 'frames', 'per_unit', 'beta', 'lifter', 'out', 'B', 'C', 'F')
    inside = C.c_void_p(x.data_ptr() + 4 * (B * Cw * F - 1))              # out begins on the last float of mag_t
    before = C.c_void_p(G['out'].data_ptr() + 4 * (B * Cw * F - 1))       # mag_t begins on the last float of out
    cases = [({'mag_t': None}, 'mag_t'), ({'out': None}, 'out'), ({'out': good['mag_t']}, 'overlap'), ({'out': inside}, 'overlap'),
             ({'mag_t': before}, 'overlap'), ({'B': 0}, 'B='), ({'B': -1}, 'B='), ({'F': 0}, 'F='), ({'F': -1}, 'F='), ({'F': 8193}, 'F='),
             ({'C': 0}, 'C='), ({'C': 5}, 'C='), ({'C': 16}, 'C='), ({'C': 18}, 'C='), ({'C': 2049}, 'C='), ({'C': -17}, 'C='),
             ({'lifter': 1}, 'lifter'), ({'lifter': 0}, 'lifter'), ({'lifter': -1}, 'lifter'), ({'lifter': 9}, 'lifter'),
             ({'lifter': 65, 'C': 1025}, 'lifter'), ({'per_unit': 0}, 'frames_per_unit'), ({'per_unit': -3}, 'frames_per_unit'),
             ({'beta': float('nan')}, 'beta'), ({'beta': 1.001}, 'beta'), ({'beta': -1.001}, 'beta'), ({'beta': float('inf')}, 'beta')]
    everything = torch.ones(G['out'].shape, dtype=torch.bool, device='cuda')
    for change, word in cases:
        for nulls in ((), ('frames',)):
            a = dict(good)
            a.update({k: None for k in nulls})
            a.update(change)
            lib.griffinlim_workspace_floats(1, 8)   # (a successful call in between: the string below is this refusal's)
            rc = fn(*[a[k] for k in order], lib.stream_ptr())
            torch.cuda.synchronize()
            msg = lib.last_error()
            print('  %r%s: rc %d, %s' % (change, ' frames NULL' if nulls else '', rc, msg))
            assert rc == -1, (change, rc)
            assert 'frames_sharpen' in msg and word in msg, (change, msg)
            assert G.margin_intact('out', everything), 'out was written although %r is refused' % (change,)
    G.check()
    assert fn(*[good[k] for k in order], lib.stream_ptr()) == 0           # and the good arguments do run
    torch.cuda.synchronize()
    G.check('out')
    assert sr.rel_err(G['out'].cpu().numpy(), sr.sharpen(xh, beta, frames, 1, Q)) <= sr.SHARPEN_RTOL


def test_graph_replay_follows_the_device_arguments(built_lib):
    """one capture of the one launch; the replay reads frames at replay time"""
    xh, _, _, beta, Q = CASES['replay_first']
    B, Cw, F = xh.shape
    x = dev(xh)
    first, second = (CASES['replay_' + name][1] for name in ('first', 'second'))
    frames = dev(first, torch.int32)
    G = Guarded({'out': ((B, Cw, F), torch.float32, 'qnan')})
    call = lambda: built_lib.frames_sharpen(x, beta, Q, frames, out=G['out'])   # noqa: E731
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            call()
    torch.cuda.synchronize()
    for fr in (first, second, first):
        frames.copy_(dev(fr, torch.int32))
        G.refill('out')
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        G.check('out')
        got = G['out'].cpu().numpy()
        assert sr.rel_err(got, sr.sharpen(xh, beta, fr, 1, Q)) <= sr.SHARPEN_RTOL, 'replay with frames %s' % (fr,)
        for b in range(B):
            assert not bits(got[b, :, fr[b]:]).any()
