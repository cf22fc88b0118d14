"""GPU: taco_frames_cepstats against the float64 restatement (tests/sharpen_ref.py): the variances made of its sums within
CEPSTATS_RTOL -- a bound measured on the CPU from the float32 restatement on these same inputs (sharpen_ref.all_cases), never from
the device -- the counts exactly, and bit for bit where the contract is exact: rows that do not know their neighbours, repeatability,
untouched surroundings.  sums, count and the workspace sit between guard bands and start as poison."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import sharpen_ref as sr
from tests.poison import Guarded

pytestmark = pytest.mark.gpu


def dev(x, dtype=torch.float32):
    return torch.as_tensor(np.asarray(x), dtype=dtype).cuda()


def raw_fn(lib):
    fn = C.CDLL(lib.LIB_PATH).taco_frames_cepstats
    fn.restype, fn.argtypes = lib.EXPORTS['taco_frames_cepstats']
    return fn


def at(t, shift):
    return C.c_void_p(t.data_ptr() + 4 * shift)


def run(lib, x, frames, Q, per_unit=1, shift=(0, 0, 0), fill='qnan'):
    """one call on x (host array) through the C ABI -> (sums (B, Q + 1, 2) float64, count (B)) as host arrays; mag_t, sums and the
    workspace shift[0..2] floats behind a 256-byte boundary (sums then is not 8-byte aligned), each between guard bands, outputs and
    workspace poisoned on entry; the bands and the floats around the shifted buffers must be intact and mag_t unwritten"""
    B, Cw, F = x.shape
    si, ss, sw = shift
    nsum, wbytes = B * (Q + 1) * 2 * 2, lib.frames_cepstats_workspace_bytes(B, Cw, F, Q)
    assert wbytes % 4 == 0
    G = Guarded({'in': ((x.size + si,), torch.float32, 'qnan'), 'sums': ((nsum + ss + 1,), torch.float32, fill),
                 'count': ((B,), torch.int32, 'ones'), 'ws': ((wbytes // 4 + sw + 1,), torch.float32, fill)})
    xin = G['in'][si:].view(B, Cw, F)
    xin.copy_(torch.from_numpy(x))
    fr = None if frames is None else dev(frames, torch.int32)
    before = {k: G[k].cpu().numpy().view(np.uint32).copy() for k in ('sums', 'ws')}
    rc = raw_fn(lib)(lib.ptr(xin), lib.ptr(fr), per_unit, Q, at(G['sums'], ss), lib.ptr(G['count']), at(G['ws'], sw), B, Cw, F,
                     lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, lib.last_error()
    G.check('count')
    words = G['sums'].cpu().numpy().view(np.uint32)
    assert np.array_equal(words[:ss], before['sums'][:ss]) and np.array_equal(words[ss + nsum:], before['sums'][ss + nsum:]), \
        'a float next to sums was written'
    ws = G['ws'].cpu().numpy().view(np.uint32)
    assert np.array_equal(ws[:sw], before['ws'][:sw]) and np.array_equal(ws[sw + wbytes // 4:], before['ws'][sw + wbytes // 4:]), \
        'a float next to the workspace was written'
    assert torch.equal(xin.cpu().view(torch.int32), torch.from_numpy(x).view(torch.int32)), 'mag_t was written'
    sums = words[ss:ss + nsum].copy().view(np.float64).reshape(B, Q + 1, 2)
    return sums, G['count'].cpu().numpy()


def check(lib, name, x, frames, per_unit, Q, **kw):
    want, n = sr.cepstats(x, frames, per_unit, Q)
    sums, count = run(lib, x, frames, Q, per_unit, **kw)
    assert np.isfinite(sums).all(), 'sums holds poison or a NaN from behind a row'
    for b in range(x.shape[0]):
        if n[b] == 0:
            assert not sums[b].view(np.uint64).any(), 'row %d has no frames and sums that are not +0' % b
    err = sr.var_err(sums, count, want, n)
    # the mean level c[0] of a row is the mean of its log-magnitudes (up to 18.4 in size, each rounded once at 6e-8 of that, and summed):
    # CEPSTATS_RTOL of 1 + |c[0]| is generous for it
    live = n > 0
    mean, mean_want = sums[live, 0, 0] / n[live], want[live, 0, 0] / n[live]
    assert (np.abs(mean - mean_want) <= sr.CEPSTATS_RTOL * (1.0 + np.abs(mean_want))).all()
    print('  %s: B %d C %d F %d Q %d: largest relative error of a variance %.3g (bound %.3g)' % ((name,) + x.shape + (Q, err, sr.CEPSTATS_RTOL)))
    assert err <= sr.CEPSTATS_RTOL
    return sums, count


CASES = {c[0]: c[1:] for c in sr.all_cases()}
SHAPES = [(Cw, Q) for Cw, Qs in sr.SHAPES for Q in Qs]


@pytest.mark.parametrize('F', sr.EDGE_F)
@pytest.mark.parametrize('CQ', SHAPES, ids=lambda cq: 'C%d_Q%d' % cq)
def test_mixed_batch_at_small_and_odd_shapes(built_lib, CQ, F):
    """a cut row with NaN behind it, a row of zeros and an empty row of NaN in one call; F on each side of the 32-frame tile's edges,
    Q = 2, the largest, and both lifter paths; mag_t, sums and the workspace 1, 2 and 3 floats behind a 256-byte boundary"""
    x, frames, r, _, Q = CASES['mixed_C%d_Q%d_F%d' % (CQ + (F,))]
    a, n = check(built_lib, 'aligned', x, frames, r, Q)
    assert list(n) == list(frames)
    assert abs(a[1, 0, 0] / (F * np.log(sr.FLOOR)) - 1.0) < 1e-5                      # the row of zeros: the floor's logarithm
    for shift, fill in (((1, 3, 2), 'noise'), ((2, 1, 3), 'ones'), ((3, 2, 1), 'qnan')):
        b, _ = check(built_lib, 'shifted %s' % (shift,), x, frames, r, Q, shift=shift, fill=fill)
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), 'the bits depend on the alignment or on the workspace contents'


def test_production_width(built_lib):
    x, frames, r, _, Q = CASES['production']
    check(built_lib, 'production', x, frames, r, Q, shift=(1, 1, 1), fill='noise')


def test_frames_per_unit_and_the_product_past_2_31(built_lib):
    x, frames, r, _, Q = CASES['per_unit_3']
    _, n = check(built_lib, 'per_unit', x, frames, r, Q)
    assert list(n) == [9, 40, 0]
    x, frames, r, _, Q = CASES['past_2_31']
    _, n = check(built_lib, 'past 2^31', x, frames, r, Q)        # the product is formed in 64 bits: all F frames, and none
    assert list(n) == [40, 0]
    _, n = check(built_lib, 'frames NULL', x, None, 1, Q)
    assert list(n) == [40, 40]


def test_a_row_does_not_depend_on_its_neighbours_and_the_lib_wrapper(built_lib):
    """a row alone, and the same row among others with NaN rows and NaN columns behind it at a larger F: the same bits; twice the same
    call: the same bits; and tacotron_amd.lib's wrapper returns what the C call returns"""
    lib = built_lib
    Cw, F, Q = 33, 37, 16
    row = sr.moving_comb(Cw, F, seed=9)
    base, _ = run(lib, row[None], None, Q)
    again, _ = run(lib, row[None], None, Q, fill='noise')
    assert np.array_equal(base.view(np.uint64), again.view(np.uint64))
    wide = np.full((3, Cw, 70), np.nan, dtype=np.float32)
    wide[0, :, :50] = sr.moving_comb(Cw, 50, seed=10)
    wide[2, :, :F] = row
    got, n = run(lib, wide, (50, 0, F), Q, shift=(1, 1, 3))
    assert np.array_equal(got[2].view(np.uint64), base[0].view(np.uint64)) and list(n) == [50, 0, F]
    sums, count = lib.frames_cepstats(dev(wide), Q, dev((50, 0, F), torch.int32))
    assert sums.dtype == torch.float64 and count.dtype == torch.int32
    assert np.array_equal(sums.cpu().numpy().view(np.uint64), got.view(np.uint64)) and count.tolist() == [50, 0, F]
    host = lib.gv_ratio(sums.cpu().numpy()[[0, 2]], count.cpu().numpy()[[0, 2]], got[[2, 0]], n[[2, 0]])
    want = sr.gv_ratio(got[[0, 2]], n[[0, 2]], got[[2, 0]], n[[2, 0]])
    assert np.allclose(host, want, rtol=1e-12) and abs(host[0] * host[1] - 1.0) < 1e-9


def test_bad_arguments_enqueue_nothing(built_lib):
    """every TACO_EINVAL case returns before a launch: sums, count and the workspace keep their fill, and the message names the
    argument; the size function refuses the same shapes"""
    lib = built_lib
    xh, frames, _, _, Q = CASES['refusal_good']
    B, Cw, F = xh.shape
    x, fr = dev(xh), dev(frames, torch.int32)
    wbytes = lib.frames_cepstats_workspace_bytes(B, Cw, F, Q)
    G = Guarded({'sums': ((B, Q + 1, 2), torch.float64, 7.0), 'count': ((B,), torch.int32, 'ones'), 'ws': ((wbytes,), torch.uint8, 'qnan')})
    fn = raw_fn(lib)
    good = dict(mag_t=lib.ptr(x), frames=lib.ptr(fr), per_unit=1, lifter=Q, sums=lib.ptr(G['sums']), count=lib.ptr(G['count']),
                ws=lib.ptr(G['ws']), B=B, C=Cw, F=F)
    order = ('mag_t', 'frames', 'per_unit', 'lifter', 'sums', 'count', 'ws', 'B', 'C', 'F')
    cases = [({'mag_t': None}, 'mag_t'), ({'sums': None}, 'sums'), ({'count': None}, 'count'), ({'ws': None}, 'workspace'),
             ({'B': 0}, 'B='), ({'B': -1}, 'B='), ({'F': 0}, 'F='), ({'F': -1}, 'F='), ({'F': 8193}, 'F='),
             ({'C': 0}, 'C='), ({'C': 5}, 'C='), ({'C': 16}, 'C='), ({'C': 18}, 'C='), ({'C': 2049}, 'C='), ({'C': -17}, 'C='),
             ({'lifter': 1}, 'lifter'), ({'lifter': 0}, 'lifter'), ({'lifter': -1}, 'lifter'), ({'lifter': 9}, 'lifter'),
             ({'lifter': 65, 'C': 1025}, 'lifter'), ({'per_unit': 0}, 'frames_per_unit'), ({'per_unit': -3}, 'frames_per_unit')]
    masks = {k: torch.ones(G[k].shape, dtype=torch.bool, device='cuda') for k in ('sums', 'count', 'ws')}
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
            assert 'frames_cepstats' in msg and word in msg, (change, msg)
            for k, m in masks.items():
                assert G.margin_intact(k, m), '%s was written although %r is refused' % (k, change)
    for bad in ((0, Cw, F, Q), (B, 16, F, Q), (B, Cw, 0, Q), (B, Cw, 8193, Q), (B, Cw, F, 1), (B, Cw, F, 9)):
        with pytest.raises(lib.TacoError):
            lib.frames_cepstats_workspace_bytes(*bad)
    G.check()
    assert fn(*[good[k] for k in order], lib.stream_ptr()) == 0           # and the good arguments do run
    torch.cuda.synchronize()
    G.check('sums', 'count')
    want, n = sr.cepstats(xh, frames, 1, Q)
    assert sr.var_err(G['sums'].cpu().numpy(), G['count'].cpu().numpy(), want, n) <= sr.CEPSTATS_RTOL


def test_graph_replay_follows_the_device_arguments(built_lib):
    """one capture of the two launches (a linear graph); the replay reads frames at replay time"""
    xh, _, _, _, Q = CASES['replay_first']
    B, Cw, F = xh.shape
    x = dev(xh)
    first, second = (CASES['replay_' + name][1] for name in ('first', 'second'))
    frames = dev(first, torch.int32)
    wbytes = built_lib.frames_cepstats_workspace_bytes(B, Cw, F, Q)
    G = Guarded({'sums': ((B, Q + 1, 2), torch.float64, 'qnan'), 'count': ((B,), torch.int32, 'ones'), 'ws': ((wbytes,), torch.uint8, 'qnan')})
    call = lambda: built_lib.frames_cepstats(x, Q, frames, out=(G['sums'], G['count']), workspace=G['ws'])   # noqa: E731
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
        G.refill('sums', 'count', 'ws')
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        G.check('sums', 'count')
        want, n = sr.cepstats(xh, fr, 1, Q)
        assert sr.var_err(G['sums'].cpu().numpy(), G['count'].cpu().numpy(), want, n) <= sr.CEPSTATS_RTOL, 'replay with frames %s' % (fr,)
