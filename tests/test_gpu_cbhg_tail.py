"""GPU: the five hand-written kernels of the CBHG tail alone, through the taco_debug_* doors (include/taco_hip.h), against the fp64
oracle's own _gru / _highway / _prenet: bigru_fwd_kernel and bigru_bwd_kernel (csrc/bigru.hip), highway_stack_fwd_kernel<AD> and
highway_stack_bwd_kernel<AD> (csrc/highway.hip), mlp2_kernel forward and backward (csrc/prenet.hip).  Cases, operands, references
and judges live in tests/cbhg_tail_cases.py and tests/cbhg_tail_ref.py; tests/test_cbhg_tail_host.py holds them to account.

Every output goes through stage_bars.compare / failures as a whole tensor and row by row (a row is one (b, t) or one m).  Every
output buffer sits in a guarded arena (tests/poison.py) with a `qnan` fill and PAD_ROWS rows more than the call may write: the
guard bands and the rows at or beyond M must keep their fill, the written rows must be finite.  The x-side rows of the GRU kernels
(not an operand of the recurrence) are NaN.  Backward doors run isolated (fed the oracle's forward stash rounded to fp32) in every
case and chained (fed the forward door's own stash) in the cases of cbhg_tail_cases.CHAINED; one case per door runs on a non-default
stream.

Bars (tests/stage_bars.py CBHG_TAIL_BARS): 4 x the worst HIP-against-fp64 error over the case table on an MI355X, rounded up to
one significant digit, never above the project's ceilings.  Measured (worst tensor rel-L2 / worst row; the fp32 torch restatement
of the same op on the same cases beside it):

    kernel             tensor          row    fp32 tensor     fp32 row     bars (tensor, row)
    bigru_fwd       1.131e-07    1.336e-07      1.012e-07    1.244e-07     5e-7, 6e-7
    bigru_bwd       1.909e-07    2.033e-07      2.755e-07    2.755e-07     8e-7, 9e-7
    highway_fwd     2.478e-07    3.163e-07      3.365e-07    5.004e-07     1e-6, 2e-6
    highway_bwd     3.733e-07    5.882e-07      4.805e-07    6.423e-07     2e-6, 3e-6
    prenet_fwd      2.666e-07    3.748e-07      4.290e-07    4.290e-07     2e-6, 2e-6
    prenet_bwd      1.861e-07    2.245e-07      2.992e-07    2.992e-07     8e-7, 9e-7

(When CBHG_TAIL_ERRORS_OUT names a file the module writes this table there; profiles/cbhg_tail_errors.txt is such a file.)
No kernel is worse than the plain fp32 restatement by more than 1.1 x (bigru_fwd); most are a little better (MFMA accumulation,
fused multiply-adds).  No ReLU decision of any chained case differed from fp64's.

The gate of the highway kernel under a bias of -30 is sigmoid(-30 + ..) ~ 9e-14, an ordinary fp32 number and not zero (in fp64 as
well): T is required to be exactly 1 under +30, where 1 + exp(-x) rounds to 1, and below 2^-20 under -30; dT is required to be
exactly zero wherever the fp32 gate that the backward kernel reads is exactly 0 or 1, as for the GRU's u (1 - u).

nl < 4: the launchers accept 1..4 layers and the plain-form kernels are run here with 1, 2 and 3 (`plain-M33-nl*`)."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import cbhg_tail_cases as cc
from tests import cbhg_tail_ref as ref
from tests.poison import Guarded

pytestmark = pytest.mark.gpu

PAD_ROWS = 40        # rows behind the last one a call may write: more than a 32-row tile
STATS = {}           # kernel -> [worst tensor, worst row, the fp32 restatement's worst tensor, worst row]
H = 128


def dev(a, dtype=None):
    if a is None:
        return None
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


class Hip:
    """The doors behind the interface of cbhg_tail_ref.F32: numpy in, numpy out, outputs carved from a guarded arena"""

    def __init__(self, lib, side_stream=False):
        self.lib, self.side = lib, side_stream

    def _call(self, fn, *args, **kw):
        torch.cuda.synchronize()
        if self.side:
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                assert torch.cuda.current_stream() != torch.cuda.default_stream()
                fn(*args, **kw)
            s.synchronize()
        else:
            fn(*args, **kw)
        torch.cuda.synchronize()

    @staticmethod
    def _arena(spec):
        """spec: name -> (rows, cols): float32 outputs of `rows` rows, allocated with PAD_ROWS more"""
        return Guarded({n: ((r + PAD_ROWS, c), torch.float32, 'qnan') for n, (r, c) in spec.items()})

    @staticmethod
    def _collect(G, spec):
        """guard bands and slack bytes intact, rows at or beyond `rows` untouched -> the written rows as numpy"""
        G.check()
        out = {}
        for n, (r, c) in spec.items():
            mask = torch.zeros(G[n].shape, dtype=torch.bool, device='cuda')
            mask[r:] = True
            assert G.margin_intact(n, mask), '%s: a row at or beyond row %d was written' % (n, r)
            out[n] = G[n][:r].cpu().numpy()
        return out

    # -- bi-GRU
    def bigru_fwd(self, xg, w, h0=None):
        B, T, _ = xg.shape
        wd = {}
        for k, v in w.items():
            wd[k] = dev(v)
            wd[k][:H] = float('nan')        # the x side is not an operand of the recurrence
        spec = {'out': (B * T, 256), 'ruc': (B * T, 768)}
        G = self._arena(spec)
        self._call(self.lib.debug_bigru_rec_fwd, dev(xg), wd, G['out'][:B * T].view(B, T, 256), G['ruc'][:B * T].view(B, T, 768), dev(h0))
        o = self._collect(G, spec)
        return o['out'].reshape(B, T, 256), o['ruc'].reshape(B, T, 768)

    def bigru_bwd(self, dout, out, ruc, wT, h0=None, want_dh0=False):
        B, T, _ = dout.shape
        spec = {'dxg': (B * T, 768), 'rh': (B * T, 256), 'dh0': (2 * B, H)}
        G = self._arena(spec)
        self._call(self.lib.debug_bigru_bwd, dev(dout), dev(out), dev(ruc), {k: dev(v) for k, v in wT.items()},
                   G['dxg'][:B * T].view(B, T, 768), G['rh'][:B * T].view(B, T, 256), dev(h0),
                   G['dh0'][:2 * B].view(2, B, H) if want_dh0 else None)
        if not want_dh0:
            spec['dh0'] = (0, H)            # nothing of it may be written
        o = self._collect(G, spec)
        return o['dxg'].reshape(B, T, 768), o['rh'].reshape(B, T, 256), (o['dh0'].reshape(2, B, H) if want_dh0 else None)

    # -- highway stack
    def highway_fwd(self, x, p, nl, T=None):
        M = x.shape[0]
        ad = 'wa' in p
        spec = {}
        for l in range(nl):
            spec.update({'y%d' % l: (M, H), 'th%d' % l: (M, 256)})
            if ad:
                spec['hx%d' % l] = (M, H)
        G = self._arena(spec)
        L = lambda k: [dev(a) for a in p[k]]
        V = lambda k: [G['%s%d' % (k, l)][:M] for l in range(nl)]
        kw = dict(wa=L('wa'), rowb=L('rowb'), hx=V('hx'), T=T) if ad else {}
        self._call(self.lib.debug_highway_stack_fwd, dev(x), L('wt'), L('bt'), L('wh'), L('bh'), V('y'), th=V('th'), **kw)
        o = self._collect(G, spec)
        return {'y': [o['y%d' % l] for l in range(nl)], 'th': [o['th%d' % l] for l in range(nl)],
                'hx': [o['hx%d' % l] for l in range(nl)] if ad else None}

    def highway_bwd(self, g, wT, th, x, waT=None):
        nl, M = len(th), g.shape[0]
        ad = waT is not None
        spec = {'gout': (M, H)}
        for l in range(nl):
            spec['dth%d' % l] = (M, 256)
            if ad:
                spec['dhx%d' % l] = (M, H)
        G = self._arena(spec)
        V = lambda k: [G['%s%d' % (k, l)][:M] for l in range(nl)]
        kw = dict(waT=[dev(a) for a in waT], dhx=V('dhx')) if ad else {}
        self._call(self.lib.debug_highway_stack_bwd, dev(g), [dev(a) for a in wT], [dev(a) for a in th], [dev(a) for a in x], V('dth'),
                   G['gout'][:M], **kw)
        o = self._collect(G, spec)
        return {'dth': [o['dth%d' % l] for l in range(nl)], 'gout': o['gout'], 'dhx': [o['dhx%d' % l] for l in range(nl)] if ad else None}

    # -- pre-net
    def prenet_fwd(self, x, p, k1=None, k2=None):
        M = x.shape[0]
        spec = {'y1': (M, 256), 'y2': (M, H)}
        G = self._arena(spec)
        self._call(self.lib.debug_prenet_fwd, dev(x), dev(p['w1']), dev(p['b1']), dev(p['w2']), dev(p['b2']), G['y1'][:M], G['y2'][:M],
                   keep1=dev(k1), keep2=dev(k2))
        o = self._collect(G, spec)
        return o['y1'], o['y2']

    def prenet_bwd(self, dy2, w2T, w1T, y1, y2, k1=None, k2=None):
        M = dy2.shape[0]
        spec = {'dz2': (M, H), 'dz1': (M, 256), 'dx': (M, 256)}
        G = self._arena(spec)
        self._call(self.lib.debug_prenet_bwd, dev(dy2), dev(w2T), dev(w1T), dev(y1), dev(y2), G['dz2'][:M], G['dz1'][:M], G['dx'][:M],
                   keep1=dev(k1), keep2=dev(k2))
        o = self._collect(G, spec)
        return o['dz2'], o['dz1'], o['dx']


@functools.lru_cache(maxsize=None)
def _f32_report(kind, cid):
    cases, run = cc.KINDS[kind]
    return run(cc.case_by_id(cases, cid), ref.F32(), chained=cid in cc.CHAINED[kind])


@pytest.fixture(scope='module', autouse=True)
def _error_table():
    yield
    out = os.environ.get('CBHG_TAIL_ERRORS_OUT')
    if out and STATS:
        with open(out, 'w') as f:
            f.write('# tests/test_gpu_cbhg_tail.py: per kernel, worst tensor rel-L2 and worst row against fp64 over the case table, and the\n'
                    '# same two figures of the fp32 torch restatement (tests/cbhg_tail_ref.py F32); bars: tests/stage_bars.py CBHG_TAIL_BARS\n')
            f.write('%-12s %12s %12s %14s %12s\n' % ('kernel', 'tensor', 'row', 'fp32 tensor', 'fp32 row'))
            for k in cc.KERNELS:
                if k in STATS:
                    f.write('%-12s %12.3e %12.3e %14.3e %12.3e\n' % ((k,) + tuple(STATS[k])))


def _run(lib, kind, c, side_stream=False):
    run = cc.KINDS[kind][1]
    rep = run(c, Hip(lib, side_stream), chained=c.id in cc.CHAINED[kind])
    base = _f32_report(kind, c.id)
    for k in cc.KERNELS:        # the figures first, then the assertion
        (rel, row), (brel, brow) = rep.worst(k), base.worst(k)
        if rel or row:
            print('  %-22s %-12s tensor %.3e  row %.3e   (fp32 restatement: %.3e  %.3e)' % (c.id, k, rel, row, brel, brow))
            s = STATS.setdefault(k, [0.0, 0.0, 0.0, 0.0])
            s[:] = [max(s[0], rel), max(s[1], row), max(s[2], brel), max(s[3], brow)]
    for site, idx, margin in rep.flips:
        print('  %-22s flip at %s%s, fp64 margin %.3e' % (c.id, site, idx, margin))
    assert not rep.fails, '\n'.join(rep.fails[:20])


@pytest.mark.parametrize('c', cc.GRU_CASES, ids=[c.id for c in cc.GRU_CASES])
def test_bigru_recurrences(built_lib, c):
    """bigru_fwd_kernel through taco_debug_bigru_rec_fwd, bigru_bwd_kernel through taco_debug_bigru_bwd: every chunk count of
    the 8-step DMA pipeline, both sides of 2 B <= 128, h0 / dh0 present and absent, saturated gates, and the impulse cases that
    pin time order and batch indexing with exact zeros"""
    _run(built_lib, 'gru', c)


@pytest.mark.parametrize('c', cc.HW_CASES, ids=[c.id for c in cc.HW_CASES])
def test_highway_stacks(built_lib, c):
    """highway_stack_fwd_kernel / _bwd_kernel, plain (1..4 layers) and adapter form: partial and full 32-row tiles, tiles that
    straddle two sequences, gate biases of +-30"""
    _run(built_lib, 'highway', c)


@pytest.mark.parametrize('c', cc.PN_CASES, ids=[c.id for c in cc.PN_CASES])
def test_prenet(built_lib, c):
    """mlp2_kernel forward and backward, with and without the keep masks"""
    _run(built_lib, 'prenet', c)


@pytest.mark.parametrize('kind', sorted(cc.STREAMED))
def test_on_a_side_stream(built_lib, kind):
    """one case per door enqueued on a non-default stream: same bars, same arena checks"""
    _run(built_lib, kind, cc.case_by_id(cc.KINDS[kind][0], cc.STREAMED[kind]), side_stream=True)


def test_bad_calls_enqueue_nothing(built_lib):
    """null, size and overlap checks of the six doors at the C ABI: TACO_EINVAL with the argument's name, outputs untouched"""
    import ctypes as C
    lib, P = built_lib, built_lib.ptr
    L = built_lib._lib
    B, T, M = 2, 3, 6
    z = lambda *s: torch.zeros(*s, device='cuda')
    G = Guarded({n: (s, torch.float32, 'qnan') for n, s in (('a768', (M, 768)), ('a256', (M, 256)), ('b256', (M, 256)), ('a128', (M, H)),
                                                            ('b128', (M, H)), ('dh0', (2 * B, H)))})
    xg, out, wg, wc, h0 = z(M, 768), z(M, 256), z(256, 256), z(256, H), z(B, H)
    wghT, wchT = z(256, H), z(H, H)
    tab = lambda *ts: (C.c_void_p * 4)(*[None if t is None else t.data_ptr() for t in ts])
    w4, b4 = [z(H, H) for _ in range(4)], [z(H) for _ in range(4)]
    wT4 = [z(256, H) for _ in range(4)]
    y4, th4 = [z(M, H) for _ in range(4)], [z(M, 256) for _ in range(4)]
    x256, w1, w2, k1 = z(M, 256), z(256, 256), z(256, H), torch.ones(M, 256, dtype=torch.uint8, device='cuda')
    S = None    # (the default stream: nothing is enqueued)
    calls = [
        (L.taco_debug_bigru_rec_fwd, (None, P(wg), P(wc), P(wg), P(wc), None, P(G['a256']), None, B, T, S), 'xg is null'),
        (L.taco_debug_bigru_rec_fwd, (P(xg), P(wg), P(wc), P(wg), None, None, P(G['a256']), None, B, T, S), 'wc_bw is null'),
        (L.taco_debug_bigru_rec_fwd, (P(xg), P(wg), P(wc), P(wg), P(wc), None, None, P(G['a768']), B, T, S), 'out is null'),
        (L.taco_debug_bigru_rec_fwd, (P(xg), P(wg), P(wc), P(wg), P(wc), None, P(G['a256']), P(G['a768']), 0, T, S), 'B = 0'),
        (L.taco_debug_bigru_rec_fwd, (P(xg), P(wg), P(wc), P(wg), P(wc), None, P(G['a256']), P(G['a768']), B, -1, S), 'T = -1'),
        (L.taco_debug_bigru_rec_fwd, (P(G['a768']), P(wg), P(wc), P(wg), P(wc), None, P(G['a256']), P(G['a768']), B, T, S), 'ruc may not overlap xg'),
        (L.taco_debug_bigru_rec_fwd, (P(xg), P(wg), P(wc), P(wg), P(wc), None, P(G['a256']), C.c_void_p(G['a256'].data_ptr() + 4 * (M * 256 - 1)), B, T, S),
         'out may not overlap ruc'),
        (L.taco_debug_bigru_bwd, (P(out), P(out), None, P(wghT), P(wchT), P(wghT), P(wchT), None, P(G['a768']), P(G['a256']), None, B, T, S), 'ruc is null'),
        (L.taco_debug_bigru_bwd, (P(out), P(out), P(xg), P(wghT), P(wchT), P(wghT), P(wchT), None, P(G['a768']), None, None, B, T, S), 'rh is null'),
        (L.taco_debug_bigru_bwd, (P(out), P(out), P(xg), P(wghT), P(wchT), P(wghT), P(wchT), P(G['dh0']), P(G['a768']), P(G['a256']), P(G['dh0']), B, T, S),
         'dh0 may not overlap h0'),
        (L.taco_debug_bigru_bwd, (P(out), P(G['a256']), P(xg), P(wghT), P(wchT), P(wghT), P(wchT), None, P(G['a768']), P(G['a256']), None, B, T, S),
         'rh may not overlap out'),
        (L.taco_debug_bigru_bwd, (P(out), P(out), P(xg), P(wghT), P(wchT), P(wghT), P(wchT), None, P(G['a768']), P(G['a256']), None, B, 1 << 30, S), 'B \\* T <= 2\\^24'),
        (L.taco_debug_highway_stack_fwd, (P(y4[0]), tab(*w4), tab(*b4), tab(*w4), tab(*b4), None, tab(G['a128'], G['b128'], y4[2], y4[3]), None, None, None, M, 5, 0, S),
         'nl must be in \\[1, 4\\], got 5'),
        (L.taco_debug_highway_stack_fwd, (P(y4[0]), tab(*w4), tab(*b4), tab(*w4), tab(*b4), None, tab(G['a128'], None, y4[2], y4[3]), None, None, None, M, 2, 0, S),
         'y\\[1\\] is null'),
        (L.taco_debug_highway_stack_fwd, (P(y4[0]), tab(*w4), None, tab(*w4), tab(*b4), None, tab(G['a128'], G['b128'], y4[2], y4[3]), None, None, None, M, 2, 0, S),
         'null pointer table'),
        (L.taco_debug_highway_stack_fwd, (P(y4[0]), tab(*w4), tab(*b4), tab(*w4), tab(*b4), None, tab(G['a128'], G['a128'], y4[2], y4[3]), None, None, None, M, 2, 0, S),
         'y\\[0\\] may not overlap y\\[1\\]'),
        (L.taco_debug_highway_stack_fwd, (P(y4[0]), tab(*w4), tab(*b4), tab(*w4), tab(*b4), None, tab(*y4), tab(*w4), tab(*b4), tab(*th4), M, 4, 4, S),
         'T must be positive and divide M'),
        (L.taco_debug_highway_stack_fwd, (P(y4[0]), tab(*w4), tab(*b4), tab(*w4), tab(*b4), None, tab(*y4), tab(*w4), tab(*b4), tab(*th4), M, 3, 3, S),
         'the adapter form has nl == 4'),
        (L.taco_debug_highway_stack_bwd, (None, tab(*wT4), tab(*th4), tab(*y4), tab(G['a256'], G['b256'], None, None), P(G['a128']), None, None, M, 2, S), 'g is null'),
        (L.taco_debug_highway_stack_bwd, (P(y4[0]), tab(*wT4), tab(*th4), tab(*y4), tab(G['a256'], G['b256'], None, None), P(y4[0]), None, None, M, 2, S),
         'gout may not overlap g'),
        (L.taco_debug_highway_stack_bwd, (P(y4[3]), tab(*wT4), tab(*th4), tab(*y4), tab(G['a256'], th4[0], None, None), P(G['a128']), None, None, M, 2, S),
         'dth\\[1\\] may not overlap th\\[0\\]'),
        (L.taco_debug_highway_stack_bwd, (P(y4[3]), tab(*wT4), tab(*th4), tab(*y4), tab(G['a256'], G['b256'], None, None), P(G['a128']), tab(*w4), None, M, 2, S),
         'the adapter form needs the dhx table'),
        (L.taco_debug_highway_stack_bwd, (P(y4[3]), tab(*wT4), tab(*th4), tab(*y4), tab(G['a256'], G['b256'], None, None), P(G['a128']), None, None, 0, 2, S), 'M must be in'),
        (L.taco_debug_prenet_fwd, (P(x256), P(w1), None, None, None, None, None, P(G['a256']), P(G['a128']), M, S), 'w2 is null'),
        (L.taco_debug_prenet_fwd, (P(x256), P(w1), None, P(w2), None, None, None, P(G['a256']), None, M, S), 'y2 is null'),
        (L.taco_debug_prenet_fwd, (P(G['a256']), P(w1), None, P(w2), None, None, None, P(G['a256']), P(G['a128']), M, S), 'y1 may not overlap x'),
        (L.taco_debug_prenet_fwd, (P(x256), P(w1), None, P(w2), None, C.c_void_p(G['a256'].data_ptr()), None, P(G['a256']), P(G['a128']), M, S), 'y1 may not overlap keep1'),
        (L.taco_debug_prenet_fwd, (P(x256), P(w1), None, P(w2), None, None, None, P(G['a256']), P(G['a128']), (1 << 22) + 1, S), 'M must be in'),
        (L.taco_debug_prenet_bwd, (P(y4[0]), P(w2), P(w1), P(k1), None, None, P(y4[1]), P(G['a128']), P(G['a256']), P(G['b256']), M, S), 'y1_in is null'),
        (L.taco_debug_prenet_bwd, (P(y4[0]), P(w2), P(w1), P(k1), None, P(x256), P(y4[1]), P(G['a128']), P(G['a256']), P(G['a256']), M, S), 'dz1 may not overlap dx'),
        (L.taco_debug_prenet_bwd, (P(G['a128']), P(w2), P(w1), P(k1), None, P(x256), P(y4[1]), P(G['a128']), P(G['a256']), P(G['b256']), M, S), 'dz2 may not overlap dy2'),
    ]
    import re
    for fn, args, msg in calls:
        rc = fn(*args)
        assert rc == -1, (fn.__name__, msg, rc)          # TACO_EINVAL
        assert re.search(msg, lib.last_error()) and lib.last_error().startswith(fn.__name__ + ':'), (msg, lib.last_error())
    torch.cuda.synchronize()
    G.check()
    for n in G.specs:
        assert bool(torch.isnan(G[n]).all()), n          # still the fill: no call wrote anything
