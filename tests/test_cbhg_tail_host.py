"""Host (no GPU): the references, the case table and the judges of the op-level CBHG-tail tests (tests/cbhg_tail_ref.py,
tests/cbhg_tail_cases.py).  The restated fp64 references are held against the oracle's composed functions; the fp32 restatement
stands in for the kernels and must meet every bar, every exact-zero check and the flip condition in every case; each seeded
defect put into the stand-in must be caught; the case table must reach every edge the tests were written for; and the wrappers of
the debug doors refuse bad arguments by name before the library is called."""
import numpy as np
import pytest
import torch

from oracle import taco_torch as ot
from tests import cbhg_tail_cases as cc
from tests import cbhg_tail_ref as ref
from tests import stage_bars as sb

H = 128


def _run_all(be, kinds=('gru', 'highway', 'prenet')):
    out = []
    for kind in kinds:
        cases, run = cc.KINDS[kind]
        out += [run(c, be, chained=c.id in cc.CHAINED[kind]) for c in cases]
    return out


@pytest.mark.parametrize('with_h0', (False, True))
def test_gru_reference_is_the_oracles_bigru(with_h0):
    """xg = x Wg[:128] + bg, x Wc[:128] + bc fed to the recurrence alone gives _bigru's output, and dxg pulled back through the
    x-side projection gives its input gradient"""
    rng = np.random.default_rng(11 + with_h0)
    B, T = 3, 11
    p = {}
    for d in ref.DIRS:
        p['g/%s/gates/kernel' % d] = torch.tensor(rng.uniform(-0.15, 0.15, (256, 256)))
        p['g/%s/gates/bias' % d] = torch.tensor(1 + rng.uniform(-0.3, 0.3, 256))
        p['g/%s/candidate/kernel' % d] = torch.tensor(rng.uniform(-0.15, 0.15, (256, 128)))
        p['g/%s/candidate/bias' % d] = torch.tensor(rng.uniform(-0.3, 0.3, 128))
    x = torch.tensor(rng.standard_normal((B, T, H)), requires_grad=True)
    h0 = torch.tensor(rng.uniform(-0.9, 0.9, (B, H)), requires_grad=True) if with_h0 else None
    dout = rng.standard_normal((B, T, 256))
    want = ot._bigru(x, p, 'g/', h0)
    (want * torch.tensor(dout)).sum().backward()
    xg = torch.cat([torch.cat([x.detach() @ p['g/%s/gates/kernel' % d][:H] + p['g/%s/gates/bias' % d],
                               x.detach() @ p['g/%s/candidate/kernel' % d][:H] + p['g/%s/candidate/bias' % d]], 2) for d in ref.DIRS], 2)
    w = {k[2:]: v.numpy() for k, v in p.items() if k.endswith('kernel')}
    got = ref.bigru_oracle(xg.numpy(), w, None if h0 is None else h0.detach().numpy(), dout)
    assert np.abs(got['out'] - want.detach().numpy()).max() < 1e-13
    wx = torch.cat([torch.cat([p['g/%s/gates/kernel' % d][:H], p['g/%s/candidate/kernel' % d][:H]], 1) for d in ref.DIRS], 1)   # (128, 768)
    assert np.abs(got['dxg'] @ wx.numpy().T - x.grad.numpy()).max() < 1e-12
    if with_h0:
        assert np.abs(got['dh0'].sum(0) - h0.grad.numpy()).max() < 1e-12


def test_highway_reference_is_the_oracles_adapter_form():
    """_highway on concat([h, tile(speaker vector)]) with the (256, 128) adapter kernel against x_l = h_l Wa[:128] + rowb[m // T] with
    rowb = sv Wa[128:] + ba"""
    rng = np.random.default_rng(5)
    B, T = 3, 7
    M = B * T
    wa = rng.standard_normal((4, 256, H)) / 16.0
    ba = rng.uniform(-0.3, 0.3, (4, H))
    sv = np.maximum(rng.standard_normal((4, B, H)), 0)
    c = cc.HwCase('x', M, 4, B, T, 'typical')
    o = cc.hw_operands(c)
    p = dict(o['p'], wa=[wa[l, :H] for l in range(4)], rowb=[sv[l] @ wa[l, H:] + ba[l] for l in range(4)])
    got = ref.highway_oracle(o['x'], p, 4, T, o['g'])
    h = torch.tensor(o['x'], dtype=torch.float64, requires_grad=True).reshape(B, T, H)
    x0 = h
    for l in range(4):
        pre = 'hw%d/' % l
        P = {pre + 'adapt/kernel': torch.tensor(wa[l]), pre + 'adapt/bias': torch.tensor(ba[l]),
             pre + 'T/kernel': torch.tensor(p['wt'][l], dtype=torch.float64), pre + 'T/bias': torch.tensor(p['bt'][l], dtype=torch.float64),
             pre + 'H/kernel': torch.tensor(p['wh'][l], dtype=torch.float64), pre + 'H/bias': torch.tensor(p['bh'][l], dtype=torch.float64)}
        h = ot._highway(torch.cat([h, torch.tensor(sv[l])[:, None, :].expand(-1, T, -1)], 2), P, pre)
        assert np.abs(got['y'][l] - h.detach().numpy().reshape(M, H)).max() < 1e-12, l
    x0.retain_grad()
    (h.reshape(M, H) * torch.tensor(o['g'], dtype=torch.float64)).sum().backward()
    assert np.abs(got['gout'] - x0.grad.numpy().reshape(M, H)).max() < 1e-12


def test_the_fp32_restatement_meets_every_bar_without_a_flip():
    reps = _run_all(ref.F32())
    bad = [f for r in reps for f in r.fails]
    assert not bad, '\n'.join(bad[:20])
    assert not [r.id for r in reps if r.flips], 'choose seeds at which the fp32 restatement takes every ReLU decision as fp64 does'
    for k in cc.KERNELS:
        rel, row = max(r.worst(k)[0] for r in reps), max(r.worst(k)[1] for r in reps)
        print('  fp32 restatement %-12s worst tensor %.3e  worst row %.3e' % (k, rel, row))
        assert 0 < rel < 2e-6 and 0 < row < 2e-6, k       # plain fp32: a few units in the last place of sums of 128 - 256 terms


@pytest.mark.parametrize('defect,kind', [('chunk_hprev', 'gru'), ('bw_row_reversed', 'gru'), ('h0_ignored', 'gru'), ('tile_last_row', 'highway'),
                                         ('tile_last_row', 'prenet'), ('rowb_tile_first', 'highway'), ('relu_factor', 'highway'),
                                         ('keep_ignored', 'prenet')])
def test_a_seeded_defect_is_caught(defect, kind):
    caught = [r.id for r in _run_all(ref.F32(defect), (kind,)) if r.fails]
    print('  %s: caught in %s' % (defect, caught))
    assert caught
    expect = {'chunk_hprev': lambda c: c.T > 8, 'bw_row_reversed': lambda c: c.T > 1, 'h0_ignored': lambda c: c.h0,
              'tile_last_row': lambda c: c.M % 32 != 0, 'rowb_tile_first': lambda c: c.id == 'adapter-B7-T5',
              'relu_factor': lambda c: True, 'keep_ignored': lambda c: c.masks}[defect]
    assert set(caught) == {c.id for c in cc.KINDS[kind][0] if expect(c)}, 'caught where the defect cannot show, or missed where it must'


def test_the_case_table_reaches_every_edge():
    for name, reached in cc.EDGES.items():
        assert reached(), name
    ids = [c.id for cases, _ in cc.KINDS.values() for c in cases]
    assert len(ids) == len(set(ids)) == 38 + 13 + 10
    assert all(c.M == c.B * c.T for c in cc.HW_CASES if c.B is not None)
    b0, t0 = cc.IMPULSE_AT
    assert all(0 < b0 < c.B - 1 and t0 == c.T - 1 - t0 == 8 for c in cc.GRU_CASES if c.regime.startswith('impulse'))


def test_bars_stay_under_the_projects_ceilings():
    assert set(sb.CBHG_TAIL_BARS) == set(cc.KERNELS)
    for k, (tensor, row) in sb.CBHG_TAIL_BARS.items():
        top = (sb.FWD_TENSOR_BAR, sb.FWD_ROW_BAR) if k.endswith('fwd') else (sb.TENSOR_BAR, sb.ROW_BAR)
        assert 0 < tensor <= top[0] and 0 < row <= top[1], k


def test_saturated_operands_are_what_the_case_says():
    c = cc.case_by_id(cc.GRU_CASES, 'sat-B5-T41-h0')
    want = cc.gru_reference(c)
    ruc = want['ruc'].astype(np.float32).reshape(c.B, c.T, 2, 3, H)
    unit = np.arange(H) % 3 == 0
    assert (((ruc[..., :2, :] == 0) | (ruc[..., :2, :] == 1))[..., unit].mean() > 0.5) and (np.abs(ruc[..., 2, unit]) == 1).all()
    assert np.abs(cc.gru_operands(c)['xg']).max() > 128          # exp2 of 1.44 * that overflows fp32
    c = cc.case_by_id(cc.HW_CASES, 'plain-M33-gates30')
    t = np.concatenate([s[:, :H] for s in cc.hw_reference(c)['th']]).astype(np.float32)
    assert ((t == 1) | (t < 2.0 ** -20)).all() and (t == 1).any() and (t < 2.0 ** -20).any() and (t > 0).all()


def _gru_args(B=2, T=3):
    z = torch.zeros
    w = {'%s/%s/kernel' % (d, k): z(256, n) for d in ref.DIRS for k, n in (('gates', 256), ('candidate', 128))}
    wT = {'%s/%s' % (d, k): z(n, H) for d in ref.DIRS for k, n in (('wghT', 256), ('wchT', 128))}
    return dict(xg=z(B, T, 768), w=w, out=z(B, T, 256), ruc=z(B, T, 768), h0=z(B, H)), dict(
        dout=z(B, T, 256), out=z(B, T, 256), ruc=z(B, T, 768), wT=wT, dxg=z(B, T, 768), rh=z(B, T, 256), h0=z(B, H), dh0=z(2, B, H))


def test_the_wrappers_refuse_bad_arguments_by_name(built_lib):
    """every check runs on tensors of any device and the device check comes last: CPU tensors reach it only when all else is right"""
    lib, z = built_lib, torch.zeros
    f, b = _gru_args()
    with pytest.raises(ValueError, match=r'^debug_bigru_rec_fwd: xg must be on the GPU'):
        lib.debug_bigru_rec_fwd(**f)
    with pytest.raises(ValueError, match=r'^debug_bigru_bwd: dout must be on the GPU'):
        lib.debug_bigru_bwd(**b)
    for fn, args, change, msg in (
            (lib.debug_bigru_rec_fwd, f, dict(h0=z(3, H)), r'h0 must be a contiguous float32 tensor of shape \(2, 128\)'),
            (lib.debug_bigru_rec_fwd, f, dict(out=None), r'out must be'),
            (lib.debug_bigru_rec_fwd, f, dict(xg=z(2, 3, 767)), r'xg must be'),
            (lib.debug_bigru_rec_fwd, f, dict(ruc=f['xg']), r'ruc may not overlap xg'),
            (lib.debug_bigru_rec_fwd, f, dict(w=dict(f['w'], **{'bw/candidate/kernel': z(256, 256)})), r"w\['bw/candidate/kernel'\] must be"),
            (lib.debug_bigru_bwd, b, dict(dh0=z(2, H)), r'dh0 must be .* shape \(2, 2, 128\)'),
            (lib.debug_bigru_bwd, b, dict(rh=b['out']), r'rh may not overlap out'),
            (lib.debug_bigru_bwd, b, dict(ruc=z(2, 3, 768).double()), r'ruc must be'),
            (lib.debug_bigru_bwd, b, dict(dxg=b['dxg'][:, :, ::1].transpose(0, 1)), r'dxg must be')):
        with pytest.raises(ValueError, match='^%s: %s' % (fn.__name__, msg)):
            fn(**dict(args, **change))
    M = 5
    L = lambda *s: [z(*s) for _ in range(4)]
    hf = dict(x=z(M, H), wt=L(H, H), bt=L(H), wh=L(H, H), bh=L(H), y=L(M, H), th=L(M, 256))
    hb = dict(g=z(M, H), wT=L(256, H), th=L(M, 256), x=L(M, H), dth=L(M, 256), gout=z(M, H))
    with pytest.raises(ValueError, match=r'^debug_highway_stack_fwd: x must be on the GPU'):
        lib.debug_highway_stack_fwd(**hf)
    with pytest.raises(ValueError, match=r'^debug_highway_stack_bwd: g must be on the GPU'):
        lib.debug_highway_stack_bwd(**hb)
    for fn, args, change, msg in (
            (lib.debug_highway_stack_fwd, hf, dict(y=[]), r'nl \(the length of y\) must be an integer in \[1, 4\]'),
            (lib.debug_highway_stack_fwd, hf, dict(wt=L(H, H)[:3]), r'wt must be a list of 4 tensors'),
            (lib.debug_highway_stack_fwd, hf, dict(bh=L(H)[:3] + [z(H + 1)]), r'bh\[3\] must be'),
            (lib.debug_highway_stack_fwd, hf, dict(th=hf['y'][:3] + [z(M, 256)]), r'th\[0\] must be'),
            (lib.debug_highway_stack_fwd, hf, dict(y=[hf['x']] + L(M, H)[:3]), r'y\[0\] may not overlap x'),
            (lib.debug_highway_stack_fwd, hf, dict(wa=L(H, H), rowb=L(1, H), hx=L(M, H), T=2), r'T must divide M'),
            (lib.debug_highway_stack_fwd, hf, dict(wa=L(H, H), rowb=L(2, H), hx=L(M, H), T=5), r'rowb\[0\] must be .* shape \(1, 128\)'),
            (lib.debug_highway_stack_fwd, dict(hf, **{k: hf[k][:2] for k in ('wt', 'bt', 'wh', 'bh', 'y', 'th')}),
             dict(wa=L(H, H), rowb=L(1, H), hx=L(M, H), T=5), r'the adapter form has 4 layers, got nl = 2'),
            (lib.debug_highway_stack_fwd, hf, dict(hx=L(M, H)), r'rowb and hx belong to the adapter form'),
            (lib.debug_highway_stack_bwd, hb, dict(gout=hb['g']), r'gout may not overlap g'),
            (lib.debug_highway_stack_bwd, hb, dict(dth=hb['dth'][:3] + hb['dth'][:1]), r'dth\[0\] may not overlap dth\[3\]'),
            (lib.debug_highway_stack_bwd, hb, dict(wT=L(H, 256)), r'wT\[0\] must be'),
            (lib.debug_highway_stack_bwd, hb, dict(waT=L(H, H)), r'dhx must be a list of 4 tensors'),
            (lib.debug_highway_stack_bwd, hb, dict(dhx=L(M, H)), r'dhx belongs to the adapter form')):
        with pytest.raises(ValueError, match='^%s: %s' % (fn.__name__, msg)):
            fn(**dict(args, **change))
    k = lambda n: torch.ones(M, n, dtype=torch.uint8)
    pf = dict(x=z(M, 256), w1=z(256, 256), b1=z(256), w2=z(256, H), b2=z(H), y1=z(M, 256), y2=z(M, H), keep1=k(256), keep2=k(H))
    pb = dict(dy2=z(M, H), w2T=z(H, 256), w1T=z(256, 256), y1_in=z(M, 256), y2_in=z(M, H), dz2=z(M, H), dz1=z(M, 256), dx=z(M, 256),
              keep1=k(256), keep2=k(H))
    with pytest.raises(ValueError, match=r'^debug_prenet_fwd: x must be on the GPU'):
        lib.debug_prenet_fwd(**pf)
    with pytest.raises(ValueError, match=r'^debug_prenet_bwd: dy2 must be on the GPU'):
        lib.debug_prenet_bwd(**pb)
    for fn, args, change, msg in (
            (lib.debug_prenet_fwd, pf, dict(keep1=z(M, 256)), r'keep1 must be a contiguous uint8 tensor'),
            (lib.debug_prenet_fwd, pf, dict(w2=None), r'w2 must be'),
            (lib.debug_prenet_fwd, pf, dict(y1=pf['x']), r'y1 may not overlap x'),
            (lib.debug_prenet_fwd, pf, dict(y2=z(M + 1, H)), r'y2 must be'),
            (lib.debug_prenet_bwd, pb, dict(y1_in=None), r'y1_in must be'),
            (lib.debug_prenet_bwd, pb, dict(keep2=k(256)), r'keep2 must be'),
            (lib.debug_prenet_bwd, pb, dict(dx=pb['dz1']), r'dz1 may not overlap dx'),
            (lib.debug_prenet_bwd, pb, dict(dz2=pb['dy2']), r'dz2 may not overlap dy2')):
        with pytest.raises(ValueError, match='^%s: %s' % (fn.__name__, msg)):
            fn(**dict(args, **change))
    pf.pop('b1')
    with pytest.raises(ValueError, match=r'^debug_prenet_fwd: x must be on the GPU'):     # (a bias may be None)
        lib.debug_prenet_fwd(b1=None, **pf)
