"""GPU: the train step's glue kernels of tacotron_amd/csrc/elementwise.hip -- the embedding gather and scatter, the highway blend and
its backward, the activation and BN-affine derivatives, the column sums, mask_rows, center_rows, mask_pos, zero_tail_rows, add, the
L1 loss with its sign gradient, the batched weight transpose, the sum of squares and clip + Adam -- through the taco_debug_* doors
(include/taco_hip.h), against the fp64 references and the derived bounds of tests/glue_ops.py.  The case lists and the proofs that
they reach every branch of the launch geometry live there and in tests/test_glue_ops_host.py.

Every output and scratch buffer is carved from a guarded arena (tests/poison.Guarded): outputs start as NaN, or as known prior content
where the call accumulates or works in place; the guard bands are checked after every call.  Copies, masks, signs and exact-zero
sites are compared bitwise; everything else per element against its bound, no element left out.  The worst |err| / bound per op is
printed and, when GLUE_OPS_ERRORS_OUT names a file, written there (profiles/glue_ops_errors.txt is such a file).
Measured: 188 tests, 3.8 s on one MI355X; every ratio below 0.79, no kernel bug found."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import glue_ops as go
from tests.poison import Guarded

pytestmark = pytest.mark.gpu
F32, f32 = np.float32, torch.float32

STATS = {}      # op -> [comparisons, worst |err| / bound] ('exact' ops: bitwise, ratio 0)


def write_error_table():
    out = os.environ.get('GLUE_OPS_ERRORS_OUT')
    lines = ['%-24s %6d %12.3e\n' % (k, STATS[k][0], STATS[k][1]) for k in sorted(STATS)]
    print()
    for ln in lines:
        print('  ' + ln, end='')
    if out and STATS:
        with open(out, 'w') as f:
            f.write('# tests/test_gpu_glue_ops.py: per op and output, comparisons made and the worst |got - ref| / derived bound (bar 1;\n'
                    '# tests/glue_ops.py); 0 = compared bitwise\n')
            f.write('%-24s %6s %12s\n' % ('op.output', 'cases', 'worst-ratio'))
            f.writelines(lines)


@pytest.fixture(scope='module', autouse=True)
def _error_table():
    yield
    write_error_table()


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def _note(op, ratio):
    s = STATS.setdefault(op, [0, 0.0])
    s[0] += 1
    s[1] = max(s[1], float(ratio))


def judge(op, what, got, ref, bound):
    """every element: |got - ref| <= bound (a zero bound asks for the exact value); prints the figure before it asserts"""
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.broadcast_to(np.asarray(bound, np.float64), np.shape(ref))
    assert got.shape == ref.shape, (op, what, got.shape, ref.shape)
    err = np.abs(got - ref)
    bad = ~(err <= bound)                       # (a NaN fails)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    worst = float(np.nanmax(ratio)) if ratio.size else 0.0
    print('  %-22s %-44s worst |err| / bound %.3e' % (op, what, worst))
    _note(op, worst if not bad.any() else np.inf)
    assert not bad.any(), '%s %s: %d of %d elements outside their bound, first at %s: got %r, ref %r, bound %.3e' % (
        op, what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), got[tuple(np.argwhere(bad)[0])], ref[tuple(np.argwhere(bad)[0])],
        bound[tuple(np.argwhere(bad)[0])])


def exact(op, what, got, ref):
    """bit for bit (NaN payloads and the sign of zero included)"""
    g, r = go.bits(got), go.bits(ref)
    assert g.shape == r.shape, (op, what, g.shape, r.shape)
    bad = g != r
    _note(op, np.inf if bad.any() else 0.0)
    assert not bad.any(), '%s %s: %d of %d elements differ bitwise, first at %s: got %r, ref %r' % (
        op, what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), np.asarray(got, F32)[tuple(np.argwhere(bad)[0])],
        np.asarray(ref, F32)[tuple(np.argwhere(bad)[0])])


def zeros_exact(op, what, got, zero):
    """the sites that must be exactly +0.0"""
    exact(op, what + ' zero sites', np.asarray(got, F32)[zero], np.zeros(int(zero.sum()), F32))


def put(G, name, a):
    G[name].view(-1).copy_(dev(np.asarray(a).reshape(-1)))
    return G[name].view(-1)


# ------------------------------------------------------------------------------------------------------------------
# embedding gather and scatter

@pytest.mark.parametrize('c', go.EMB_CASES, ids=[c.id for c in go.EMB_CASES])
def test_embedding_gather_and_scatter(built_lib, c, monkeypatch):
    monkeypatch.setenv('TACO_DETERMINISTIC', '1' if c.det else '0')
    rng = go.rng_of(c.id + '-data')
    ids = go.emb_ids(c)
    table = rng.standard_normal((c.V, c.width)).astype(F32)
    dout = rng.standard_normal((c.rows, c.width)).astype(F32)
    G = Guarded({'out': ((c.rows, c.width), f32, 'qnan'), 'dtable': ((c.V, c.width), f32, 0.0)})
    ids_t, dout_t = dev(ids), dev(dout.reshape(-1))
    built_lib.debug_embedding(dev(table.reshape(-1)), ids_t, G['out'].view(-1), c.rows, c.V, c.width)
    G.check('out')
    exact('embedding', c.id, host(G['out']), go.embedding_ref(table, ids))
    geo = go.emb_geometry(c.rows, c.det)
    ref, tot, n, S = go.embedding_bwd_ref(dout, ids, table, geo)
    runs = []
    for _ in range(2 if c.det else 1):
        put(G, 'dtable', table)                                         # the table row holds a prior value: the scatter adds to it
        built_lib.debug_embedding_bwd(dout_t, ids_t, G['dtable'].view(-1), c.rows, c.V, c.width)
        G.check()
        runs.append(host(G['dtable']).copy())
    got = runs[0]
    judge('embedding_bwd', c.id, got, ref, go.sum_bound(n, S, go.C_EMB, prior=table.astype(np.float64), total=ref, adds=geo['segs']))
    idle = (n[:, 0] == 0)
    exact('embedding_bwd', c.id + ' rows no id names', got[idle], table[idle])
    assert c.pattern == 'one' or c.V == 1 or idle[go.EMB_NEVER(c.V)]
    if c.det:
        exact('embedding_bwd', c.id + ' second deterministic run', runs[1], runs[0])


# ------------------------------------------------------------------------------------------------------------------
# highway blend

@pytest.mark.parametrize('M', go.HIGHWAY_M)
def test_highway_combine_and_backward(built_lib, M):
    th, x, dy = go.highway_operands(M)
    G = Guarded({'y': ((M, 128), f32, 'qnan'), 'dth': ((M, 256), f32, 'qnan'), 'dx': ((M, 128), f32, 'qnan')})
    th_t, x_t = dev(th.reshape(-1)), dev(x.reshape(-1))
    built_lib.debug_highway_combine(th_t, x_t, G['y'].view(-1), M)
    G.check('y')
    ref, S = go.highway_ref(th, x)
    judge('highway_combine', 'M=%d' % M, host(G['y']), ref, go.ew_bound(go.K_HW_Y, S))
    built_lib.debug_highway_combine_bwd(th_t, x_t, dev(dy.reshape(-1)), G['dth'].view(-1), G['dx'].view(-1), M)
    G.check('dth', 'dx')
    r = go.highway_bwd_ref(th, x, dy)
    dth = host(G['dth'])
    judge('highway_combine_bwd.dT', 'M=%d' % M, dth[:, :128], r['dt'], go.ew_bound(go.K_HW_DT, r['S_dt']))
    judge('highway_combine_bwd.dH', 'M=%d' % M, dth[:, 128:], r['dh'], go.ew_bound(go.K_HW_DH, r['S_dh']))
    zeros_exact('highway_combine_bwd.dH', 'M=%d' % M, dth[:, 128:], r['zero'])
    judge('highway_combine_bwd.dx', 'M=%d' % M, host(G['dx']), r['dx'], go.ew_bound(go.K_HW_DX, r['S_dx']))


# ------------------------------------------------------------------------------------------------------------------
# activation derivatives

@pytest.mark.parametrize('c', go.ACT_CASES, ids=[c.id for c in go.ACT_CASES])
def test_act_bwd(built_lib, c):
    y, dy, keep = go.act_operands(c)
    G = Guarded({'dz': ((c.n,), f32, 'qnan')})
    keep_t = None if keep is None else dev(keep)
    if c.inplace:                                  # dz == dy, as the model calls it
        put(G, 'dz', dy)
        built_lib.debug_act_bwd(dev(y), G['dz'], G['dz'], c.n, c.act, keep=keep_t)
        G.check()
    else:
        built_lib.debug_act_bwd(dev(y), dev(dy), G['dz'], c.n, c.act, keep=keep_t)
        G.check('dz')
    ref, S, zero = go.act_bwd_ref(y, dy, keep, c.act)
    got = host(G['dz'])
    if go.K_ACT[c.act] == 0:
        exact('act_bwd.' + c.act, c.id, got, ref.astype(F32) + F32(0))
    else:
        judge('act_bwd.' + c.act, c.id, got, ref, go.ew_bound(go.K_ACT[c.act], S))
        zeros_exact('act_bwd.' + c.act, c.id, got, zero)


@pytest.mark.parametrize('c', go.AFF_CASES, ids=[c.id for c in go.AFF_CASES])
def test_affine_act_bwd(built_lib, c, monkeypatch):
    monkeypatch.setenv('TACO_DETERMINISTIC', '1' if c.det else '0')
    pre, gamma, dy, pg, pb = go.aff_operands(c)
    G = Guarded({'dz': ((c.M, c.N), f32, 'qnan'), 'dgamma': ((c.N,), f32, 0.0), 'dbeta': ((c.N,), f32, 0.0)})
    runs = []
    for _ in range(2 if c.det else 1):
        put(G, 'dgamma', pg), put(G, 'dbeta', pb)
        built_lib.debug_affine_act_bwd(dev(pre.reshape(-1)), dev(gamma), dev(dy.reshape(-1)), G['dz'].view(-1), G['dgamma'], G['dbeta'], c.M, c.N, c.act)
        G.check('dz')
        runs.append((host(G['dgamma']).copy(), host(G['dbeta']).copy()))
    r = go.affine_act_bwd_ref(pre, gamma, dy, c.act, pg, pb)
    adds = go.col_geometry(c.M, c.det)['chunks']
    dz = host(G['dz'])
    judge('affine_act_bwd.dz', c.id, dz, r['dz'], go.ew_bound(go.K_AFF_DZ, r['S_dz']))
    zeros_exact('affine_act_bwd.dz', c.id, dz, r['zero'])
    judge('affine_act_bwd.dgamma', c.id, runs[0][0], r['dgamma'], go.sum_bound(r['n'], r['S_g'], go.C_AFF_G, prior=pg.astype(np.float64), total=r['dgamma'], adds=adds))
    judge('affine_act_bwd.dbeta', c.id, runs[0][1], r['dbeta'], go.sum_bound(r['n'], r['S_b'], go.C_TREE, prior=pb.astype(np.float64), total=r['dbeta'], adds=adds))
    if c.det:
        exact('affine_act_bwd.dgamma', c.id + ' second deterministic run', runs[1][0], runs[0][0])
        exact('affine_act_bwd.dbeta', c.id + ' second deterministic run', runs[1][1], runs[0][1])


@pytest.mark.parametrize('c', go.COLSUM_CASES, ids=[c.id for c in go.COLSUM_CASES])
def test_colsum_batched(built_lib, c):
    rng = go.rng_of(c.id)
    x = rng.standard_normal((c.B * c.T, c.ld)).astype(F32)
    x[:, c.N:] = np.nan                                  # the pitch padding is never read
    G = Guarded({'out': ((c.B, c.N), f32, 'qnan')})      # overwritten, not accumulated: the NaN must be gone
    built_lib.debug_colsum_batched(dev(x.reshape(-1)), G['out'].view(-1), c.B, c.T, c.N, ld=c.ld)
    G.check('out')
    ref, S = go.colsum_ref(x, c.B, c.T, c.N)
    judge('colsum_batched', c.id, host(G['out']), ref, go.sum_bound(c.T, S, go.C_TREE))


# ------------------------------------------------------------------------------------------------------------------
# row masks

@pytest.mark.parametrize('c', go.ROW_CASES, ids=[c.id for c in go.ROW_CASES])
def test_mask_rows_and_center_rows(built_lib, c):
    x, length = go.row_operands(c)
    B = go.ROW_B
    G = Guarded({'masked': ((B, c.T, c.C), f32, 'qnan'), 'centred': ((B, c.T, c.C), f32, 'qnan')})
    x_t, len_t = dev(x.reshape(-1)), dev(length)
    built_lib.debug_mask_rows(x_t, len_t, G['masked'].view(-1), B, c.T, c.C)
    built_lib.debug_center_rows(x_t, len_t, G['centred'].view(-1), B, c.T, c.C)
    G.check('masked', 'centred')
    exact('mask_rows', c.id, host(G['masked']), go.mask_rows_ref(x, length))
    ref, bound, zero = go.center_rows_ref(x, length)
    got = host(G['centred'])
    judge('center_rows', c.id, got, ref, bound)
    zeros_exact('center_rows', c.id, got, zero)


@pytest.mark.parametrize('c', go.MASK_POS_CASES, ids=[c.id for c in go.MASK_POS_CASES])
def test_mask_pos(built_lib, c):
    rng = go.rng_of(c.id)
    g = rng.standard_normal((c.rows, c.ldg)).astype(F32)
    y = go.plant_zeros(rng.standard_normal((c.rows, c.ldy)).astype(F32), rng, every=5)
    G = Guarded({'g': ((c.rows, c.ldg), f32, 0.0)})
    put(G, 'g', g)
    built_lib.debug_mask_pos(G['g'].view(-1), dev(y.reshape(-1)), c.rows, c.cols, float(c.scale), ldg=c.ldg, ldy=c.ldy)
    G.check()
    want = g.copy()                                      # the rest of every record keeps its bits
    want[:, :c.cols] = go.mask_pos_ref(g[:, :c.cols], y[:, :c.cols], c.scale)
    exact('mask_pos', c.id, host(G['g']), want)


@pytest.mark.parametrize('c', go.ZERO_TAIL_CASES, ids=[c.id for c in go.ZERO_TAIL_CASES])
def test_zero_tail_rows(built_lib, c):
    rng = go.rng_of(c.id)
    B, Td = len(go.TAIL_LEN), go.TAIL_TD
    x0 = rng.standard_normal((B, Td, c.C0)).astype(F32)
    x0[:, :, ::3] = np.nan                               # rows below the length keep their bits, NaN payloads included: nothing is read
    spec = {'x0': ((B, Td, c.C0), f32, 0.0)}
    if c.C1:
        x1 = rng.standard_normal((B, Td, c.C1)).astype(F32)
        spec['x1'] = ((B, Td, c.C1), f32, 0.0)
    G = Guarded(spec)
    put(G, 'x0', x0)
    if c.C1:
        put(G, 'x1', x1)
    built_lib.debug_zero_tail_rows(G['x0'].view(-1), c.C0, dev(go.TAIL_LEN), B, Td, x1=G['x1'].view(-1) if c.C1 else None, C1=c.C1 or 0)
    G.check()
    exact('zero_tail_rows', c.id + ' x0', host(G['x0']), go.zero_tail_ref(x0, go.TAIL_LEN))
    if c.C1:
        exact('zero_tail_rows', c.id + ' x1', host(G['x1']), go.zero_tail_ref(x1, go.TAIL_LEN))


@pytest.mark.parametrize('n', (1, 1001, (1 << 20) + 3))
def test_add(built_lib, n):
    rng = go.rng_of('add-%d' % n)
    a, b = rng.standard_normal(n).astype(F32), (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(F32)
    G = Guarded({'y': ((n,), f32, 'qnan')})
    built_lib.debug_add(dev(a), dev(b), G['y'], n)
    G.check('y')
    judge('add', 'n=%d' % n, host(G['y']), a.astype(np.float64) + b, go.ew_bound(2, np.abs(a.astype(np.float64) + b)))     # one rounded operation on its own result: k = 2


# ------------------------------------------------------------------------------------------------------------------
# L1 loss

@pytest.mark.parametrize('c', go.L1_CASES, ids=[c.id for c in go.L1_CASES])
def test_l1_loss_and_sign_gradient(built_lib, c):
    spec = {'parts': ((2 * go.LOSS_PARTS,), f32, 'qnan'), 'loss': ((3,), f32, 'qnan'), 'out': ((3,), f32, 'qnan')}
    ops, refs = [None, None], [None, None]
    for i, t in enumerate(c.terms):
        if t is None:
            continue
        M, N, ldg, with_grad = t
        a, b = go.l1_operands(c.id, i, M, N)
        ops[i] = dict(a=dev(a.reshape(-1)), b=dev(b.reshape(-1)), M=M, N=N, ldg=ldg)
        s, sign = go.l1_ref(a, b)
        refs[i] = (s, sign, go.l1_geometry(M, N, ldg if with_grad else N))
        if with_grad:
            spec['grad%d' % i] = ((M, ldg), f32, 'qnan')
    G = Guarded(spec)
    for i, t in enumerate(c.terms):
        if t is not None and t[3]:
            ops[i]['grad'] = G['grad%d' % i].view(-1)
    runs = []
    for _ in range(2):
        G.refill('parts', 'loss', 'out')                 # NaN in every partial before the call: blocks without work must write their 0
        built_lib.debug_l1_loss(ops, G['parts'], G['loss'], out=G['out'])
        G.check(*spec)
        runs.append(host(G['loss']).copy())
    exact('l1.loss', c.id + ' second run', runs[1], runs[0])
    loss, parts = runs[0], host(G['parts']).reshape(2, go.LOSS_PARTS)
    exact('l1.loss', c.id + ' out', host(G['out']), loss[[0, 1, 2]])
    b0, b1, b2 = go.l1_bounds([None if r is None else (r[0], r[2]) for r in refs])
    s = [0.0 if r is None else r[0] for r in refs]
    judge('l1.loss', c.id, loss, np.array([s[0] + s[1], s[0], s[1]]), np.array([b0, b1, b2]))
    for i, r in enumerate(refs):
        busy = 0 if r is None else r[2]['busy_blocks']
        exact('l1.parts', c.id + ' idle blocks of term %d' % i, parts[i, busy:], np.zeros(go.LOSS_PARTS - busy, F32))
        if r is None:
            continue
        judge('l1.parts', c.id + ' sum of term %d' % i, np.array(parts[i].astype(np.float64).sum()), np.array(r[0]), np.array(go.sum_bound(r[2]['lane_terms'], r[0], 1 + 6 + 16)))
        if c.terms[i][3]:
            M, N, ldg, _ = c.terms[i]
            want = np.zeros((M, ldg), F32)               # exactly 0 at a == b and in the pad columns
            want[:, :N] = r[1]
            exact('l1.grad', c.id + ' term %d' % i, host(G['grad%d' % i]), want)


# ------------------------------------------------------------------------------------------------------------------
# batched transpose

@pytest.mark.parametrize('name', list(go.TRANSPOSE_CASES), ids=list(go.TRANSPOSE_CASES))
def test_transpose_batch(built_lib, name):
    kinds = go.TRANSPOSE_CASES[name]
    rng = go.rng_of(name)
    spec, srcs, jobs = {}, [], []
    for i, j in enumerate(kinds):
        ldi, ldo = j.ldi or j.N, j.ldo or j.K
        src = rng.standard_normal((j.taps * j.K, ldi)).astype(F32)
        src[:, j.N:] = np.nan
        srcs.append(src)
        spec['dst%d' % i] = ((j.taps * j.N, ldo), f32, 'noise')
    G = Guarded(spec)
    before = [host(G['dst%d' % i]).copy() for i in range(len(kinds))]
    for i, j in enumerate(kinds):
        jobs.append(dict(src=dev(srcs[i].reshape(-1)), dst=G['dst%d' % i].view(-1), taps=j.taps, K=j.K, N=j.N, ldi=j.ldi, ldo=j.ldo))
    built_lib.debug_transpose_batch(jobs)
    G.check()
    for i, j in enumerate(kinds):
        want = before[i].copy()                          # the bytes between K and the pitch keep their (noise) content
        want[:, :j.K] = go.transpose_ref(srcs[i][:, :j.N].reshape(j.taps, j.K, j.N)).reshape(j.taps * j.N, j.K)
        exact('transpose_batch', '%s job %d' % (name, i), host(G['dst%d' % i]), want)


# ------------------------------------------------------------------------------------------------------------------
# sum of squares, clip + Adam

@pytest.mark.parametrize('n', go.SUMSQ_N)
def test_sumsq(built_lib, n):
    rng = go.rng_of('sumsq-%d' % n)
    x = rng.standard_normal(n).astype(F32)
    G = Guarded({'x': ((n,), f32, 0.0), 'parts': ((go.SUMSQ_PARTS,), f32, 'qnan')})      # (the arena's buffers are 256-byte aligned)
    put(G, 'x', x)
    runs = []
    for _ in range(2):
        G.refill('parts')
        built_lib.debug_sumsq(G['x'], n, G['parts'])
        G.check('parts')
        runs.append(host(G['parts']).copy())
    exact('sumsq', 'n=%d second run' % n, runs[1], runs[0])
    ss, rel = go.sumsq_ref(x)
    judge('sumsq', 'n=%d (%s)' % (n, ', '.join(sorted(go.sumsq_labels(n)))), np.array(runs[0].astype(np.float64).sum()), np.array(ss), np.array(rel * ss))
    first_idle = min(go.SUMSQ_PARTS, max(1, -(-(n // 4) // 256)))        # blocks without an element write their 0 (block 0 owns the tail)
    exact('sumsq', 'n=%d idle blocks' % n, runs[0][first_idle:], np.zeros(go.SUMSQ_PARTS - first_idle, F32))


def _adam_buffers(c, p, m, v):
    G = Guarded({'p': ((c.n,), f32, 0.0), 'm': ((c.n,), f32, 0.0), 'v': ((c.n,), f32, 0.0), 'scratch': ((go.SUMSQ_PARTS,), f32, 'noise'),
                 'gnorm': ((1,), f32, 'noise')})
    put(G, 'p', p), put(G, 'm', m), put(G, 'v', v)
    return G


@pytest.mark.parametrize('c', go.ADAM_CASES, ids=[c.id for c in go.ADAM_CASES])
def test_clip_adam(built_lib, c):
    p, g, m, v, cap = go.adam_operands(c)
    G = _adam_buffers(c, p, m, v)
    built_lib.clip_adam_step(G['p'], dev(g), G['m'], G['v'], go.ADAM_LR, cap, c.step, G['scratch'], G['gnorm'])
    G.check('scratch', 'gnorm')
    r = go.adam_ref(p, g, m, v, go.ADAM_LR, cap, c.step)
    judge('clip_adam.norm', c.id, host(G['gnorm']), np.array([r['gn']]), np.array([r['b_gn']]))
    judge('clip_adam.m', c.id, host(G['m']), r['m'], r['b_m'])
    judge('clip_adam.v', c.id, host(G['v']), r['v'], r['b_v'])
    judge('clip_adam.p', c.id, host(G['p']), r['p'], r['b_p'])


def test_clip_adam_guarded_skips_the_update_when_an_error_word_is_set(built_lib):
    c = go.ADAM_CASES[4]
    p, g, m, v, cap = go.adam_operands(c)
    for words in ((1, 0), (0, 7)):
        G = _adam_buffers(c, p, m, v)
        built_lib.clip_adam_step(G['p'], dev(g), G['m'], G['v'], go.ADAM_LR, cap, c.step, G['scratch'], G['gnorm'], err_words=dev(np.array(words, np.int32)))
        G.check('gnorm')
        exact('clip_adam.guarded', 'p', host(G['p']), p), exact('clip_adam.guarded', 'm', host(G['m']), m), exact('clip_adam.guarded', 'v', host(G['v']), v)
        exact('clip_adam.guarded', 'norm', host(G['gnorm']), np.array([-1.0], F32))


# ------------------------------------------------------------------------------------------------------------------
# refusals

def test_bad_arguments_return_einval_and_enqueue_nothing(built_lib):
    """real device buffers this time: after a refused call every output still holds its poison"""
    L = built_lib._lib
    G = Guarded({k: ((4096,), f32, 'qnan') for k in ('o0', 'o1', 'o2', 'parts', 'loss')})
    a = dev(np.ones(4096, F32))
    ids = dev(np.zeros(64, np.int32))
    P = lambda t: C.c_void_p(t.data_ptr())
    o0, o1, o2, parts, loss = (P(G[k]) for k in ('o0', 'o1', 'o2', 'parts', 'loss'))
    tab = lambda *p: (C.c_void_p * len(p))(*[x.value for x in p])
    ints = lambda *v: (C.c_int * len(v))(*v)
    s = built_lib.stream_ptr()
    calls = (
        lambda: L.taco_debug_embedding(P(a), P(ids), o0, 4, 3, 18, s),
        lambda: L.taco_debug_embedding_bwd(P(a), P(ids), o0, 4, 3, 1028, s),
        lambda: L.taco_debug_highway_combine(P(a), P(a), o0, 0, s),
        lambda: L.taco_debug_highway_combine_bwd(P(a), P(a), P(a), o0, o0, 2, s),
        lambda: L.taco_debug_act_bwd(P(a), P(a), None, o0, 8, 9, s),
        lambda: L.taco_debug_affine_act_bwd(P(a), P(a), P(a), o0, o1, o1, 4, 8, 1, s),
        lambda: L.taco_debug_colsum_batched(P(a), 7, o0, 2, 3, 8, s),
        lambda: L.taco_debug_mask_rows(P(a), P(ids), o0, 2, 3, 6, s),
        lambda: L.taco_debug_center_rows(P(a), None, o0, 2, 3, 8, s),
        lambda: L.taco_debug_mask_pos(o0, 8, P(a), 7, 4, 8, 2.0, s),
        lambda: L.taco_debug_zero_tail_rows(o0, 8, o0, 8, P(ids), 2, 3, s),
        lambda: L.taco_debug_add(P(a), None, o0, 8, s),
        lambda: L.taco_debug_l1_loss(P(a), P(a), o0, 3, 2, 4, None, None, None, 0, 0, 0, parts, loss, None, s),
        lambda: L.taco_debug_transpose_batch(1, tab(P(a)), tab(o0), ints(3), ints(4), ints(5), ints(8), ints(4), s),
        lambda: L.taco_debug_sumsq(P(a), 0, o0, s),
    )
    assert len({n for call in calls for n in call.__code__.co_names if n.startswith('taco_debug_')}) == 15      # one refusal per door
    for call in calls:
        assert call() == -1 and built_lib.last_error().startswith('taco_debug_')          # TACO_EINVAL
    torch.cuda.synchronize()
    G.check()
    for k in G.specs:
        assert bool(torch.isnan(G[k]).all()), k
