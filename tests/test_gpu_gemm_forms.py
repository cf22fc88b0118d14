"""GPU: the GEMM forms only the model's own launches build -- the pooled forward and backward epilogues of gemm2.hip and their
two-pass twins, the bank gather, the atomic K-problem batch, the row bias, the grouped and the strided-batch weight gradient --
through the taco_debug_* doors (include/taco_hip.h), against the fp64 references of tests/gemm_forms.py.  The case lists, the
contracts that say which form a case takes and the seam proofs live there and in tests/test_gemm_forms_host.py.

Built from Flat / judge of tests/test_gpu_gemm_paths.py: every tensor is a flat buffer of one guarded arena; outputs start as NaN,
or as random prior content where the call accumulates; the pitch padding of every input is NaN; after each call everything
outside the written region is bytewise what it was.  Bars: rel-L2 <= 5e-6 and gemm_paths.element_bound per element with the
reference's own error scale; for column sums (dgamma, dbeta, dbias) n is the number of summed terms and the scale the sum of the
|terms|, for the fused pooled backward too.  No form needed a wider bar.  The worst figures per label go into the table that
tests/test_gpu_gemm_paths.py writes (write_error_table, GEMM_PATHS_ERRORS_OUT), under a comment line of their own."""
import numpy as np
import pytest
import torch

from tests import gemm_forms as gf
from tests import gemm_paths as gp
from tests.test_gpu_gemm_paths import STATS, Flat, _gemm_labels, judge, write_error_table

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope='module', autouse=True)
def _error_table():
    yield
    write_error_table()
    rows = [k for k in sorted(STATS) if k in gf.FORM_LABELS]
    for k in rows:
        print('  %-18s %6d cases  rel-L2 %.3e  elem-ratio %.3e' % (k, STATS[k][0], STATS[k][1], STATS[k][2]))


def _col(v):
    return np.asarray(v)[None, :]


def _randomise(F, name, rng):
    """random prior content in the whole buffer, pitch padding included (it must survive bytewise)"""
    F.buf(name).copy_(torch.as_tensor(rng.standard_normal(F.buf(name).numel()).astype(F32)).cuda())


# ------------------------------------------------------------------------------------------------------------------
# pooled forward epilogue

@pytest.mark.parametrize('c', gf.POOL_FWD_CASES, ids=[c.id for c in gf.POOL_FWD_CASES])
def test_pooled_forward_epilogue(built_lib, c, monkeypatch):
    """conv bank + ReLU + affine + max-pool as one launch (ConvGemmProblem::pool == 1) at every seam of the 127-row tile stride:
    the successor row in the same lane, in the lane 32 away, in the next wave, in the next tile; the halo row skipped unless it
    ends a sequence.  In every case the two-pass twin, conv + bn_maxpool on the same kernel form into dense rows, must give the
    same bits (gemm_forms.pool_fwd_operands says which gamma makes its factor the fused launch's)."""
    monkeypatch.setenv('TACO_GEMM2_MIN_TILES', '1')
    monkeypatch.setenv('TACO_GEMM2_BF16X', c.bx)
    M, T, Fn, N, K = c.M, c.T, c.F, c.N, c.K
    lda, ldc, FN = K + c.apad, Fn * N + c.cpad, Fn * N
    o = gf.pool_fwd_operands(c)
    x, Ws, bs, scale, shift = o['x'], o['Ws'], o['bs'], o['scale'], o['shift']
    sm = gf.scale_mul_of(c)
    spec = {'x': (M * lda, 'qnan'), 'scale': (FN, 'qnan'), 'shift': (FN, 'qnan'), 'pool': (M * ldc, 'qnan'), 'bank': (M * ldc, 'qnan'),
            'gamma2': (FN, 'qnan'), 'bank2': (M * FN, 'qnan'), 'pool2': (M * FN, 'qnan')}
    for f in range(Fn):
        spec['W%d' % f], spec['b%d' % f] = ((f + 1) * K * N, 'qnan'), (N, 'qnan')
    F = Flat(spec)
    xt = F.put('x', x, 0, lda)
    Wt = [F.put('W%d' % f, Ws[f].reshape((f + 1) * K, N), 0, N) for f in range(Fn)]
    bt = [F.put_vec('b%d' % f, bs[f], 0) for f in range(Fn)]
    st, ht, gt = F.put_vec('scale', scale, 0), F.put_vec('shift', shift, 0), F.put_vec('gamma2', o['gamma'], 0)
    pool = F.out('pool', 0, M, FN, ldc)
    bank = F.out('bank', 0, M, FN, ldc) if c.pre else None
    bank2, pool2 = F.out('bank2', 0, M, FN, FN), F.out('pool2', 0, M, FN, FN)       # the twin's are dense whatever ldc is
    assert gf.pool_contract(1, N, ldc, pool.data_ptr(), bank.data_ptr() if c.pre else None, bias=True, act=1)
    F.snapshot()
    built_lib.weight_image(None)
    imgs = [built_lib.weight_image(Wt[f], taps=f + 1, K=K, N=N) for f in range(Fn)] if c.img else []      # (kept alive to the end)
    ran = []
    labels = _gemm_labels(built_lib, lambda: ran.append(built_lib.debug_conv_bank_pool_fwd(xt, Wt, bt, st, ht, pool, M, T, N, K, scale_mul=sm, bank=bank,
                                                                                           lda=lda, ldc=ldc)))
    assert ran == [True], 'the pooled epilogue did not run (TACO_ENOTFOUND)'
    assert len(labels) == 1 and labels[0].startswith('nn n=%d M=%d N=%d K=%d taps=1..%d pool1' % (Fn, M, N, K, Fn)), labels
    built_lib.debug_gemm2_window(0, 1 << 30)
    for f in range(1, Fn + 1):
        built_lib.conv_gemm(xt, Wt[f - 1], bank2[(f - 1) * N:], M, N, K, taps=f, T=T, pad_l=(f - 1) // 2, act=1, bias=bt[f - 1], lda=lda, ldw=N, ldc=FN)
    assert built_lib.debug_gemm2_window(0, 1 << 30) == Fn, 'the twin convolutions must run on gemm2.hip too'
    built_lib.debug_bn_maxpool_fwd(bank2, gt, ht, pool2, M // T, T, FN)
    # launches that read the weights as pre-split plane images: the fused one and, on the same kernel form, the twin's convolutions
    assert built_lib.weight_image(None) == ((1 + Fn) if c.img else 0) and len(imgs) == (Fn if c.img else 0)
    F.check_untouched()
    ref_pool, ref_bank, S_pool, S_bank, n = gf.pool_fwd_ref(x, Ws, bs, scale, shift, sm, T)
    label = gf.pool_fwd_label(c)
    got_pool = F.get('pool', 0, M, FN, ldc)
    judge(label, c.id + ' pool', got_pool, ref_pool, n, S_pool, 1.0)
    if c.pre:
        got_bank = F.get('bank', 0, M, FN, ldc)
        judge(label, c.id + ' bank', got_bank, ref_bank, n, S_bank, 1.0)
    else:
        assert bool(torch.isnan(F.buf('bank')).all())
    got2 = F.get('pool2', 0, M, FN, FN)
    judge('ew.bnpool.fwd', c.id + ' two-pass pool', got2, ref_pool, n, S_pool, 1.0)
    assert np.array_equal(got2.view(np.int32), got_pool.view(np.int32)), 'fused and two-pass pool differ in %d elements' % int((got2 != got_pool).sum())
    if c.pre:
        assert np.array_equal(F.get('bank2', 0, M, FN, FN).view(np.int32), got_bank.view(np.int32))


def test_pooled_forward_falls_back_where_the_library_does(built_lib, monkeypatch):
    """TACO_GEMM2_MIN_TILES above the batch's tile count, and gemm2.hip switched off: TACO_ENOTFOUND, nothing written"""
    M, T, N, K = 128, 64, 128, 32
    F = Flat({'x': (M * K, 0.5), 'W0': (K * N, 0.5), 'b0': (N, 0.5), 'scale': (N, 1.0), 'shift': (N, 0.0), 'pool': (M * N, 'qnan')})
    F.snapshot()
    for tiles in ('2', '0'):
        monkeypatch.setenv('TACO_GEMM2_MIN_TILES', tiles)
        assert built_lib.debug_conv_bank_pool_fwd(F.buf('x'), [F.buf('W0')], [F.buf('b0')], F.buf('scale'), F.buf('shift'), F.buf('pool'), M, T, N, K) is False
    F.check_untouched()


# ------------------------------------------------------------------------------------------------------------------
# pooled backward epilogue and its two-pass twin

def _check_pool_bwd(label, c, got_dx, got_g, got_b, r, exact):
    judge(label, c.id + ' dx', got_dx, r['dx'], r['n_dx'], r['S_dx'], r['g_dx'])
    judge(label, c.id + ' dgamma', _col(got_g), _col(r['dgamma']), r['n_col'], _col(r['S_g']), 1.0)
    judge(label, c.id + ' dbeta', _col(got_b), _col(r['dbeta']), r['n_col'], _col(r['S_b']), 1.0)
    assert (got_dx[r['dx'] == 0] == 0).all(), 'dx must be exactly 0 where the reference is'
    if exact:       # the grid case: every value the kernel forms is exact in fp32 -- +-dy scale, or (dy[m] + dy[m-1]) scale
        bad = got_dx.astype(np.float64) != r['dx']
        assert not bad.any(), '%s: %d elements of dx differ from the exact value, first at %s' % (c.id, int(bad.sum()), np.argwhere(bad)[0])


@pytest.mark.parametrize('c', gf.POOL_BWD_CASES, ids=[c.id for c in gf.POOL_BWD_CASES])
def test_pooled_backward_epilogue(built_lib, c, monkeypatch):
    """the max-pool / affine / ReLU backward as the epilogue of the GEMM that produces d(pooled) (pool == 2): ownership of rows
    1..127, dy of the previous row from the same lane, the lane 32 away or the wave below, clamped x loads at rows 0 and M - 1, the
    >= / > tie rule (pinned exactly by the grid cases), column sums through LDS and one atomic per column into prior content.
    bn_maxpool_bwd gets the same data (dy given) and the same checks."""
    monkeypatch.setenv('TACO_GEMM2_MIN_TILES', '1')
    monkeypatch.setenv('TACO_GEMM2_BF16X', c.bx)
    M, T, N, K, taps, pad_l = c.M, c.T, c.N, c.K, gf.POOL_BWD_TAPS, gf.POOL_BWD_PAD
    lda, ldc = K + c.apad, N + c.cpad
    grid = c.data == 'grid'
    o = (gf.grid_pool_operands if grid else gf.margin_pool_operands)(c.id, M, T, N, K, taps)
    sm = gf.scale_mul_of(c)
    rng = np.random.default_rng(gp.seed_of(c.id) + 1)
    pg, pb = rng.standard_normal(N).astype(F32), rng.standard_normal(N).astype(F32)
    F = Flat({'A': (M * lda, 'qnan'), 'W': (taps * K * N, 'qnan'), 'x': (M * ldc, 'qnan'), 'scale': (N, 'qnan'), 'shift': (N, 'qnan'),
              'dx': (M * ldc, 'qnan'), 'dg': (N, 'qnan'), 'db': (N, 'qnan'),
              'x2': (M * N, 'qnan'), 'gamma2': (N, 'qnan'), 'dy2': (M * N, 'qnan'), 'dx2': (M * N, 'qnan'), 'dg2': (N, 'qnan'), 'db2': (N, 'qnan')})
    At, Wt = F.put('A', o['A'], 0, lda), F.put('W', o['W'].reshape(taps * K, N), 0, N)
    xt = F.put('x', o['x'], 0, ldc)                 # rows outside [0, M) of pool_x are guard band
    st, ht = F.put_vec('scale', o['scale'].astype(F32), 0), F.put_vec('shift', o['shift'].astype(F32), 0)
    dg, db = F.put_vec('dg', pg, 0), F.put_vec('db', pb, 0)
    dx = F.out('dx', 0, M, N, ldc)
    F.out('dg', 0, 1, N, N), F.out('db', 0, 1, N, N)
    assert gf.pool_contract(2, N, ldc, dx.data_ptr(), pool_x_ptr=xt.data_ptr())
    # reference; the decisions must not depend on rounding: exact on the grid, a margin of 1e-3 otherwise -- for scale_mul and for RS
    r = gf.pool_bwd_ref(o['A'], o['W'], o['x'], o['scale'], o['shift'], sm, T, pad_l, pg.astype(np.float64), pb.astype(np.float64))
    if not grid:
        assert min(gf.decision_margin(o['x'], o['scale'], o['shift'], s, T) for s in (sm, gf.RS)) >= 1e-3
    # the twin's operands: dy as fp32, dense rows; on the grid a gamma whose product with the kernel's own RS is the scale exactly
    dy32 = r['dy'].astype(F32)
    gamma2 = gf.gamma_for_scale(o['scale']) if grid else o['scale'].astype(F32)
    r2 = gf.bn_pool_bwd_ref(o['x'], o['scale'], o['shift'], 1.0 if grid else gf.RS, dy32, np.abs(dy32.astype(np.float64)), T, 0,
                            pg.astype(np.float64), pb.astype(np.float64), gamma_mul=gf.RS)
    if grid:
        assert np.array_equal(dy32.astype(np.float64), r['dy'])
    x2, g2, y2 = F.put('x2', o['x'], 0, N), F.put_vec('gamma2', gamma2, 0), F.put('dy2', dy32, 0, N)
    dg2, db2 = F.put_vec('dg2', pg, 0), F.put_vec('db2', pb, 0)
    dx2 = F.out('dx2', 0, M, N, N)
    F.out('dg2', 0, 1, N, N), F.out('db2', 0, 1, N, N)
    F.snapshot()
    built_lib.weight_image(None)
    img = built_lib.weight_image(Wt, taps=taps, K=K, N=N) if c.img else None
    ran = []
    labels = _gemm_labels(built_lib, lambda: ran.append(built_lib.debug_conv_gemm_pool_bwd(At, Wt, xt, st, ht, dx, dg, db, M, T, N, K, taps=taps, pad_l=pad_l,
                                                                                           scale_mul=sm, lda=lda, ldw=N, ldc=ldc)))
    assert ran == [True], 'the pooled backward epilogue did not run (TACO_ENOTFOUND)'
    assert len(labels) == 1 and ' pool2' in labels[0], labels
    assert built_lib.weight_image(None) == int(c.img) and (img is not None) == c.img
    built_lib.debug_bn_maxpool_bwd(x2, g2, ht, y2, dx2, dg2, db2, M // T, T, N)
    F.check_untouched()
    _check_pool_bwd('g2.pool2', c, F.get('dx', 0, M, N, ldc), F.get('dg', 0, 1, N, N)[0], F.get('db', 0, 1, N, N)[0], r, grid)
    _check_pool_bwd('ew.bnpool.bwd', c, F.get('dx2', 0, M, N, N), F.get('dg2', 0, 1, N, N)[0], F.get('db2', 0, 1, N, N)[0], r2, grid)


def test_pooled_backward_falls_back_where_the_library_does(built_lib, monkeypatch):
    """TACO_DETERMINISTIC=1 and a disabled gemm2.hip: TACO_ENOTFOUND, nothing written, dgamma / dbeta untouched"""
    M, T, N, K = 128, 64, 128, 32
    F = Flat({'A': (M * K, 0.5), 'W': (3 * K * N, 0.5), 'x': (M * N, 0.5), 'scale': (N, 1.0), 'shift': (N, 0.0), 'dx': (M * N, 'qnan'),
              'dg': (N, 7.0), 'db': (N, 7.0)})
    F.snapshot()
    for env, val in (('TACO_DETERMINISTIC', '1'), ('TACO_GEMM2_MIN_TILES', '0')):
        monkeypatch.setenv('TACO_GEMM2_MIN_TILES', '1')
        monkeypatch.setenv(env, val)
        assert built_lib.debug_conv_gemm_pool_bwd(F.buf('A'), F.buf('W'), F.buf('x'), F.buf('scale'), F.buf('shift'), F.buf('dx'), F.buf('dg'), F.buf('db'),
                                                  M, T, N, K) is False
        monkeypatch.delenv(env)
    F.check_untouched()


# ------------------------------------------------------------------------------------------------------------------
# bank gather and the atomic batch

def _gather_operands(c):
    rng = np.random.default_rng(gp.seed_of(c.id))
    M, taps = c.B * c.T, c.F * (c.F + 1) // 2
    return dict(M=M, taps=taps, dbank=rng.standard_normal((M, c.F * c.K)).astype(F32),
                WTs=[(rng.standard_normal((f, c.K, c.N)) / np.sqrt(c.K * taps)).astype(F32) for f in range(1, c.F + 1)],
                res=rng.standard_normal((M, c.N)).astype(F32), prior=rng.standard_normal((M, c.N)).astype(F32), rng=rng)


def _gather_arena(c, d, extra=None):
    M, taps, K, N = d['M'], d['taps'], c.K, c.N
    lda, ldc = c.F * K + c.apad, N + c.apad
    spec = {'dbank': (M * lda, 'qnan'), 'WT': (taps * K * N, 'qnan'), 'res': (M * ldc, 'qnan'), 'dx': (M * ldc, 'qnan')}
    spec.update(extra or {})
    F = Flat(spec)
    At = F.put('dbank', d['dbank'], 0, lda)
    F.put('WT', np.concatenate(d['WTs'], 0).reshape(taps * K, N), 0, N)
    WT = [F.buf('WT')[f * (f + 1) // 2 * K * N:] for f in range(c.F)]          # contiguous, one behind the other
    rt = F.put('res', d['res'], 0, ldc)
    _randomise(F, 'dx', d['rng'])
    F.put('dx', d['prior'], 0, ldc)
    return F, At, WT, rt, lda, ldc


@pytest.mark.parametrize('c', gf.GATHER_CASES, ids=[c.id for c in gf.GATHER_CASES])
def test_bank_gather(built_lib, c, monkeypatch):
    """the conv bank's input gradient as ONE reduction over the taps of all widths (bank_filters) cut into [it0, it1) chunks, then
    the slab sum with residual into prior content: the global tap's column block, row shift and weight slice; a cut inside a
    filter and inside a tap's k-tiles; sequences shorter than the widest kernel"""
    monkeypatch.setenv('TACO_GEMM2_BF16X', c.bx)
    d = _gather_operands(c)
    M, K, N = d['M'], c.K, c.N
    nit, per, chunks = gf.gather_chunks(c.F, K, c.S)
    F, At, WT, rt, lda, ldc = _gather_arena(c, d, {'slabs': (len(chunks) * M * N, 'qnan')})
    dx = F.out('dx', 0, M, N, ldc)
    slabs = F.out('slabs', 0, 1, len(chunks) * M * N, len(chunks) * M * N)
    assert gp.nn_flags(At.data_ptr(), lda, WT[0].data_ptr(), N, N, K) == 3
    F.snapshot()
    built_lib.weight_image(None)
    img = built_lib.weight_image(F.buf('WT'), taps=d['taps'], K=K, N=N) if c.img else None       # one image of all the taps, as the model's
    built_lib.debug_gemm2_window(0, 1 << 30)
    assert built_lib.debug_bank_gather(At, WT, dx, slabs, M, c.T, K, N, c.S, residual=rt, lda=lda, ldc=ldc, ldr=ldc) is True
    assert built_lib.debug_gemm2_window(0, 1 << 30) == 1
    assert built_lib.weight_image(None) == int(c.img) and (img is not None) == c.img
    F.check_untouched()
    ref, S, n = gf.gather_ref(d['dbank'], d['WTs'], c.T, d['res'].astype(np.float64), d['prior'].astype(np.float64))
    # the slab sum adds len(chunks) partial sums, the residual and the prior content: a few more roundings of the running sum, inside (n + 16)
    judge(gf.gather_label(c), c.id, F.get('dx', 0, M, N, ldc), ref, n, S, 1.0)


@pytest.mark.parametrize('why', ('pad_l', 'not-contiguous', 'S=1', 'slabs-too-small', 'gemm2-off'))
def test_bank_gather_refuses_what_the_library_does(built_lib, why, monkeypatch):
    """TACO_ENOTFOUND with nothing written, where cbhg_bwd falls back to the atomic batch"""
    c = next(c for c in gf.GATHER_CASES if c.id == 'bg-F3-T7')
    d = _gather_operands(c)
    M, K, N = d['M'], c.K, c.N
    F, At, WT, rt, lda, ldc = _gather_arena(c, d, {'slabs': (3 * M * N, 'qnan'), 'W2': (2 * K * N, 0.25)})
    kw = dict(residual=rt, lda=lda, ldc=ldc, ldr=ldc)
    slabs, S = F.buf('slabs'), 3
    if why == 'pad_l':
        kw['pad_l'] = 0                        # forward pad of F = 3 is 1, the backward pad the kernel needs is 1 as well: 0 is neither
    elif why == 'not-contiguous':
        WT = [WT[0], F.buf('W2'), WT[2]]
    elif why == 'S=1':
        S = 1
    elif why == 'slabs-too-small':
        slabs = slabs[:3 * M * N - 1]
    else:
        monkeypatch.setenv('TACO_GEMM2_MIN_TILES', '0')
    F.snapshot()
    assert built_lib.debug_bank_gather(At, WT, F.buf('dx'), slabs, M, c.T, K, N, S, **kw) is False
    F.check_untouched()


@pytest.mark.parametrize('c,g2', gf.ATOMIC_CASES, ids=['%s-g2=%s' % (c.id, g2) for c, g2 in gf.ATOMIC_CASES])
def test_atomic_batch(built_lib, c, g2, monkeypatch):
    """the gather's fall-back: F transposed convolutions as F problems of one launch that add into dx_out with fp32 atomics, the
    residual on the width-1 problem -- on gemm.hip's kernel and on gemm2.hip's, to the same bound as the gather"""
    monkeypatch.setenv('TACO_GEMM2_MIN_TILES', g2)
    monkeypatch.setenv('TACO_GEMM2_BF16X', c.bx)
    d = _gather_operands(c)
    M, K, N = d['M'], c.K, c.N
    F, At, WT, rt, lda, ldc = _gather_arena(c, d)
    dx = F.out('dx', 0, M, N, ldc)
    F.snapshot()
    built_lib.weight_image(None)
    built_lib.debug_gemm2_window(0, 1 << 30)
    labels = _gemm_labels(built_lib, lambda: built_lib.debug_conv_gemm_batch_atomic(At, WT, dx, M, c.T, K, N, residual=rt, lda=lda, ldc=ldc, ldr=ldc))
    assert built_lib.debug_gemm2_window(0, 1 << 30) == int(g2)
    assert len(labels) == 1 and labels[0].startswith('nn n=%d ' % c.F) and ' atomic' in labels[0], labels
    F.check_untouched()
    ref, S, n = gf.gather_ref(d['dbank'], d['WTs'], c.T, d['res'].astype(np.float64), d['prior'].astype(np.float64))
    judge('nn.atomic', '%s g2=%s' % (c.id, g2), F.get('dx', 0, M, N, ldc), ref, n, S, 1.0)


@pytest.mark.parametrize('c', gf.ROWBIAS_CASES, ids=[c.id for c in gf.ROWBIAS_CASES])
def test_row_bias(built_lib, c, monkeypatch):
    """bias_stride: the per-sequence bias of the speaker sites, a tile spanning two sequences, rowb dense and pitched"""
    monkeypatch.setenv('TACO_GEMM2_MIN_TILES', c.g2)
    M, T, N, K, B = c.M, c.T, c.N, c.K, c.M // c.T
    stride = N + c.stride_pad
    rng = np.random.default_rng(gp.seed_of(c.id))
    A, W, rowb = rng.standard_normal((M, K)).astype(F32), (rng.standard_normal((K, N)) / np.sqrt(K)).astype(F32), rng.standard_normal((B, N)).astype(F32)
    F = Flat({'A': (M * K, 'qnan'), 'W': (K * N, 'qnan'), 'rowb': (B * stride, 'qnan'), 'C': (M * N, 'qnan')})
    At, Wt, bt = F.put('A', A, 0, K), F.put('W', W, 0, N), F.put('rowb', rowb, 0, stride)
    Ct = F.out('C', 0, M, N, N)
    F.snapshot()
    built_lib.weight_image(None)
    built_lib.debug_gemm2_window(0, 1 << 30)
    labels = _gemm_labels(built_lib, lambda: built_lib.debug_conv_gemm_rowbias(At, Wt, bt, Ct, M, T, N, K, bias_stride=stride))
    assert built_lib.debug_gemm2_window(0, 1 << 30) == int(c.g2)
    assert len(labels) == 1 and labels[0].endswith(' rowbias'), labels
    F.check_untouched()
    ref, S = gf.rowbias_ref(A, W, rowb, T)
    judge('nn.rowbias', c.id, F.get('C', 0, M, N, N), ref, K, S, 1.0)


# ------------------------------------------------------------------------------------------------------------------
# grouped and strided-batch weight gradients

@pytest.mark.parametrize('group,dbias,merge,det', gf.TN_GROUP_RUNS, ids=['%s-dbias%d-merge%s-det%s' % r for r in gf.TN_GROUP_RUNS])
def test_grouped_tn(built_lib, group, dbias, merge, det, monkeypatch):
    """launch_gemm_tn_batch: problems of differing (M, N, K, taps, pad_l) in ONE grid, accumulated into prior content, dbias
    added once per problem (tap 0 / k-tile 0 only), with merged and unmerged taps and in deterministic mode.  The same problems
    one by one through taco_gemm_tn must agree to the bound."""
    monkeypatch.setenv('TACO_TN2', '0')
    monkeypatch.setenv('TACO_TN_MERGE_TAPS', merge)
    monkeypatch.setenv('TACO_DETERMINISTIC', det)
    probs = gf.TN_GROUPS[group]
    rng = np.random.default_rng(gp.seed_of(group))
    data, spec = [], {}
    for i, p in enumerate(probs):
        data.append(dict(A=rng.standard_normal((p.M, p.K)).astype(F32), Y=rng.standard_normal((p.M, p.N)).astype(F32),
                         W0=rng.standard_normal((p.taps * p.K, p.N)).astype(F32), b0=rng.standard_normal(p.N).astype(F32)))
        spec.update({'A%d' % i: (p.M * p.K, 'qnan'), 'Y%d' % i: (p.M * p.N, 'qnan'), 'W%d' % i: (p.taps * p.K * p.N, 'qnan'), 'b%d' % i: (p.N, 'qnan'),
                     'V%d' % i: (p.taps * p.K * p.N, 'qnan')})
    F = Flat(spec)
    args = []
    for i, (p, d) in enumerate(zip(probs, data)):
        At, Yt = F.put('A%d' % i, d['A'], 0, p.K), F.put('Y%d' % i, d['Y'], 0, p.N)
        F.put('W%d' % i, d['W0'], 0, p.N), F.put('V%d' % i, d['W0'], 0, p.N), F.put_vec('b%d' % i, d['b0'], 0)
        Wt, Vt = F.out('W%d' % i, 0, p.taps * p.K, p.N, p.N), F.out('V%d' % i, 0, p.taps * p.K, p.N, p.N)
        bt = F.out('b%d' % i, 0, 1, p.N, p.N) if dbias else None
        args.append(dict(A=At, Y=Yt, W=Wt, V=Vt, dbias=bt, M=p.M, T=p.T, N=p.N, K=p.K, taps=p.taps, pad_l=p.pad_l))
    F.snapshot()
    labels = _gemm_labels(built_lib, lambda: built_lib.debug_gemm_tn_group([{k: v for k, v in a.items() if k != 'V'} for a in args]))
    assert len(labels) == 1 and labels[0].startswith('tn-batch n=%d ' % len(probs)), labels     # all of them in ONE grid
    for a in args:
        built_lib.gemm_tn(a['A'], a['Y'], a['V'], a['M'], a['N'], a['K'], taps=a['taps'], T=a['T'], pad_l=a['pad_l'], accumulate=True)
    F.check_untouched()
    for i, (p, d) in enumerate(zip(probs, data)):
        ref, S, rb, Sb = gf.tn_group_ref(p, d['A'], d['Y'], d['W0'].astype(np.float64), d['b0'].astype(np.float64) if dbias else None)
        what = '%s[%d] taps=%d K=%d N=%d' % (group, i, p.taps, p.K, p.N)
        got = F.get('W%d' % i, 0, p.taps * p.K, p.N, p.N)
        judge('tn.group', what + ' dW', got, ref, p.M, S, 1.0)
        one = F.get('V%d' % i, 0, p.taps * p.K, p.N, p.N)
        judge('tn.group', what + ' dW one by one', one, ref, p.M, S, 1.0)
        assert (np.abs(got.astype(np.float64) - one) <= 2 * gp.element_bound(p.M, S, 1.0, ref)).all()
        if dbias:
            judge('tn.group', what + ' dbias', _col(F.get('b%d' % i, 0, 1, p.N, p.N)[0]), _col(rb), p.M, _col(Sb), 1.0)


@pytest.mark.parametrize('c', gf.TN_STRIDED_CASES, ids=[c.id for c in gf.TN_STRIDED_CASES])
def test_strided_batch_tn(built_lib, c, monkeypatch):
    """batch / strideA / strideY / strideW: the decoder's d keys product, pad_l = 1 (row 0 of every member meets a zero row: the
    alignments of the previous step), dY records with a pitch and a member stride that is no multiple of it, accumulated"""
    monkeypatch.setenv('TACO_TN2', '0')
    Bn, M, K, N = c.batch, c.M, c.K, gf.TN_STRIDED_N
    lda, ldy, ldw = K, N + 4, 2 * N
    sA, sY, sW = M * lda, M * ldy + 12, K * ldw
    rng = np.random.default_rng(gp.seed_of(c.id))
    A, Y = rng.standard_normal((Bn, M, K)).astype(F32), rng.standard_normal((Bn, M, N)).astype(F32)
    W0 = rng.standard_normal((Bn, K, N)).astype(F32)
    F = Flat({'A': (Bn * sA, 'qnan'), 'Y': (Bn * sY, 'qnan'), 'W': (Bn * sW, 'qnan')})
    _randomise(F, 'W', rng)
    for z in range(Bn):
        F.put('A', A[z], z * sA, lda), F.put('Y', Y[z], z * sY, ldy), F.put('W', W0[z], z * sW, ldw)
        F.out('W', z * sW, K, N, ldw)
    F.snapshot()
    labels = _gemm_labels(built_lib, lambda: built_lib.debug_gemm_tn_strided(F.buf('A'), F.buf('Y'), F.buf('W'), M, N, K, Bn, sA, sY, sW, pad_l=1,
                                                                             lda=lda, ldy=ldy, ldw=ldw))
    assert len(labels) == 1 and labels[0].startswith('tn M=%d N=%d K=%d taps=1 batch=%d ' % (M, N, K, Bn)), labels
    F.check_untouched()
    ref, S = gf.tn_strided_ref(A, Y, W0.astype(np.float64), 1)
    got = np.stack([F.get('W', z * sW, K, N, ldw) for z in range(Bn)])
    judge('tn.strided', c.id, got.reshape(Bn * K, N), ref.reshape(Bn * K, N), M + 1, S.reshape(Bn * K, N), 1.0)
