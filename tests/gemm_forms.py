"""What the op-level tests of the GEMM forms only the model reaches share (no GPU needed to import): fp64 references with error
scales, a Python restatement of the launchers' contracts, and the enumerated case lists.  Sibling of tests/gemm_paths.py, whose
references (nn_ref, tn_ref), error bound (element_bound) and PATH_TABLE it builds on; the forms run through the taco_debug_* doors of
include/taco_hip.h ("op-level debug doors of the GEMM forms").

References
  pool_fwd_ref     conv bank + ReLU -> bank;  z = bank scale scale_mul + shift;  pool[m] = max(z[m], z[m + 1]) inside a sequence
  pool_bwd_ref     dy = the GEMM;  the >= / > routing of kernels.h (ConvGemmProblem::pool == 2) written out;  dx, dgamma, dbeta
  bn_pool_bwd_ref  the same routing with dy given (bn_maxpool_bwd_kernel)
  gather_ref       the bank gather restated from the kernels.h comment (global tap g = f (f - 1) / 2 + j);  gather_ref_convs: the same
                   sum independently as F transposed 'same' convolutions through nn_ref
  rowbias_ref, tn_group_ref, tn_strided_ref

Restated contracts (tacotron_amd/csrc/gemm2.hip): m_tiles, pool_contract, gather_contract (dma_contract's bank_filters clause),
gather_chunks (cbhg_bwd's [it0, it1) cut with S given), tile_rows (which local row of which m-tile a row is).

Path labels added to gemm_paths.PATH_TABLE (tests/test_gemm_forms_host.py requires the case lists to reach every one)
  g2.pool1.f32 / g2.pool1.bx   the pooled forward epilogue in both MFMA forms
  g2.pool2                     the pooled backward epilogue
  ew.bnpool.fwd / ew.bnpool.bwd   their two-pass twins (elementwise.hip)
  g2.bank.S2 / g2.bank.S3      the bank gather with the number of chunks that really run
  nn.atomic                    the K-problem atomic_out batch (gemm.hip's kernel and gemm2.hip's)
  nn.rowbias                   bias_stride
  tn.group / tn.strided        launch_gemm_tn_batch's grouped grid; batch / strideA / strideY / strideW
"""
from collections import namedtuple

import numpy as np

from tests import gemm_paths as gp

BN_EPS = np.float32(1e-3)                                        # common.h kBnEps
RS = float(np.float32(1) / np.sqrt(np.float32(1) + BN_EPS))      # 1 / sqrtf(1 + eps) as the host and the kernels form it, in fp32
TM = 128

FORM_LABELS = ('g2.pool1.f32', 'g2.pool1.bx', 'g2.pool2', 'ew.bnpool.fwd', 'ew.bnpool.bwd', 'g2.bank.S2', 'g2.bank.S3', 'nn.atomic',
               'nn.rowbias', 'tn.group', 'tn.strided')

# ------------------------------------------------------------------------------------------------------------------
# restated contracts


def m_tiles(M, pool):
    """gemm2.hip m_tiles: pooled problems advance by TM - 1 rows (the last row of a tile is the next tile's first)"""
    return gp.cdiv(M - 1 if M > 1 else 1, TM - 1) if pool else gp.cdiv(M, TM)


def tile_rows(M, pool):
    """[(tmm, m0, [rows of the tile that exist])]"""
    step = TM - 1 if pool else TM
    return [(t, t * step, list(range(t * step, min(M, t * step + TM)))) for t in range(m_tiles(M, pool))]


def pool_contract(pool, N, ldc, c_ptr, cpre_ptr=None, keep=False, residual=False, bias_stride=0, atomic_out=False, it0=0, it1=0,
                  pool_x_ptr=None, has_dgamma=True, has_dbeta=True, has_scale=True, has_shift=True, bias=False, act=0):
    common = (N % 4 == 0 and ldc % 4 == 0 and c_ptr % 16 == 0 and (cpre_ptr is None or cpre_ptr % 16 == 0) and not keep and
              not residual and bias_stride == 0 and not atomic_out and it0 == 0 and it1 == 0)
    if pool == 2:
        return (common and pool_x_ptr is not None and pool_x_ptr % 16 == 0 and has_dgamma and has_dbeta and has_scale and has_shift and
                cpre_ptr is None and not bias and act == 0)
    return common


def gather_contract(F, K, taps, pad_l, lda):
    """the bank_filters clause of gemm2.hip dma_contract"""
    return F == 0 or (taps == F * (F + 1) // 2 and K % 32 == 0 and pad_l == (F - 1) - (F - 1) // 2 and lda >= F * K)


def gather_chunks(F, K, S):
    """cbhg_bwd's cut of the (tap, 32-deep k-tile) sequence: -> (nit, per, [(it0, it1)])"""
    nit = F * (F + 1) // 2 * (K // 32)
    per = gp.cdiv(nit, S)
    return nit, per, [(c * per, min(nit, (c + 1) * per)) for c in range(gp.cdiv(nit, per))]


def gather_tap(g):
    """global tap g -> (f, j): the filter width it belongs to and its tap inside that filter"""
    f = 1
    while g >= f:
        g -= f
        f += 1
    return f, g


# ------------------------------------------------------------------------------------------------------------------
# references


def _equivalent_scale(n, bound, ref):
    """S such that gemm_paths.element_bound(n, S, 1, ref) == bound (bound >= the |ref| term by construction)"""
    S = (bound - 8 * 2.0 ** -24 * np.abs(ref)) / ((n + 16) * 2.0 ** -23)
    assert (S >= -1e-30).all()
    return np.maximum(S, 0)


def _has_next(M, T):
    return (np.arange(M) % T) + 1 < T


def pool_fwd_ref(x, Ws, biases, scale, shift, scale_mul, T):
    """x (M, K); Ws[f-1] (f, K, N); scale, shift (F N) -> (pool, bank, S_pool, S_bank, n): element_bound(n[f], S_bank, 1, bank) bounds
    bank; element_bound(n[f], S_pool, 1, pool) is the larger of the bounds of the two z rows a pooled element is the max of (max is
    1-Lipschitz in each argument), the affine's factor |scale scale_mul| folded into S_pool.  n: (F N) products per column."""
    M = x.shape[0]
    F, N = len(Ws), Ws[0].shape[2]
    bank, S_bank, n = np.zeros((M, F * N)), np.zeros((M, F * N)), np.zeros(F * N)
    for f in range(1, F + 1):
        _, pre, S = gp.nn_ref(x, Ws[f - 1], biases[f - 1], T, (f - 1) // 2, 1)
        bank[:, (f - 1) * N:f * N], S_bank[:, (f - 1) * N:f * N], n[(f - 1) * N:f * N] = pre, S, f * x.shape[1]
    sc = np.asarray(scale, np.float64) * float(scale_mul)
    z = bank * sc + np.asarray(shift, np.float64)
    bz = gp.element_bound(n, S_bank, np.abs(sc), z)
    nxt = _has_next(M, T)
    pool, bp = z.copy(), bz.copy()
    pool[nxt] = np.maximum(z[nxt], z[1:][nxt[:-1]])
    bp[nxt] = np.maximum(bz[nxt], bz[1:][nxt[:-1]])
    return pool, bank, _equivalent_scale(n, bp, pool), S_bank, n


def _route(z, dy, T):
    """kernels.h: dz[m] = [last or z[m] >= z[m+1]] dy[m] + [not first and z[m] > z[m-1]] dy[m-1] -> (dz, ge, gt)"""
    M = z.shape[0]
    t = np.arange(M) % T
    first, last = (t == 0)[:, None], (t == T - 1)[:, None]
    zn, zp, dyp = np.roll(z, -1, 0), np.roll(z, 1, 0), np.roll(dy, 1, 0)
    ge = last | (z >= zn)
    gt = ~first & (z > zp)
    return ge * dy + gt * dyp, ge, gt


def decision_margin(x, scale, shift, scale_mul, T):
    """smallest |z[m] - z[m+1]| over neighbours of one sequence"""
    z = np.asarray(x, np.float64) * (np.asarray(scale, np.float64) * float(scale_mul)) + np.asarray(shift, np.float64)
    nxt = _has_next(z.shape[0], T)
    d = np.abs(z[nxt] - z[1:][nxt[:-1]])
    return float(d.min()) if d.size else np.inf


def bn_pool_bwd_ref(x, scale, shift, scale_mul, dy, S_dy, T, n_dy, prior_g=None, prior_b=None, gamma_mul=None):
    """dy (M, N) with its error scale S_dy and product count n_dy (a dy that is given, not computed: S_dy = |dy|, n_dy = 0).  scale is
    what multiplies x AFTER scale_mul is applied to it; gamma_mul (default scale_mul) is the factor of dgamma = sum dz x gamma_mul.
    -> dict(dx, dgamma, dbeta, S_dx, S_g, S_b, n_dx, n_col, dz).  dx is EXACTLY 0 where x <= 0 (S_dx is 0 there).  Column sums: n_col
    = M summed terms, S_b = sum |dz| and S_g = sum |dz x| gamma_mul (plus |prior content|), for the fused epilogue too: the error its
    GEMM leaves in every dz has to fit into the same bar."""
    x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    M = x.shape[0]
    sc = np.asarray(scale, np.float64) * float(scale_mul)
    z = x * sc + np.asarray(shift, np.float64)
    dz, ge, gt = _route(z, dy, T)
    S_dz = ge * S_dy + gt * np.roll(S_dy, 1, 0)
    # every dy is routed exactly once: to its own row, or (inside a sequence, when the next row is strictly larger) to the next row
    assert np.allclose(dz.sum(0), dy.sum(0), rtol=0, atol=1e-12 * (np.abs(dy).sum(0).max() + 1))
    t = np.arange(M) % T
    to_next = np.roll(gt, -1, 0) & (t != T - 1)[:, None]
    assert ((ge.astype(int) + to_next.astype(int)) == 1).all()
    pos = x > 0
    gm = float(scale_mul if gamma_mul is None else gamma_mul)
    out = dict(dz=dz, dx=pos * dz * sc, S_dx=pos * S_dz, dgamma=(dz * x).sum(0) * gm, dbeta=dz.sum(0),
               S_g=np.abs(dz * x).sum(0) * gm, S_b=np.abs(dz).sum(0), n_dx=n_dy + 1, n_col=M, g_dx=np.abs(sc))
    if prior_g is not None:
        out['dgamma'], out['S_g'] = out['dgamma'] + prior_g, out['S_g'] + np.abs(prior_g)
    if prior_b is not None:
        out['dbeta'], out['S_b'] = out['dbeta'] + prior_b, out['S_b'] + np.abs(prior_b)
    return out


def pool_bwd_ref(A, W, x, scale, shift, scale_mul, T, pad_l, prior_g=None, prior_b=None):
    """A (M, K), W (taps, K, N): dy = the GEMM, then bn_pool_bwd_ref.  Also returns dy."""
    dy, _, S_dy = gp.nn_ref(A, W, None, T, pad_l, 0)
    out = bn_pool_bwd_ref(x, scale, shift, scale_mul, dy, S_dy, T, W.shape[0] * W.shape[1], prior_g, prior_b)
    out['dy'] = dy
    return out


def gather_ref(dbank, WTs, T, residual=None, prior=None):
    """The kernels.h comment restated: taps of all F widths in order, global tap g = f (f - 1) / 2 + j reads the rows shifted by
    j - ((f - 1) - (f - 1) / 2) from the K-column block f - 1 of dbank and the g-th (K, N) slice of the contiguous weights.
    -> (dx, S, n)"""
    F = len(WTs)
    K, N = WTs[0].shape[1:]
    Wall = np.concatenate([np.asarray(w, np.float64) for w in WTs], 0)          # (F (F + 1) / 2, K, N)
    dbank = np.asarray(dbank, np.float64)
    out, S = np.zeros((dbank.shape[0], N)), np.zeros((dbank.shape[0], N))
    for g in range(F * (F + 1) // 2):
        f, j = gather_tap(g)
        assert g == f * (f - 1) // 2 + j
        a = gp._shifted(dbank[:, (f - 1) * K:f * K], T, j - ((f - 1) - (f - 1) // 2))
        out += a @ Wall[g]
        S += np.abs(a) @ np.abs(Wall[g])
    for extra in (residual, prior):
        if extra is not None:
            out, S = out + extra, S + np.abs(extra)
    return out, S, F * (F + 1) // 2 * K


def gather_ref_convs(dbank, WTs, T, residual=None, prior=None):
    """independently: the sum of F transposed 'same' convolutions, each through nn_ref with its own backward pad"""
    K = WTs[0].shape[1]
    out = 0.0
    for f in range(1, len(WTs) + 1):
        out = out + gp.nn_ref(np.asarray(dbank)[:, (f - 1) * K:f * K], WTs[f - 1], None, T, (f - 1) - (f - 1) // 2, 0)[0]
    for extra in (residual, prior):
        if extra is not None:
            out = out + extra
    return out


def rowbias_ref(A, W, rowb, T):
    """C = A . W + rowb[m // T] -> (C, S)"""
    C, _, S = gp.nn_ref(A, np.asarray(W)[None], None, A.shape[0], 0, 0)
    rb = np.repeat(np.asarray(rowb, np.float64), T, 0)
    return C + rb, S + np.abs(rb)


def tn_group_ref(p, A, Y, W0, b0=None):
    """one problem of a grouped launch: dW = prior + shift(A)^T Y, dbias = prior + sum_m Y -> (dW, S, dbias, S_b)"""
    dW, S = gp.tn_ref(A, Y, p.taps, p.T, p.pad_l)
    dW, S = dW.reshape(p.taps * p.K, p.N) + W0, S.reshape(p.taps * p.K, p.N) + np.abs(W0)
    if b0 is None:
        return dW, S, None, None
    Y = np.asarray(Y, np.float64)
    return dW, S, Y.sum(0) + b0, np.abs(Y).sum(0) + np.abs(b0)


def tn_strided_ref(A, Y, W0, pad_l):
    """A (batch, M, K), Y (batch, M, N), W0 (batch, K, N): every member on its own, a sequence of T = M rows -> (dW, S)"""
    outs = [gp.tn_ref(A[z], Y[z], 1, A.shape[1], pad_l) for z in range(A.shape[0])]
    return np.stack([o[0][0] for o in outs]) + W0, np.stack([o[1][0] for o in outs]) + np.abs(W0)


# ------------------------------------------------------------------------------------------------------------------
# operands


def grid_pool_operands(case_id, M, T, N, K, taps):
    """The tie-rule case: every value on a coarse binary grid, so that dy, z, the decisions and dx are exact in fp32 and in fp64.
    x: multiples of 2^-4 in [0, 2], about half exact zeros, planted runs of equal neighbours; scale per column from {1, -1, 0.5,
    -0.5, 0, 2}; shift multiples of 2^-4; A multiples of 2^-2, W of 2^-3 (dy: sums of <= taps K multiples of 2^-5 below 2^7);
    columns 6 and 7 of x are all zero (dx exactly 0 there while dbeta still receives the gradient)."""
    rng = np.random.default_rng(gp.seed_of(case_id))
    x = rng.integers(0, 33, (M, N)) / 16.0
    x[rng.random((M, N)) < 0.5] = 0.0
    for _ in range(M * N // 24):                      # runs of 2 .. 5 equal neighbours
        m, n, L = rng.integers(0, M), rng.integers(0, N), rng.integers(2, 6)
        x[m:m + L, n] = x[m, n]
    x[:, 6:8] = 0.0
    scale = np.array([1, -1, 0.5, -0.5, 0, 2])[np.arange(N) % 6].astype(np.float64)
    shift = rng.integers(-16, 17, N) / 16.0
    A = rng.integers(-4, 5, (M, K)) / 4.0
    W = rng.integers(-4, 5, (taps, K, N)) / 8.0
    return dict(x=x, scale=scale, shift=shift, A=A, W=W)


def margin_pool_operands(case_id, M, T, N, K, taps):
    """The general case: x >= 0 on a 2^-6 grid with no two equal neighbours in a column (zeros included, never two in a row),
    |scale| in [0.25, 2]: every decision has a margin of 2^-6 / 4 > 1e-3 whatever scale_mul in [0.99, 1] is."""
    rng = np.random.default_rng(gp.seed_of(case_id))
    x = rng.integers(3, 129, (M, N)).astype(np.float64)
    x[rng.random((M, N)) < 0.35] = 0.0
    for m in range(1, M):
        same = x[m] == x[m - 1]
        x[m, same] = np.where(x[m - 1, same] == 0, 5.0 + (m % 7), 0.0)
    x /= 64.0
    scale = rng.uniform(0.25, 2.0, N) * rng.choice([-1.0, 1.0], N)
    f = np.float32
    return dict(x=x.astype(f), scale=scale.astype(f), shift=rng.standard_normal(N).astype(f), A=rng.standard_normal((M, K)).astype(f),
                W=(rng.standard_normal((taps, K, N)) / np.sqrt(K * taps)).astype(f))


def pool_fwd_operands(c):
    """Operands of a pooled-forward case.  gamma: what the two-pass twin (bn_maxpool, which multiplies by its own 1 / sqrt(1 + eps))
    is given so that it applies the fused launch's factor to the bit: the scale itself where scale_mul is RS; where scale_mul is 1
    the scale IS fl(gamma RS) of a random gamma."""
    rng = np.random.default_rng(gp.seed_of(c.id))
    f32, FN = np.float32, c.F * c.N
    x = rng.standard_normal((c.M, c.K)).astype(f32)
    Ws = [(rng.standard_normal((f, c.K, c.N)) / np.sqrt(c.K * f)).astype(f32) for f in range(1, c.F + 1)]
    bs = [rng.standard_normal(c.N).astype(f32) for _ in range(c.F)]
    gamma, shift = rng.standard_normal(FN).astype(f32), rng.standard_normal(FN).astype(f32)
    scale = gamma if c.smul == 'rs' else (gamma * f32(RS)).astype(f32)
    return dict(x=x, Ws=Ws, bs=bs, scale=scale, shift=shift, gamma=gamma)


def gamma_for_scale(scale):
    """fp32 gamma with fl(gamma * RS) == scale exactly (the two-pass kernels multiply gamma by their own 1 / sqrt(1 + eps)): RS < 1, so
    consecutive floats near scale / RS have products less than one unit of scale apart and one of them rounds onto it"""
    rs = np.float32(RS)
    out = np.zeros(len(scale), np.float32)
    for i, s in enumerate(np.asarray(scale, np.float32)):
        up = dn = np.float32(s / rs)
        cands = [up]
        for _ in range(4):
            up, dn = np.nextafter(up, np.float32(np.inf)), np.nextafter(dn, np.float32(-np.inf))
            cands += [up, dn]
        hit = [g for g in cands if np.float32(g * rs) == s]
        assert hit, s
        out[i] = hit[0]
    return out


# ------------------------------------------------------------------------------------------------------------------
# case lists

# (a) pooled forward epilogue.  F filters of widths 1..F (taps 1..F), N columns each, ldc = F N + cpad, lda = K + apad; pre: store bank
#     (Cpre); smul: '1' or 'rs'; bx: TACO_GEMM2_BF16X.  The (M, T) pairs place sequence ends and starts on the seams of the 127-row
#     tile stride (tests/test_gemm_forms_host.py proves which).
PF = namedtuple('PF', 'id M T F N K cpad apad pre smul bx img', defaults=(False,))
POOL_FWD_CASES = [
    PF('pf-127x127',      127, 127, 1, 128, 32, 0, 0, True,  'rs', '1'),
    PF('pf-128x128',      128, 128, 3, 128, 32, 0, 0, True,  'rs', '1', True),
    PF('pf-128x2',        128,   2, 1, 132, 64, 4, 4, False, '1',  '0'),
    PF('pf-129x129',      129, 129, 3,   4, 32, 4, 0, True,  '1',  '1'),
    PF('pf-129x1',        129,   1, 3, 132, 32, 0, 0, True,  'rs', '0'),
    PF('pf-254x127',      254, 127, 3, 128, 64, 0, 4, False, 'rs', '1', True),
    PF('pf-255x5',        255,   5, 1,   4, 64, 0, 0, True,  'rs', '0'),
    PF('pf-256x128',      256, 128, 3, 132, 32, 4, 0, True,  '1',  '1', True),
    PF('pf-256x2',        256,   2, 3, 128, 32, 0, 0, True,  'rs', '0'),
    PF('pf-256x2-F1',     256,   2, 1, 128, 64, 4, 0, False, '1',  '1'),
    PF('pf-260x52',       260,  52, 3,   4, 64, 0, 0, False, 'rs', '1', True),
    PF('pf-252x126',      252, 126, 1, 132, 32, 0, 0, True,  'rs', '1'),
    PF('pf-260x5',        260,   5, 3, 128, 32, 4, 4, True,  'rs', '0'),
]

# (b) pooled backward epilogue: one problem, taps 3, pad_l 1; ldc = N + cpad (pool_x and C share it).  data: 'margin' or 'grid' (the
#     tie-rule case, scale_mul 1).  Every row also runs bn_maxpool_bwd (dense, scale_mul = RS) on its own data with dy given.
PB = namedtuple('PB', 'id M T N K cpad apad smul bx data img', defaults=(False,))
POOL_BWD_CASES = [
    PB('pb-127x127',      127, 127, 128, 32, 0, 0, 'rs', '1', 'margin', True),
    PB('pb-128x128',      128, 128, 132, 64, 4, 0, '1',  '0', 'margin'),
    PB('pb-128x2',        128,   2,   4, 32, 0, 4, 'rs', '1', 'margin'),
    PB('pb-129x129',      129, 129, 128, 64, 4, 0, 'rs', '0', 'margin'),
    PB('pb-129x1',        129,   1, 132, 32, 0, 0, '1',  '1', 'margin'),
    PB('pb-254x127',      254, 127,   4, 64, 4, 0, 'rs', '1', 'margin'),
    PB('pb-255x5',        255,   5, 128, 32, 0, 0, 'rs', '0', 'margin'),
    PB('pb-256x128',      256, 128, 128, 32, 0, 4, '1',  '1', 'margin'),
    PB('pb-256x2',        256,   2, 132, 32, 4, 0, 'rs', '1', 'margin', True),
    PB('pb-260x52',       260,  52, 128, 64, 0, 0, 'rs', '0', 'margin'),
    PB('pb-252x126',      252, 126, 128, 32, 4, 0, 'rs', '1', 'margin'),
    PB('pb-tie-254x127',  254, 127, 128, 32, 0, 0, '1',  '1', 'grid', True),
    PB('pb-tie-256x128',  256, 128, 132, 32, 4, 0, '1',  '0', 'grid'),
    PB('pb-tie-260x5',    260,   5, 128, 32, 0, 0, '1',  '1', 'grid'),
]
POOL_BWD_TAPS, POOL_BWD_PAD = 3, 1

# (c) bank gather: F widths, K columns per block, lda = F K + apad, M = B T, S chunks asked for (`chunks`: what gather_chunks gives).
#     T = F - 1 and T = F: a sequence shorter than / as long as the widest kernel.
BG = namedtuple('BG', 'id F K apad N T B S bx img', defaults=(False,))
GATHER_CASES = [
    BG('bg-F1-K64',       1, 64, 0, 128,   7,  3, 2, '1'),      # nit 2: the cut falls between the two k-tiles of the only tap
    BG('bg-F2-T1',        2, 32, 4,  80,   1,  5, 2, '1'),      # nit 3, per 2: S does not divide nit; the cut falls inside filter 2
    BG('bg-F2-T2',        2, 64, 0, 132,   2,  4, 3, '0'),      # nit 6, per 2: one tap per chunk
    BG('bg-F3-T2',        3, 32, 0, 128,   2,  7, 2, '1'),      # T = F - 1
    BG('bg-F3-T130',      3, 64, 4,  80, 130,  2, 3, '1', True),      # three m-tiles
    BG('bg-F4-T3',        4, 64, 0, 132,   3,  5, 3, '1', True),      # nit 20, per 7: cuts at 7 and 14, inside taps 3 and 7 and inside filters 3 and 4
    BG('bg-F4-T4',        4, 32, 0, 128,   4, 33, 3, '0'),      # nit 10, per 4: last chunk 2
    BG('bg-F4-T130',      4, 64, 4,  80, 130,  1, 2, '1'),      # nit 20, per 10: the cut falls inside filter 4
    BG('bg-F3-T7',        3, 32, 0, 132,   7, 19, 3, '1'),
]
# the same operands through the K-problem atomic batch, on gemm.hip's kernel (g2 '0') and on gemm2.hip's ('1')
ATOMIC_CASES = [(c, g2) for c in GATHER_CASES for g2 in ('0', '1')]

# (d) row bias: B = 3 sequences of T = 50 rows, so that one 64-row tile (and one 128-row tile) spans two sequences
RB = namedtuple('RB', 'id M T N K stride_pad g2')
ROWBIAS_CASES = [RB('rb-dense-nn', 150, 50, 132, 64, 0, '0'), RB('rb-pitch-nn', 150, 50, 132, 64, 4, '0'),
                 RB('rb-dense-g2', 150, 50, 132, 64, 0, '1'), RB('rb-pitch-g2', 150, 50, 132, 64, 4, '1')]

# (e) grouped TN: the problems of one launch_gemm_tn_batch call
TG = namedtuple('TG', 'M T N K taps pad_l')
TN_GROUPS = {
    'tg-5': [TG(260, 65, 128, 80, 8, 3), TG(63, 63, 4, 128, 3, 1), TG(260, 130, 128, 132, 1, 0), TG(63, 21, 128, 128, 3, 1), TG(260, 52, 4, 80, 1, 0)],
    'tg-3': [TG(63, 63, 128, 132, 3, 1), TG(260, 260, 4, 80, 8, 3), TG(260, 20, 128, 128, 1, 0)],
}
TN_GROUP_RUNS = [(g, dbias, merge, det) for g in TN_GROUPS for dbias in (False, True) for merge in ('0', '1') for det in ('0', '1')]

# (f) strided-batch TN, the d keys product: M = T = Td, K = Tt, N = 256, taps 1, pad_l 1; ldy = N + 4 and strideY = M ldy + 12 (the
#     record pitch and a stride that is no multiple of it), ldw = 2 N, lda = K
TS = namedtuple('TS', 'id batch M K')
TN_STRIDED_CASES = [TS('ts-b1-Td1', 1, 1, 5), TS('ts-b3-Td7', 3, 7, 37), TS('ts-b3-Td65', 3, 65, 130), TS('ts-b3-Td1', 3, 1, 37),
                    TS('ts-b1-Td65', 1, 65, 5)]
TN_STRIDED_N = 256


def scale_mul_of(c):
    return RS if c.smul == 'rs' else 1.0


def pool_fwd_label(c):
    return 'g2.pool1.%s' % ('bx' if c.bx == '1' else 'f32')


def gather_label(c):
    return 'g2.bank.S%d' % len(gather_chunks(c.F, c.K, c.S)[2])


def seam_placements(cases):
    """What the (M, T) pairs of `cases` place where, from the restated tiling: ends / starts = {local row} of the sequence ends /
    of the sequence starts in tiles with tmm > 0."""
    ends, starts, mult, nomult, t1 = set(), set(), False, False, False
    for c in cases:
        for tmm, m0, rows in tile_rows(c.M, True):
            for m in rows:
                if m % c.T == c.T - 1:
                    ends.add(m - m0)
                if m % c.T == 0 and tmm > 0:
                    starts.add(m - m0)
        mult |= (c.M - 1) % (TM - 1) == 0
        nomult |= (c.M - 1) % (TM - 1) != 0
        t1 |= c.T == 1
    return dict(ends=ends, starts=starts, mult=mult, nomult=nomult, t1=t1)


def form_labels():
    """label -> ids of the cases of this file that reach it, from the restated contracts"""
    out = {}
    for c in POOL_FWD_CASES:
        assert pool_contract(1, c.N, c.F * c.N + c.cpad, gp.host_ptr(0), gp.host_ptr(0) if c.pre else None, bias=True, act=1), c.id
        out.setdefault(pool_fwd_label(c), []).append(c.id)
    for c in POOL_BWD_CASES:
        assert pool_contract(2, c.N, c.N + c.cpad, gp.host_ptr(0), pool_x_ptr=gp.host_ptr(0)), c.id
        out.setdefault('g2.pool2', []).append(c.id)
        out.setdefault('ew.bnpool.bwd', []).append(c.id)
    for c in POOL_FWD_CASES:                        # every one also runs conv + bn_maxpool and compares the bits
        out.setdefault('ew.bnpool.fwd', []).append(c.id)
    for c in GATHER_CASES:
        taps = c.F * (c.F + 1) // 2
        assert gather_contract(c.F, c.K, taps, (c.F - 1) - (c.F - 1) // 2, c.F * c.K + c.apad) and c.N % 4 == 0, c.id
        out.setdefault(gather_label(c), []).append(c.id)
    for c, g2 in ATOMIC_CASES:
        out.setdefault('nn.atomic', []).append('%s/g2=%s' % (c.id, g2))
    for c in ROWBIAS_CASES:
        out.setdefault('nn.rowbias', []).append(c.id)
    for run in TN_GROUP_RUNS:
        out.setdefault('tn.group', []).append('%s/dbias=%d/merge=%s/det=%s' % run)
    for c in TN_STRIDED_CASES:
        out.setdefault('tn.strided', []).append(c.id)
    return out
