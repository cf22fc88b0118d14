"""What the op-level tests of the train step's glue kernels share (no GPU needed to import): fp64 references, derived bounds, a
restatement of the launch geometry of tacotron_amd/csrc/elementwise.hip, and the case lists.  The kernels are reached through the
taco_debug_* doors of include/taco_hip.h ("glue kernels"); tests/test_glue_ops_host.py proves what this module claims about its
cases, tests/test_gpu_glue_ops.py runs them.

References: plain NumPy fp64 on the fp32 operand values, one short function per op, from the kernel's header comment.  Every discrete
decision of a kernel (y > 0, pre > 0, d > 0, t < len, an id's clamp) is taken on a stored fp32 value, so the reference takes the same
one exactly and needs no flip allowance.  For sums the reference also returns n (terms summed into the element) and S (the sum of
their magnitudes), as tests/gemm_paths.py does.

Bounds (u = 2^-24, the unit roundoff of fp32; device code is compiled with contraction on, which only removes roundings):
  exact   copies, masks and signs: the embedding gather, mask_rows, zero_tail_rows, transpose_batch, mask_pos (scale 1 and 2 are
          exact factors), the L1 sign gradient, act_bwd NONE / RELU (with keep: a factor 2), and every exact-zero site.  Compared
          bitwise; a zero site must hold +0.0.
  ew_bound(k, S) = k u S   an expression of k - 1 rounded operations on terms whose magnitudes sum to S: each operation's rounding is
          at most u times the magnitude of its result, which is at most S; the k-th unit covers the second-order terms.  k per op is
          stated at its reference (K_*).
  sum_bound(n, S, c, ...) = (n + c) u S [+ prior term]   n the LONGEST chain of additions a term passes through before the fixed tree
          at the end, c the depth of that tree plus the roundings of forming one term: every addition rounds by at most u times a
          partial sum, which is at most S.  (For the column kernels n is simply the number of terms: any order is covered.)
          Accumulating onto a prior value with ONE addition adds u |prior + sum|.  With `adds` > 1 additions (fp32 atomics of several
          workgroups, in any order) each of them rounds by at most u times a running total that is at most |prior| + S, so the prior
          term is adds u (|prior| + S): the issue's form is the case adds = 1.
  norm    gn = sqrt(ss), ss within d = sum_bound / S relative: |gn - ref| <= ref (d / 2 + 3 u) (first order in d, sqrtf within one
          unit in the last place = 2 u, one more for d^2).
  Adam    adam_ref below, from the same rules, with the fp32 constants the kernel uses.
Loose by about sqrt(n) for the sums: the bounds are there for the single wrong row at a segment seam that is too small to move a
tensor norm.  No element, row or case is excluded from a comparison.
"""
import math
import zlib
from collections import namedtuple

import numpy as np

F32 = np.float32
U = 2.0 ** -24
C_TREE = 4          # the four row lanes (or four waves) added in a fixed order at the end of a column kernel / block_sum of 256 threads
RS32 = F32(1.0) / np.sqrt(F32(1.0) + F32(1e-3))      # 1.0f / sqrtf(1.0f + kBnEps): three correctly rounded fp32 operations
K_RS = 3            # ... whose results are within 3 u of 1 / sqrt(1.001)
LOSS_PARTS, SUMSQ_PARTS, MAX_TRANSPOSE_BATCH = 512, 256, 96
EMB_PASS, EMB_MAX_SEGS = 4096, 32
ACTS = ('none', 'relu', 'sigmoid', 'tanh')


def seed_of(case_id):
    return zlib.crc32(str(case_id).encode())


def rng_of(case_id):
    return np.random.default_rng(seed_of(case_id))


def ew_bound(k, S):
    return k * U * np.asarray(S, np.float64)


def sum_bound(n, S, c, prior=None, total=None, adds=1):
    b = (np.asarray(n, np.float64) + c) * U * np.asarray(S, np.float64)
    if prior is not None:
        b = b + (U * np.abs(total) if adds == 1 else adds * U * (np.abs(prior) + S))
    return b


def norm_bound(ref_norm, rel_ss):
    return ref_norm * (0.5 * rel_ss + 3 * U)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def plant_zeros(a, rng, every=7):
    """+0.0 and -0.0 at fixed strides of the flattened array (in place), so that every `> 0` test meets both"""
    f = a.reshape(-1)
    f[0::every] = 0.0
    f[3::2 * every] = -0.0
    return a


# ------------------------------------------------------------------------------------------------------------------
# launch geometry restated (launch_embedding_bwd, col_grid, launch_center_rows, launch_l1, launch_sumsq)

def emb_geometry(rows, det):
    """-> dict(segs, rps, seams, passes (per segment), pass_seams): launch_embedding_bwd + the list passes of the kernel"""
    segs = 1 if det else max(1, min(EMB_MAX_SEGS, (rows + 255) // 256))
    rps = (rows + segs - 1) // segs
    spans = [(k * rps, min(rows, (k + 1) * rps)) for k in range(segs)]
    passes = [max(0, -(-(b - a) // EMB_PASS)) for a, b in spans]
    pass_seams = [a + j * EMB_PASS for a, b in spans for j in range(1, -(-(b - a) // EMB_PASS)) if a < b]
    return dict(segs=segs, rps=rps, seams=[a for a, b in spans[1:] if a < rows], passes=passes, pass_seams=pass_seams)


def emb_labels(rows, det):
    g = emb_geometry(rows, det)
    seg = 'seg1' if g['segs'] == 1 else 'segN'
    out = {'emb.%s.pass%s' % (seg, '1' if max(g['passes']) == 1 else 'N')}
    if max(g['passes']) >= 3:
        out.add('emb.pass3')
    return out


def col_geometry(M, det):
    """col_grid -> dict(chunks = grid.y, rpb = rows per block, lane_rows = the most rows one row lane adds)"""
    chunks = min(2048, (M + 31) // 32)
    if det:
        chunks = 1
    chunks = max(chunks, 1)
    rpb = (M + chunks - 1) // chunks
    gy = (M + rpb - 1) // rpb
    return dict(chunks=gy, rpb=rpb, lane_rows=(min(rpb, M) + 3) // 4, ragged=M % rpb != 0)


def col_labels(M, det):
    g = col_geometry(M, det)
    if g['chunks'] == 1:
        return {'col.chunk1'}
    return {'col.chunkN.ragged' if g['ragged'] else 'col.chunkN'}


def center_geometry(T, C):
    per = (T + 3) // 4
    quarters = [(z * per, min(T, z * per + per)) for z in range(4)]
    return dict(per=per, quarters=quarters, empty=sum(1 for a, b in quarters if a >= b), inactive_quads=(-(C // 4)) % 64)


def center_labels(T, C):
    g = center_geometry(T, C)
    return {'center.quarter-empty' if g['empty'] else 'center.quarters-full', 'center.inactive-quads' if g['inactive_quads'] else 'center.all-quads'}


def l1_geometry(M, N, ldg):
    """launch_l1: 512 blocks of 16 waves, one wave per row at a time, rows walked in 256-wide pieces up to ldg"""
    nwaves = LOSS_PARTS * 16
    return dict(rows_per_wave=-(-M // nwaves), busy_blocks=min(LOSS_PARTS, -(-M // 16)), pieces=-(-ldg // 256), lane_terms=-(-M // nwaves) * 4 * -(-ldg // 256))


def l1_labels(M, N, ldg):
    g = l1_geometry(M, N, ldg)
    return {'l1.wave-multirow' if g['rows_per_wave'] > 1 else 'l1.wave-onerow', 'l1.idle-blocks' if g['busy_blocks'] < LOSS_PARTS else 'l1.all-blocks',
            'l1.pad-cols' if ldg > N else 'l1.dense'}


# depth of the fixed trees behind a lane's own chain: |a - b| itself (1), wave_sum (6), the 16 waves of a block in sequence (16);
# finish_loss: two partials per thread (2), wave_sum (6), four waves (4); loss[0] = loss[1] + loss[2] (1)
C_L1_TERM = 1 + 6 + 16 + 2 + 6 + 4
C_L1_TOTAL = C_L1_TERM + 1


def sumsq_geometry(n):
    """launch_sumsq: 256 blocks of 256 threads over n // 4 float4: thread i runs the 4-way unrolled loop while i + 3 stride < n4, then
    the remainder loop; the n % 4 scalars are added by block 0.  -> float4 counts per loop form and the longest chain"""
    stride, n4 = SUMSQ_PARTS * 256, n // 4
    i = np.arange(stride, dtype=np.int64)
    u = np.maximum(0, -(-(n4 - 3 * stride - i) // (4 * stride)))          # unrolled iterations of thread i
    r = np.maximum(0, -(-(n4 - (i + 4 * stride * u)) // stride))          # remainder iterations behind them
    unrolled, rem, both, chain = int(u.max()), int(r.max()), int(np.minimum(u, r).max()), int((u + r).max())
    return dict(n4=n4, unrolled=unrolled, rem=rem, both=both, tail=n - 4 * n4, chain=chain)


def sumsq_labels(n):
    g = sumsq_geometry(n)
    if g['n4'] == 0:
        return {'sumsq.tail-only'}
    form = 'unroll+rem' if g['both'] else 'unroll' if g['unrolled'] else 'rem'
    return {'sumsq.%s%s' % (form, '+tail' if g['tail'] else '')}


# a float4's four products and three additions (7, contraction only removes some), (a1 + a2) + a3 and acc += (2), the tail element (1),
# wave_sum (6), four waves (4)
C_SUMSQ = 7 + 2 + 1 + 6 + 4
C_NORM = C_SUMSQ + 1 + 6 + 4        # clip_adam_kernel: one partial per thread (1), wave_sum (6), four waves (4)

GEOMETRY_LABELS = {'emb.seg1.pass1', 'emb.seg1.passN', 'emb.segN.pass1', 'emb.segN.passN', 'emb.pass3', 'col.chunk1', 'col.chunkN', 'col.chunkN.ragged',
                   'center.quarter-empty', 'center.quarters-full', 'center.inactive-quads', 'center.all-quads', 'l1.wave-multirow', 'l1.wave-onerow',
                   'l1.idle-blocks', 'l1.all-blocks', 'l1.pad-cols', 'l1.dense', 'sumsq.tail-only', 'sumsq.rem', 'sumsq.rem+tail', 'sumsq.unroll+tail',
                   'sumsq.unroll+rem+tail'}


# ------------------------------------------------------------------------------------------------------------------
# references

def clamp_ids(ids, V):
    return np.clip(np.asarray(ids, np.int64), 0, V - 1)


def embedding_ref(table, ids):
    return np.asarray(table)[clamp_ids(ids, len(table))]


def embedding_bwd_ref(dout, ids, prior, geo=None):
    """-> (prior + sum, sum, n (V, 1), S (V, width)).  n is the number of rows of an id; with `geo` (emb_geometry) it is the longest chain
    of additions instead: a row lane of workgroup (v, segment) adds every fourth listed row of each list pass, at most
    ceil(rows of v in the segment / 4) + passes terms, which is far below the row count where one id owns most rows -- the bound
    then still sees ONE row lost at a seam.  (Behind the chain: the other three lanes, C_EMB = 3, then the segment's one addition
    onto the table row: sum_bound's prior term with adds = segments.)"""
    V = len(prior)
    d = np.asarray(dout, np.float64)
    cid = clamp_ids(ids, V)
    tot, S = np.zeros(prior.shape), np.zeros(prior.shape)
    np.add.at(tot, cid, d)
    np.add.at(S, cid, np.abs(d))
    n = np.bincount(cid, minlength=V).astype(np.float64)
    if geo is not None:
        spans = [(k * geo['rps'], min(len(cid), (k + 1) * geo['rps'])) for k in range(geo['segs'])]
        chain = [np.ceil(np.bincount(cid[a:b], minlength=V) / 4) + p for (a, b), p in zip(spans, geo['passes'])]
        n = np.where(n > 0, np.max(chain, axis=0), 0.0)
    return prior.astype(np.float64) + tot, tot, n[:, None], S


C_EMB = 3


K_HW_Y, K_HW_DT, K_HW_DH, K_HW_DX = 5, 6, 2, 3


def highway_ref(th, x):
    """th (M, 256) = [T | H]: y = H T + x (1 - T): four operations -> K_HW_Y = 5 on S = |H T| + |x| (1 + |T|)"""
    th, x = np.asarray(th, np.float64), np.asarray(x, np.float64)
    t, h = th[:, :128], th[:, 128:]
    return h * t + x * (1 - t), np.abs(h * t) + np.abs(x) * (1 + np.abs(t))


def highway_bwd_ref(th, x, dy):
    """-> dict: dt = dy (H - x) T (1 - T) (five operations), dh = H > 0 ? dy T : 0 (one), dx = dy (1 - T) (two), their S, and `zero`, the
    dh sites that must be exactly 0"""
    th, x, g = np.asarray(th, np.float64), np.asarray(x, np.float64), np.asarray(dy, np.float64)
    t, h = th[:, :128], th[:, 128:]
    pos = h > 0
    return dict(dt=g * (h - x) * t * (1 - t), S_dt=np.abs(g) * (np.abs(h) + np.abs(x)) * np.abs(t) * (1 + np.abs(t)),
                dh=np.where(pos, g * t, 0.0), S_dh=np.abs(g * t), zero=~pos, dx=g * (1 - t), S_dx=np.abs(g) * (1 + np.abs(t)))


K_ACT = {'none': 0, 'relu': 0, 'sigmoid': 4, 'tanh': 4}       # 0: bit-exact; sigmoid / tanh: three operations


def act_bwd_ref(y, dy, keep, act):
    """-> (dz, S, zero): dz = dy act'(y) against the stored OUTPUT y; keep: a factor 2 or exactly 0"""
    y, g = np.asarray(y, np.float64), np.asarray(dy, np.float64)
    zero = np.zeros(y.shape, bool)
    if act == 'none':
        dz, S = g, np.abs(g)
    elif act == 'relu':
        zero = ~(y > 0)
        dz, S = np.where(zero, 0.0, g), np.abs(g)
    elif act == 'sigmoid':
        dz, S = g * y * (1 - y), np.abs(g * y) * (1 + np.abs(y))
    else:
        dz, S = g * (1 - y * y), np.abs(g) * (1 + y * y)
    if keep is not None:
        k = np.asarray(keep) != 0
        zero = zero | ~k
        dz, S = np.where(k, 2 * dz, 0.0), 2 * S
    return dz, S, zero


K_AFF_DZ = K_RS + 3          # rs, gamma rs, dy s
C_AFF_G = C_TREE + K_RS + 2  # a dgamma term is dy pre rs: two products and rs


def affine_act_bwd_ref(pre, gamma, dy, act, prior_g, prior_b):
    """pre, dy (M, N): dgamma = prior + sum_m dy pre rs, dbeta = prior + sum_m dy, dz = dy gamma rs, 0 where relu and !(pre > 0)"""
    p, g, gm = np.asarray(pre, np.float64), np.asarray(dy, np.float64), np.asarray(gamma, np.float64)
    rs = 1.0 / math.sqrt(1.0 + 1e-3)
    zero = ~(p > 0) if act == 'relu' else np.zeros(p.shape, bool)
    sg, sb = (g * p * rs).sum(0), g.sum(0)
    return dict(dz=np.where(zero, 0.0, g * gm * rs), S_dz=np.abs(g * gm * rs), zero=zero, sum_g=sg, sum_b=sb, dgamma=prior_g + sg, dbeta=prior_b + sb,
                S_g=np.abs(g * p * rs).sum(0), S_b=np.abs(g).sum(0), n=float(len(p)))


def colsum_ref(x, B, T, N):
    """x ((B T), ld) -> (out (B, N), S)"""
    v = np.asarray(x, np.float64)[:, :N].reshape(B, T, N)
    return v.sum(1), np.abs(v).sum(1)


def row_mask(length, B, T, lo=None):
    n = np.asarray(length, np.int64)
    if lo is not None:
        n = np.clip(n, lo, T)
    return np.arange(T)[None, :] < n[:, None]


def mask_rows_ref(x, length):
    B, T, _ = x.shape
    return np.where(row_mask(length, B, T)[:, :, None], x, F32(0))


def center_rows_ref(x, length):
    """-> (out, bound, zero): n = clamp(len, 1, T); out[b, s] = x - mean over s' < n for s < n, else exactly 0.  The mean is a column sum
    whose longest chain is a row lane's ceil(n / 4) terms, then the other three lanes, times the rounded 1 / n (two more roundings):
    sum_bound(ceil(n / 4), S, 3 + 2) / n; the subtraction rounds by u (|x| + |mean|)"""
    B, T, _ = x.shape
    live = row_mask(length, B, T, lo=1)[:, :, None]
    n = live.sum(1, keepdims=True).astype(np.float64)
    v = np.asarray(x, np.float64)
    mean = (v * live).sum(1, keepdims=True) / n
    S = (np.abs(v) * live).sum(1, keepdims=True)
    out = np.where(live, v - mean, 0.0)
    bound = np.where(live, sum_bound(np.ceil(n / 4), S, 3 + 2) / n + U * (np.abs(v) + np.abs(mean)), 0.0)
    return out, bound, ~np.broadcast_to(live, x.shape)


def mask_pos_ref(g, y, scale):
    """scale 1 and 2: exact"""
    return np.where(np.asarray(y) > 0, F32(scale) * np.asarray(g, F32), F32(0))


def zero_tail_ref(x, length):
    B, Td, _ = x.shape
    return np.where(row_mask(length, B, Td)[:, :, None], x, F32(0))


def l1_ref(a, b):
    """-> (sum |a - b|, sign(a - b) as fp32 with +0.0 at ties)"""
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return np.abs(d).sum(), np.sign(d).astype(F32) + F32(0)


def l1_bounds(terms):
    """terms: [(S_i, l1_geometry_i) or None] * 2 -> bounds of (loss[0], loss[1], loss[2])"""
    each = [0.0 if t is None else sum_bound(t[1]['lane_terms'], t[0], C_L1_TERM) for t in terms]
    S = sum(0.0 if t is None else t[0] for t in terms)
    n = max(0 if t is None else t[1]['lane_terms'] for t in terms)
    return sum_bound(n, S, C_L1_TOTAL), each[0], each[1]


def transpose_ref(src):
    """src (taps, K, N) -> (taps, N, K), tap order reversed"""
    return np.ascontiguousarray(np.asarray(src)[::-1].transpose(0, 2, 1))


def sumsq_ref(x):
    """-> (ss, relative bound of the ordered sum of the 256 partials' total): every term is positive, S = ss"""
    v = np.asarray(x, np.float64)
    return float((v * v).sum()), (sumsq_geometry(len(v))['chain'] + C_SUMSQ) * U


def host_lr_t(lr, step):
    """launch_clip_adam: the bias-corrected rate in double, handed to the kernel as a float"""
    return F32(float(lr) * math.sqrt(1.0 - 0.999 ** float(step)) / (1.0 - 0.9 ** float(step)))


def adam_ref(p, g, m, v, lr, cap, step):
    """One clip + Adam step in fp64 on the fp32 values the kernel uses: 0.9f, 1 - 0.9f, 0.999f, 1 - 0.999f (both differences are exact
    in fp32), 1e-8f, the host's (float) lr_t.  -> dict(gn, p, m, v) and their bounds:
      e_g   relative error of gi = g scale: 0 where scale is exactly 1 (cap <= 0, or gn < cap: cap / cap); else the norm's (d / 2 + 3 u),
            the division and the product (2 u)
      m     b1 m + (1 - b1) gi: three operations                    (3 + 1) u S_m + e_g |(1 - b1) gi|
      v     b2 v + ((1 - b2) gi) gi: four operations               (4 + 1) u S_v + 2 e_g |(1 - b2) gi^2|;  S_v = v' (all terms >= 0)
      p     p - lr_t m' / (sqrt(v') + eps): D = sqrt(v') + eps is within e_D = e_v / 2 + 2 u (sqrtf) + u (the sum) relative, with e_v =
            bound_v / v'; the quotient Q = lr_t m' / D rounds twice more (the division within 2 u):
            bound_p = (lr_t / D) (bound_m + |m'| (e_D + 3 u)) + u (|p| + |Q|) + u |p'|"""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    b1, b2, eps = float(F32(0.9)), float(F32(0.999)), float(F32(1e-8))
    c1, c2 = float(F32(1) - F32(0.9)), float(F32(1) - F32(0.999))
    lr_t = float(host_lr_t(lr, step))
    ss, rel_ss = sumsq_ref(g)
    rel_ss = rel_ss + (1 + 6 + 4) * U
    gn = math.sqrt(ss)
    clipped = cap > 0 and gn > cap
    scale = cap / gn if clipped else 1.0
    e_g = (0.5 * rel_ss + 3 * U + 2 * U) if clipped else 0.0
    gi = g * scale
    m1, v1 = b1 * m + c1 * gi, b2 * v + c2 * gi * gi
    bm = 4 * U * (np.abs(b1 * m) + np.abs(c1 * gi)) + e_g * np.abs(c1 * gi)
    bv = 5 * U * v1 + 2 * e_g * c2 * gi * gi
    D = np.sqrt(v1) + eps
    e_D = 0.5 * bv / np.maximum(v1, 1e-300) + 3 * U
    Q = lr_t * m1 / D
    p1 = p - Q
    bp = lr_t / D * (bm + np.abs(m1) * (e_D + 3 * U)) + U * (np.abs(p) + np.abs(Q)) + U * np.abs(p1)
    return dict(gn=gn, b_gn=norm_bound(gn, rel_ss), clipped=clipped, p=p1, m=m1, v=v1, b_p=bp, b_m=bm, b_v=bv)


# ------------------------------------------------------------------------------------------------------------------
# cases

EmbCase = namedtuple('EmbCase', 'id V width rows pattern det')
_E = lambda V, w, rows, pat, det=False: EmbCase('emb-V%d-w%d-r%d-%s%s' % (V, w, rows, pat, '-det' if det else ''), V, w, rows, pat, det)
EMB_BIG_ROWS = 131073 + 5
EMB_CASES = [_E(1, 16, 1, 'one'), _E(1, 260, 257, 'mixed'), _E(33, 16, 255, 'mixed'), _E(33, 256, 256, 'pad90'), _E(33, 256, 257, 'mixed'),
             _E(33, 260, 1000, 'pad90'), _E(33, 1024, 1000, 'one'), _E(33, 1024, 257, 'mixed'), _E(33, 16, 1000, 'mixed'), _E(33, 256, 1, 'one'),
             _E(33, 16, EMB_BIG_ROWS, 'pad90'),
             _E(33, 256, 4096, 'pad90', True), _E(33, 260, 4097, 'mixed', True), _E(33, 16, 8200, 'pad90', True), _E(1, 1024, 4097, 'mixed', True),
             _E(33, 256, 257, 'mixed', True)]
EMB_NEVER = lambda V: V - 2          # the id no row of a 'pad90' / 'mixed' case carries (V > 1)
EMB_ONE = lambda V: min(5, V - 1)
EMB_SEAM = lambda V: min(1, V - 1)


def emb_ids(c):
    """int32 ids of a case.  'one': every row EMB_ONE.  'mixed': uniform over [0, V) without EMB_NEVER.  'pad90': the same with 90 % of
    the rows set to 0.  'mixed' and 'pad90' rows 1 (mod 97) hold -3 and rows 2 (mod 97) hold V + 5 (clamped to 0 and V - 1, as in the
    forward gather).  Both rows at every segment seam and at every list-pass seam hold EMB_SEAM, an id few other rows carry: a row lost
    or doubled at a seam changes a table row that both sides add to, by far more than the bound of that row's short sum"""
    rng = rng_of(c.id)
    if c.pattern == 'one':
        return np.full(c.rows, EMB_ONE(c.V), np.int32)
    ids = rng.integers(0, c.V, c.rows)
    if c.V > 1:
        ids[ids == EMB_NEVER(c.V)] = 0
    if c.pattern == 'pad90':
        ids[rng.random(c.rows) < 0.9] = 0
    ids[1::97], ids[2::97] = -3, c.V + 5
    g = emb_geometry(c.rows, c.det)
    for s in g['seams'] + g['pass_seams']:
        ids[s - 1] = ids[s] = EMB_SEAM(c.V)
    return ids.astype(np.int32)


HIGHWAY_M = (1, 33, 4097)


def highway_operands(M):
    """th (M, 256), x, dy (M, 128).  Columns 0 / 1: gate exactly 0 / 1; columns 2, 3: candidate +0.0 / -0.0 (gate and dy non-zero there);
    column 4: both 0; every 7th candidate of the rest is +-0 as well"""
    rng = rng_of('highway-%d' % M)
    t = rng.uniform(0.05, 0.95, (M, 128)).astype(F32)
    h = plant_zeros(rng.standard_normal((M, 128)).astype(F32), rng)
    h[:, 0:2] = rng.standard_normal((M, 2)).astype(F32) + F32(3)
    t[:, 0], t[:, 1], h[:, 2], h[:, 3], t[:, 4], h[:, 4] = 0.0, 1.0, 0.0, -0.0, 0.0, 0.0
    x, dy = rng.standard_normal((M, 128)).astype(F32), rng.standard_normal((M, 128)).astype(F32)
    dy[dy == 0] = 1.0
    return np.concatenate([t, h], 1), x, dy


ActCase = namedtuple('ActCase', 'id n act keep inplace')
ACT_BIG = (1 << 20) + 3
ACT_CASES = [ActCase('act-%s-n%d%s%s' % (a, n, '-keep' if k else '', '-inplace' if ip else ''), n, a, k, ip)
             for n in (1, 1001) for a in ACTS for k in (False, True) for ip in (False, True)]
ACT_CASES += [ActCase('act-%s-n%d%s%s' % (a, ACT_BIG, '-keep' if k else '', '-inplace' if ip else ''), ACT_BIG, a, k, ip)
              for a in ACTS for k, ip in ((False, True), (True, False))]


def act_operands(c):
    rng = rng_of(c.id)
    y = plant_zeros((0.7 * rng.standard_normal(c.n)).astype(F32), rng) if c.n > 1 else np.array([0.4], F32)
    dy = rng.standard_normal(c.n).astype(F32)
    dy[dy == 0] = 1.0
    keep = (rng.random(c.n) < 0.5).astype(np.uint8) if c.keep else None
    if c.keep and c.n == 1:
        keep[0] = 1
    return y, dy, keep


AffCase = namedtuple('AffCase', 'id M N act det')
AFF_CASES = [AffCase('aff-M%d-N%d-%s%s' % (M, N, a, '-det' if d else ''), M, N, a, d)
             for N in (80, 128, 132, 256) for M in (1, 31, 33, 129, 1000) for a in ('none', 'relu') for d in ((False, True) if M in (33, 1000) else (False,))]
AFF_CASES += [AffCase('aff-M64-N128-%s' % a, 64, 128, a, False) for a in ('none', 'relu')]      # two chunks of exactly 32 rows


def aff_operands(c):
    rng = rng_of(c.id)
    pre = plant_zeros(rng.standard_normal((c.M, c.N)).astype(F32), rng)
    dy = rng.standard_normal((c.M, c.N)).astype(F32)
    dy[dy == 0] = 1.0
    gamma = (1 + 0.3 * rng.standard_normal(c.N)).astype(F32)
    return pre, gamma, dy, rng.standard_normal(c.N).astype(F32), rng.standard_normal(c.N).astype(F32)


ColCase = namedtuple('ColCase', 'id B T N ld')
COLSUM_CASES = [ColCase('col-B%d-T%d-N%d-ld%d' % a, *a) for a in
                ((1, 5, 512, 512), (1, 32, 256, 256), (3, 1, 16, 16), (2, 3, 80, 84), (4, 4, 130, 130), (2, 5, 130, 200), (3, 41, 80, 80), (2, 41, 16, 20))]

RowCase = namedtuple('RowCase', 'id T C')
ROW_CASES = [RowCase('rows-T%d-C%d' % (T, C), T, C) for T in (1, 2, 3, 5, 37) for C in (256, 260, 512)]
ROW_B = 6
ROW_BIG_MEAN = (3, 4)        # batch rows whose columns carry a common component of 1e3 under a spread of 1e-2


def row_lengths(T):
    return np.array([-1, 0, 1, T - 1, T, T + 3], np.int32)


def row_operands(c):
    rng = rng_of(c.id)
    x = rng.standard_normal((ROW_B, c.T, c.C)).astype(F32)
    for b in ROW_BIG_MEAN:
        x[b] = (1e3 * np.where(rng.random((1, c.C)) < 0.5, 1.0, -1.0) + 1e-2 * rng.standard_normal((c.T, c.C))).astype(F32)
    return x, row_lengths(c.T)


PosCase = namedtuple('PosCase', 'id rows cols ldg ldy scale')
MASK_POS_CASES = [PosCase('pos-r%d-c%d-g%d-y%d-s%d' % a, *a) for a in
                  ((1, 1, 1, 1, 1), (33, 128, 384, 256, 2), (257, 100, 104, 300, 2), (1000, 128, 132, 256, 1), (5, 256, 256, 256, 2))]

TailCase = namedtuple('TailCase', 'id C0 C1')
ZERO_TAIL_CASES = [TailCase('tail-C%d-%s' % (a, b or 'none'), a, b) for a, b in ((160, None), (160, 2050), (2050, 160), (2050, None))]
TAIL_TD = 7
TAIL_LEN = np.array([0, 1, TAIL_TD, TAIL_TD + 4, TAIL_TD - 1], np.int32)

L1Case = namedtuple('L1Case', 'id terms')          # terms: two of None | (M, N, ldg, grad?)
_L1_SHAPES = ((1, 1025, 1028), (37, 1025, 1028), (37, 160, 160), (9001, 5, 8), (3, 400, 400))
L1_CASES = [L1Case('l1-%dx%d-ld%d-%s-slot%d' % (M, N, ld, 'grad' if g else 'nograd', (i + g) % 2),
                   tuple((M, N, ld, g) if s == (i + g) % 2 else None for s in (0, 1)))
            for i, (M, N, ld) in enumerate(_L1_SHAPES) for g in (True, False)]
L1_CASES.append(L1Case('l1-model-pair', ((37, 160, 160, True), (37, 1025, 1028, True))))


def l1_operands(case_id, slot, M, N):
    """a, b (M, N): b = a at every 5th element (ties); a = +0.0, b = -0.0 at every 11th and the other way round at every 13th"""
    rng = rng_of('%s-%d' % (case_id, slot))
    a, b = rng.standard_normal(M * N).astype(F32), rng.standard_normal(M * N).astype(F32)
    b[::5] = a[::5]
    a[::11], b[::11] = 0.0, -0.0
    a[::13], b[::13] = -0.0, 0.0
    return a.reshape(M, N), b.reshape(M, N)


TrJob = namedtuple('TrJob', 'taps K N ldi ldo')
_TR_KINDS = (TrJob(3, 1, 1, 0, 0), TrJob(1, 31, 33, 0, 0), TrJob(3, 31, 33, 0, 0), TrJob(1, 80, 1025, 1028, 84), TrJob(3, 256, 128, 0, 0),
             TrJob(1, 256, 128, 132, 260), TrJob(1, 1, 1, 5, 3), TrJob(3, 80, 1025, 0, 0))
TRANSPOSE_CASES = {'tr-one-3x31x33': [_TR_KINDS[2]], 'tr-one-1x1x1': [TrJob(1, 1, 1, 0, 0)], 'tr-one-pitched-80x1025': [_TR_KINDS[3]],
                   'tr-one-3x256x128': [_TR_KINDS[4]], 'tr-batch-96': [_TR_KINDS[i % len(_TR_KINDS)] for i in range(MAX_TRANSPOSE_BATCH)]}

SUMSQ_N = (1, 3, 4, 5, 100003, 4 * 196607 + 3, 4 * 196609 + 1, 4 * 262145 + 2)

AdamCase = namedtuple('AdamCase', 'id n mode step')      # mode: off (cap <= 0) | below | above | zero (an all-zero gradient)
ADAM_CAP, ADAM_LR = 5.0, 5e-4
ADAM_CASES = [AdamCase('adam-n%d-%s-step%d' % a, *a) for a in
              ((1, 'above', 1), (3, 'below', 2), (4, 'off', 100000), (5, 'above', 100000), (100003, 'above', 1), (100003, 'below', 2),
               (100003, 'zero', 1), (100003, 'off', 2), (4 * 196609 + 1, 'above', 2), (4 * 262145 + 2, 'below', 100000))]


def adam_operands(c):
    """p, g, m, v; the gradient's norm is a factor 8 below or above the cap (no decision near it)"""
    rng = rng_of(c.id)
    p, g = rng.standard_normal(c.n).astype(F32), rng.standard_normal(c.n)
    m, v = (0.1 * rng.standard_normal(c.n)).astype(F32), (0.01 * rng.random(c.n)).astype(F32)
    target = {'off': 40.0, 'below': ADAM_CAP / 8, 'above': ADAM_CAP * 8, 'zero': 0.0}[c.mode]
    g = (g * (target / max(np.linalg.norm(g), 1e-30))).astype(F32)
    return p, g, m, v, (0.0 if c.mode == 'off' else ADAM_CAP)
