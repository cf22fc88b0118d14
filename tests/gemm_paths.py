"""What the op-level GEMM path tests share (no GPU needed to import): fp64 references with error scales, a Python
restatement of the launchers' dispatch predicates, and the enumerated case lists.

References
  nn_ref   C = post(act(sum_tap shift_tap(A) . W[tap] + bias)) as gemm.hip's header states it, with the pre-affine copy Cpre
           and S[m, n] = sum |a| |w| + |bias| over the same terms (the scale of the accumulation's rounding error).
           `conv_ref` -- the (C, Cpre) pair every GEMM test of tests/test_gpu_ops.py compares with -- is this function.
  tn_ref   dW[tap] = shift_tap(A)^T . dY and its S.

Restated dispatch (tacotron_amd/csrc; the GPU tests hand in real data_ptr() values, the host tests 256-byte aligned ones)
  nn_flags         gemm.hip  conv_gemm_set_flags                      (bit 0: A operand, bit 1: W operand)
  nn_tile          gemm.hip  launch_conv_gemm_batch, `work >= 384`    (one problem per launch)
  gemm2_takes      gemm.hip  launch_conv_gemm_batch `flags == 3` + gemm2.hip launch_conv_gemm2 / dma_contract (tiles >= min)
  gemm2_form       gemm2.hip launch_conv_gemm2, `env_bf16x() && chain <= bf16x_max_chain()`
  gemm2_epilogue   gemm2.hip launch_conv_gemm2, `vec` / `shifted` (flag bits 2 and 3), else the scalar stores
  ksplit_plan      gemm.hip  launch_conv_gemm_tapsplit: maxS, the makespan model, TACO_KSPLIT, `per`, the chunks [it0, it1)
  tn_plan          gemm.hip  plan_gemm_tn (flags, merge_taps, tile rule, splits / chunk) + dispatch_tn (bf16x3 or fp32 on flags 3)
The defaults of the switches these read are those of tacotron_amd/csrc/switches.def.

Path labels (PATH_TABLE; tests/test_gemm_paths_host.py requires the case lists to reach every one)
  nn.t64.f0 .. nn.t128.f3      conv_gemm_kernel<1,1,VA,VW> / <2,2,VA,VW> of gemm.hip, f = the flags
  g2.{f32,bx}.{vec,shifted,scalar}   conv_gemm2_kernel's MFMA form and epilogue form
  ksplit.S2 / S3 / S5          the k-split launch with the S that really runs
  tn.t64.* / tn.t128.*         gemm_tn_kernel<1,1,..> / <2,2,..>: f3.bx, f3.f32, f1, f2, f0
  g2.pool1.* g2.pool2 ew.bnpool.* g2.bank.S* nn.atomic nn.rowbias tn.group tn.strided   see tests/gemm_forms.py

The forms only the model's own launches build -- bias_stride, atomic_out, scale_mul, pool, bank_filters, the grouped TN launch and
strideA / strideY / strideW -- have their references, contracts, labels and case lists in tests/gemm_forms.py (through the debug
doors of include/taco_hip.h); their labels are part of PATH_TABLE below.  Still reached by the model-level tests only: the conv-bank
XCD order of gemm2.hip (xcd_map == 2), which needs a batch of 8 or 16 problems with equal tile counts -- a tile ORDER, not a form:
it changes which workgroup computes a tile, not what the tile holds.
"""
import zlib
from collections import namedtuple

import numpy as np

from oracle import taco_numpy as on

# ------------------------------------------------------------------------------------------------------------------
# references


def _shifted(A, T, sh):
    """rows of A (M, K), M = B * T, moved by `sh` inside their own sequence; rows pulled from outside it are zeros"""
    M, K = A.shape
    x = A.reshape(M // T, T, K)
    out = np.zeros_like(x)
    lo, hi = max(0, -sh), min(T, T - sh)
    if hi > lo:
        out[:, lo:hi] = x[:, lo + sh:hi + sh]
    return out.reshape(M, K)


def nn_ref(A, W, bias, T, pad_l, act, keep=None, scale=None, shift=None, residual=None):
    """A (M, K) with M = B * T; W (taps, K, N).  Returns (C, Cpre, S) in fp64.  `scale` and `shift` are independent: either
    alone is legal (the kernels test `P.scale || P.shift`)."""
    A, W = np.asarray(A, np.float64), np.asarray(W, np.float64)
    M, K = A.shape
    taps, _, N = W.shape
    y, S = np.zeros((M, N)), np.zeros((M, N))
    for j in range(taps):
        a = _shifted(A, T, j - pad_l)
        y += a @ W[j]
        S += np.abs(a) @ np.abs(W[j])
    if bias is not None:
        y = y + bias
        S = S + np.abs(bias)
    if act == 1:
        y = np.maximum(y, 0)
    elif act == 2:
        y = on.sigmoid(y)
    elif act == 3:
        y = np.tanh(y)
    if keep is not None:
        y = y * (np.asarray(keep) != 0) * 2
    pre = y.copy()
    if scale is not None or shift is not None:
        y = y * (scale if scale is not None else 1.0) + (shift if shift is not None else 0.0)
    if residual is not None:
        y = y + residual
    return y, pre, S


def conv_ref(A, W, bias, T, pad_l, act, keep=None, scale=None, shift=None, residual=None):
    return nn_ref(A, W, bias, T, pad_l, act, keep, scale, shift, residual)[:2]


def tn_ref(A, dY, taps, T, pad_l):
    """A (M, K), dY (M, N) -> (dW (taps, K, N), S) with S = sum_m |a| |dy| over the same terms."""
    A, dY = np.asarray(A, np.float64), np.asarray(dY, np.float64)
    K, N = A.shape[1], dY.shape[1]
    dW, S = np.zeros((taps, K, N)), np.zeros((taps, K, N))
    for j in range(taps):
        a = _shifted(A, T, j - pad_l)
        dW[j] = a.T @ dY
        S[j] = np.abs(a).T @ np.abs(dY)
    return dW, S


def element_bound(n, S, g, ref):
    """|got - ref| <= (n + 16) 2^-23 S g + 8 * 2^-24 |ref|: one unit in the last place of the running sum per accumulated product
    in any order (the matrix pipe rounds every product onto the accumulator's grid), 2^-23 per product for the three plane
    products the bf16x3 form drops (m l, l m, l l <= 2^-24 |a| |w| each), a few units for the device tanh / sigmoid; g is the
    Lipschitz factor of what follows the sum (2 with keep, |scale|; 1 for the activations).  Derived, not measured, and loose by
    about sqrt(n): it is there for the single wrong element that is too small to move a tensor norm."""
    return (n + 16) * 2.0 ** -23 * S * g + 8 * 2.0 ** -24 * np.abs(ref)


def seed_of(case_id):
    return zlib.crc32(case_id.encode()) & 0x7fffffff


# ------------------------------------------------------------------------------------------------------------------
# dispatch restatement

GEMM2_MIN_TILES = 160       # switches.def defaults
BF16X_MAX_CHAIN = 2048
TN_BLOCKS = 3072
TN_BIG_TILES = 128
MAX_GEMM_BATCH = 16         # kernels.h kMaxGemmBatch


def cdiv(a, b):
    return -(-a // b)


def nn_flags(a_ptr, lda, w_ptr, ldw, N, K, nld=0):
    nld = nld if nld > 0 else (N if N % 4 == 0 else 0)
    f = 0
    if lda % 4 == 0 and a_ptr % 16 == 0 and K % 4 == 0:
        f |= 1
    if ldw % 4 == 0 and w_ptr % 16 == 0 and (K * ldw) % 4 == 0 and nld > 0 and nld % 4 == 0 and nld <= ldw:
        f |= 2
    return f


def nn_tile(M, N):
    return 128 if cdiv(M, 128) * cdiv(N, 128) >= 384 else 64


def gemm2_takes(flags, M, N, K, taps, lda, ldw, min_tiles=GEMM2_MIN_TILES, force=False):
    if flags != 3 or min_tiles <= 0:
        return False
    lim = 1 << 31
    if not ((M + taps + 1) * lda * 4 + K * 4 < lim and (taps * K + 32) * ldw * 4 < lim):
        return False
    return cdiv(M, 128) * cdiv(N, 128) >= (1 if force else min_tiles)


def gemm2_form(bf16x, chain):
    return 'bx' if bf16x and chain <= BF16X_MAX_CHAIN else 'f32'


def gemm2_epilogue(c_ptr, ldc, N, cpre_ptr=None, res_ptr=None, ldr=0, keep_ptr=None):
    """None = the option is off (a null pointer)"""
    vec = (N % 4 == 0 and ldc % 4 == 0 and c_ptr % 16 == 0 and (cpre_ptr is None or cpre_ptr % 16 == 0) and
           (res_ptr is None or (ldr % 4 == 0 and res_ptr % 16 == 0)) and (keep_ptr is None or keep_ptr % 4 == 0))
    if vec:
        return 'vec'
    if c_ptr % 16 == 0 and ldc % 4 != 0 and cpre_ptr is None and res_ptr is None and keep_ptr is None:
        return 'shifted'
    return 'scalar'


def nn_path(M, N, K, taps, lda, ldw, ldc, a_ptr, w_ptr, c_ptr, cpre_ptr=None, res_ptr=None, ldr=0, keep_ptr=None, nld=0,
            min_tiles=GEMM2_MIN_TILES, bf16x=True):
    f = nn_flags(a_ptr, lda, w_ptr, ldw, N, K, nld)
    if gemm2_takes(f, M, N, K, taps, lda, ldw, min_tiles):
        return 'g2.%s.%s' % (gemm2_form(bf16x, taps * K), gemm2_epilogue(c_ptr, ldc, N, cpre_ptr, res_ptr, ldr, keep_ptr))
    return 'nn.t%d.f%d' % (nn_tile(M, N), f)


def ksplit_plan(M, N, K, taps, slab_floats, forced=0, flags=3, min_tiles=GEMM2_MIN_TILES):
    """-> (S, per, [(it0, it1)]) of the k-split launch, in 32-deep k-tiles; S = 1: no k-split launch is made.  A forced S outside
    [1, maxS] is ignored and the makespan model's choice runs."""
    mn = M * N
    nit = taps * cdiv(K, 32)
    if not (flags == 3 and N % 4 == 0 and min_tiles > 0 and slab_floats > 0):
        return 1, nit, [(0, nit)]
    tiles = cdiv(M, 128) * cdiv(N, 128)
    maxS = min(MAX_GEMM_BATCH, slab_floats // mn, nit // 6)
    bestS, best = 1, 1e30
    for S in range(1, maxS + 1):
        slab_units = (2.0 * S * mn * 4.0 / 4.0e12) / 1.7e-6 if S > 1 else 0.0
        cost = float(cdiv(tiles * S, 256)) * cdiv(nit, S) + slab_units
        if cost < best * 0.97:
            best, bestS = cost, S
    if 1 <= forced <= maxS:
        bestS = forced
    if bestS < 2:
        return 1, nit, [(0, nit)]
    per = cdiv(nit, bestS)
    return bestS, per, [(c * per, min(nit, (c + 1) * per)) for c in range(bestS)]


def tn_plan(a_ptr, lda, y_ptr, ldy, M, N, K, taps, pad_l, merge=True, deterministic=False, bf16x=True):
    """-> dict(flags, merged, K, taps (as the kernel sees them), bm, splits, chunk, form, label)"""
    nld = N if N % 4 == 0 else 0
    lim31 = 1 << 31
    flags = 0
    if lda % 4 == 0 and a_ptr % 16 == 0 and K % 4 == 0 and (M + taps + 48) * lda * 4 < lim31:
        flags |= 1
    if ldy % 4 == 0 and y_ptr % 16 == 0 and nld > 0 and nld <= ldy and (M + 16) * ldy * 4 < lim31:
        flags |= 2
    merged = bool(merge and (flags & 1) and 1 < taps <= 17 and K % 64 != 0 and pad_l <= 16 and taps - 1 - pad_l <= 16)
    if merged:
        K, taps = K * taps, 1
    big = cdiv(K, 128) * cdiv(N, 128) * taps >= TN_BIG_TILES and K >= 128 and N >= 128
    bm = 128 if big else 64
    tiles = cdiv(K, bm) * cdiv(N, bm) * taps
    splits = 1 if deterministic else cdiv(TN_BLOCKS, tiles)
    splits = max(1, min(splits, cdiv(M, 320) if M >= 1280 else cdiv(M, 64)))
    chunk = cdiv(cdiv(M, splits), 16) * 16
    splits = cdiv(M, chunk)
    form = ('f3.bx' if bf16x and chunk <= BF16X_MAX_CHAIN else 'f3.f32') if flags == 3 else 'f%d' % flags
    return dict(flags=flags, merged=merged, K=K, taps=taps, bm=bm, splits=splits, chunk=chunk, form=form,
                label='tn.t%d.%s' % (bm, form))


PATH_TABLE = frozenset(
    ['nn.t%d.f%d' % (t, f) for t in (64, 128) for f in range(4)] +
    ['g2.%s.%s' % (m, e) for m in ('f32', 'bx') for e in ('vec', 'shifted', 'scalar')] +
    ['ksplit.S2', 'ksplit.S3', 'ksplit.S5'] +
    ['tn.t%d.%s' % (t, f) for t in (64, 128) for f in ('f3.bx', 'f3.f32', 'f1', 'f2', 'f0')] +
    # the forms of tests/gemm_forms.py
    ['g2.pool1.f32', 'g2.pool1.bx', 'g2.pool2', 'ew.bnpool.fwd', 'ew.bnpool.bwd', 'g2.bank.S2', 'g2.bank.S3', 'nn.atomic', 'nn.rowbias',
     'tn.group', 'tn.strided'])

# ------------------------------------------------------------------------------------------------------------------
# case lists.  Offsets are in floats from a 256-byte aligned buffer start (offK: bytes); every pitch is written out.
# opts: b bias, k keep, s scale, h shift, r residual, p Cpre.   g2: TACO_GEMM2_MIN_TILES ('' = leave the default), bx: TACO_GEMM2_BF16X.

NN = namedtuple('NN', 'id M T N K taps pad_l act opts lda ldw ldc ldr offA offW offC offR offK offP offB g2 bx path')


def _nn(id, M, T, N, K, taps, pad_l, act, opts, lda, ldw, ldc, ldr, offA, offW, offC, offR, offK, offP, offB, g2, bx, path):
    return NN(id, M, T, N, K, taps, pad_l, act, opts, lda, ldw, ldc, ldr, offA, offW, offC, offR, offK, offP, offB, g2, bx, path)


# (a) load paths of gemm.hip's NN kernel, 64 x 64 tile.  Every way to break bit 0 (A operand) and bit 1 (W operand) by itself,
#     both, neither; every flags class has a k-tile tail (K % 16 != 0) and an M tail (70, 130 are no multiples of 64).
#            id               M   T   N   K taps pad act opts   lda ldw ldc ldr oA oW oC oR oK oP oB  g2   bx  path
NN_LOAD_CASES = [
    _nn('a-lda1',            70, 35, 64, 20, 3,  1, 0, '',      21, 64, 67, 64, 0, 0, 2, 0, 0, 0, 0, '',  '1', 'nn.t64.f2'),
    _nn('a-lda2',           130, 26, 80, 36, 1,  0, 1, 'b',     38, 80, 80, 80, 0, 0, 0, 0, 0, 0, 0, '',  '1', 'nn.t64.f2'),
    _nn('a-lda3',            70, 35, 80, 20, 4,  0, 0, '',      23, 80, 81, 80, 0, 0, 1, 0, 0, 0, 0, '',  '1', 'nn.t64.f2'),
    _nn('a-offA1',          130, 26, 64, 36, 2,  3, 0, 'b',     36, 64, 64, 64, 1, 0, 0, 0, 0, 0, 0, '',  '1', 'nn.t64.f2'),
    _nn('a-offA2',           70, 35, 64, 20, 3, -1, 3, '',      24, 64, 66, 64, 2, 0, 3, 0, 0, 0, 0, '',  '1', 'nn.t64.f2'),
    _nn('a-offA3',          130, 26, 80, 20, 3,  1, 0, 'br',    20, 80, 80, 83, 3, 0, 0, 1, 0, 0, 0, '',  '1', 'nn.t64.f2'),
    _nn('a-K17',             70, 35, 64, 17, 3,  1, 0, '',      20, 64, 64, 64, 0, 0, 0, 0, 0, 0, 0, '',  '1', 'nn.t64.f2'),
    _nn('a-K18',            130, 26, 80, 18, 4,  0, 2, 'b',     20, 80, 84, 80, 0, 0, 0, 0, 0, 0, 0, '',  '1', 'nn.t64.f2'),
    _nn('a-K19',             70, 35, 64, 19, 2,  3, 0, '',      20, 64, 65, 64, 0, 0, 0, 0, 0, 0, 0, '',  '1', 'nn.t64.f2'),
    _nn('w-ldw1',            70, 35, 64, 20, 3,  1, 0, 'b',     20, 65, 64, 64, 0, 0, 0, 0, 0, 0, 0, '',  '1', 'nn.t64.f1'),
    _nn('w-ldw2',           130, 26, 80, 36, 4,  0, 1, '',      36, 82, 83, 80, 0, 0, 1, 0, 0, 0, 0, '',  '1', 'nn.t64.f1'),
    _nn('w-ldw3',            70, 35, 80, 20, 1,  0, 0, 'bsh',   24, 83, 80, 80, 0, 0, 0, 0, 0, 0, 1, '',  '1', 'nn.t64.f1'),
    _nn('w-offW1',          130, 26, 64, 36, 3, -1, 0, '',      36, 64, 64, 64, 0, 1, 0, 0, 0, 0, 0, '',  '1', 'nn.t64.f1'),
    _nn('w-offW2',           70, 35, 64, 20, 2,  3, 2, 'b',     20, 68, 66, 64, 0, 2, 0, 0, 0, 0, 0, '',  '1', 'nn.t64.f1'),
    _nn('w-offW3',          130, 26, 80, 20, 3,  1, 0, 'kp',    20, 80, 80, 80, 0, 3, 0, 0, 0, 2, 0, '',  '1', 'nn.t64.f1'),
    _nn('w-N61',             70, 35, 61, 20, 3,  1, 0, 'b',     20, 64, 61, 61, 0, 0, 0, 0, 0, 0, 0, '',  '1', 'nn.t64.f1'),
    _nn('w-N62',            130, 26, 62, 36, 4,  0, 3, '',      36, 64, 64, 62, 0, 0, 0, 0, 0, 0, 0, '',  '1', 'nn.t64.f1'),
    _nn('w-N63',             70, 35, 63, 20, 2,  3, 0, 'br',    20, 64, 63, 64, 0, 0, 3, 0, 0, 0, 0, '',  '1', 'nn.t64.f1'),
    _nn('aw-K17-N61',        70, 35, 61, 17, 3,  1, 1, 'b',     17, 61, 61, 61, 0, 0, 0, 0, 0, 0, 0, '',  '1', 'nn.t64.f0'),
    _nn('aw-offA1-offW3',   130, 26, 64, 36, 4,  0, 0, '',      36, 64, 64, 64, 1, 3, 1, 0, 0, 0, 0, '',  '1', 'nn.t64.f0'),
    _nn('aw-lda2-ldw1',      70, 35, 80, 20, 2,  3, 0, 'bksrp', 22, 81, 82, 81, 0, 0, 0, 0, 1, 1, 1, '',  '1', 'nn.t64.f0'),
    _nn('aw-K19-N63-neg',   130, 26, 63, 19, 3, -1, 2, 'h',     19, 63, 63, 63, 2, 1, 0, 0, 0, 0, 0, '',  '1', 'nn.t64.f0'),
    _nn('v-dense',           70, 35, 64, 20, 3,  1, 0, 'b',     20, 64, 64, 64, 0, 0, 0, 0, 0, 0, 0, '0', '1', 'nn.t64.f3'),
    _nn('v-pitched',        130, 26, 80, 36, 4,  0, 1, 'bs',    40, 84, 81, 80, 0, 0, 0, 0, 0, 0, 0, '0', '1', 'nn.t64.f3'),
    _nn('v-shift-out',       70, 35, 80, 36, 2,  3, 0, '',      36, 80, 80, 80, 4, 4, 0, 0, 0, 0, 0, '0', '1', 'nn.t64.f3'),
    _nn('v-neg-pad',        130, 26, 64, 20, 3, -1, 3, 'b',     20, 64, 64, 64, 0, 0, 2, 0, 0, 0, 0, '0', '1', 'nn.t64.f3'),
    _nn('v-dense-taps1',    130, 26, 64, 36, 1,  0, 0, '',      36, 64, 64, 64, 0, 0, 0, 0, 0, 0, 0, '0', '1', 'nn.t64.f3'),
]

# (b) 128 x 128 tile of gemm.hip: 24 x 16 = 384 tiles, one case per flags class
NN_BIG_CASES = [
    _nn('big-f3',   3067, 3067, 2048, 12, 1, 0, 0, 'b', 12, 2048, 2048, 2048, 0, 0, 0, 0, 0, 0, 0, '0', '1', 'nn.t128.f3'),
    _nn('big-f1',   3067, 3067, 2045, 12, 1, 0, 1, 'b', 12, 2045, 2045, 2045, 0, 0, 0, 0, 0, 0, 0, '',  '1', 'nn.t128.f1'),
    _nn('big-f2',   3069,  341, 2048, 13, 2, 0, 0, '',  13, 2048, 2048, 2048, 0, 0, 0, 0, 0, 0, 0, '',  '1', 'nn.t128.f2'),
    _nn('big-f0',   3069,  341, 2045, 12, 2, 1, 0, 'b', 12, 2048, 2047, 2045, 1, 0, 1, 0, 0, 0, 0, '',  '1', 'nn.t128.f0'),
]

# (c) epilogue options: every row runs on gemm.hip (TACO_GEMM2_MIN_TILES=0), on gemm2.hip's fp32 form and on its bf16x3 form
#     (MIN_TILES=1, TACO_GEMM2_BF16X 0 / 1); `path` is the EPILOGUE FORM gemm2.hip must choose.  M = 200 (T = 40), K = 36, taps 3.
EPI = namedtuple('EPI', 'id N act opts ldc ldr offC offR offK offP offB form')
#      id                  N  act opts      ldc  ldr oC oR oK oP oB  form
EPI_CASES = [
    EPI('vec-all',        128, 1, 'bkshrp', 128, 128, 0, 0, 0, 0, 0, 'vec'),
    EPI('vec-pitch4',     132, 2, 'brp',    136, 132, 0, 0, 0, 0, 0, 'vec'),
    EPI('vec-scale-only', 260, 3, 's',      260, 260, 0, 0, 0, 0, 0, 'vec'),
    EPI('vec-shift-only', 128, 0, 'h',      128, 128, 0, 0, 0, 0, 0, 'vec'),
    EPI('vec-keep-offB',  260, 1, 'bksh',   264, 260, 4, 0, 4, 0, 1, 'vec'),
    EPI('vec-res-pitch',  132, 0, 'r',      132, 136, 0, 4, 0, 0, 0, 'vec'),
    EPI('sh-ldc1',        128, 1, 'bsh',    129, 128, 0, 0, 0, 0, 0, 'shifted'),
    EPI('sh-ldc2',        132, 3, 's',      134, 132, 0, 0, 0, 0, 0, 'shifted'),
    EPI('sh-ldc1-offB',   260, 2, 'bh',     261, 260, 0, 0, 0, 0, 1, 'shifted'),
    EPI('sh-ldc2-plain',  128, 0, '',       130, 128, 0, 0, 0, 0, 0, 'shifted'),
    EPI('sh-ldc3',        260, 0, 'b',      263, 260, 0, 0, 0, 0, 0, 'shifted'),
    EPI('sc-offC1',       128, 1, 'bkshrp', 128, 128, 1, 0, 0, 0, 0, 'scalar'),
    EPI('sc-ldr1',        132, 0, 'br',     132, 133, 0, 0, 0, 0, 0, 'scalar'),
    EPI('sc-offR1',       260, 2, 'sr',     260, 260, 0, 1, 0, 0, 0, 'scalar'),
    EPI('sc-offK1',       128, 3, 'bkp',    128, 128, 0, 0, 1, 0, 0, 'scalar'),
    EPI('sc-offP1',       132, 1, 'hp',     132, 132, 0, 0, 0, 1, 0, 'scalar'),
    EPI('sc-ldc1-keep',   260, 0, 'bkh',    261, 260, 0, 0, 0, 0, 0, 'scalar'),
    EPI('sc-ldc2-pre',    128, 2, 'bp',     130, 128, 0, 0, 0, 0, 0, 'scalar'),
    EPI('sc-ldc1-res',    132, 3, 'sr',     133, 132, 0, 0, 0, 0, 1, 'scalar'),
    EPI('sc-everything',  132, 0, 'bkshrp', 133, 133, 1, 1, 1, 1, 1, 'scalar'),
    EPI('sc-offC1-plain', 260, 1, 's',      260, 260, 1, 0, 0, 0, 0, 'scalar'),
]
EPI_ENGINES = [('gemm', '0', '1'), ('g2-f32', '1', '0'), ('g2-bx', '1', '1')]      # (id, MIN_TILES, BF16X)
EPI_SHAPE = dict(M=200, T=40, K=36, taps=3, pad_l=1)


def epi_as_nn(e, engine):
    """the full NN row of epilogue case `e` on `engine` (operands dense and aligned: flags 3)"""
    name, g2, bx = engine
    s = EPI_SHAPE
    path = 'nn.t64.f3' if name == 'gemm' else 'g2.%s.%s' % ('bx' if bx == '1' else 'f32', e.form)
    return _nn('%s/%s' % (e.id, name), s['M'], s['T'], e.N, s['K'], s['taps'], s['pad_l'], e.act, e.opts, s['K'], e.N, e.ldc, e.ldr,
               0, 0, e.offC, e.offR, e.offK, e.offP, e.offB, g2, bx, path)


# (d) taco_debug_conv_gemm_nld: W rows zero-padded to nld loadable columns (N rounded up to 4, or that + 4 <= ldw), every ldc % 4;
#     lda = K by the entry's Python door.  M = 130, K = 36, dense (taps 1).
NLD = namedtuple('NLD', 'id N nld ldw ldc act bias g2 bx path')
NLD_CASES = [
    NLD('nld-131-ldc0',       131, 132, 132, 132, 0, True,  '1', '1', 'g2.bx.scalar'),
    NLD('nld-131-ldc1',       131, 136, 136, 133, 1, False, '1', '1', 'g2.bx.shifted'),
    NLD('nld-131-ldc2',       131, 132, 140, 134, 3, False, '1', '0', 'g2.f32.shifted'),
    NLD('nld-131-ldc3',       131, 136, 140, 131, 0, True,  '1', '0', 'g2.f32.shifted'),
    NLD('nld-262-ldc0',       262, 268, 268, 264, 2, False, '1', '0', 'g2.f32.scalar'),
    NLD('nld-262-ldc1',       262, 264, 272, 265, 0, True,  '1', '0', 'g2.f32.shifted'),
    NLD('nld-262-ldc2',       262, 268, 272, 262, 1, True,  '1', '1', 'g2.bx.shifted'),
    NLD('nld-262-ldc3',       262, 264, 264, 263, 3, False, '1', '1', 'g2.bx.shifted'),
    NLD('nld-131-gemm',       131, 132, 136, 133, 1, False, '0', '1', 'nn.t64.f3'),
    NLD('nld-262-gemm',       262, 268, 272, 262, 0, True,  '0', '1', 'nn.t64.f3'),
]
NLD_SHAPE = dict(M=130, K=36)

# (e) forced k-split (TACO_KSPLIT) through taco_debug_conv_gemm_ksplit (lda = K, ldw = ldc = N).  `slabs`: slab buffer in units of
#     M * N floats; S = the split that must really run (`ksplit_plan`): a forced value above min(16, slabs, nit / 6) is ignored.
#     The first two shapes are the issue's; the third has nit = 33, the smallest at which S = 5 is in range.
KS = namedtuple('KS', 'id M T N K taps pad_l act force slabs S path')
KSPLIT_CASES = [
    KS('ks-conv-S2',        260,  65, 128, 200, 3, 1, 1, 2, 3, 2, 'ksplit.S2'),     # per 11: it0 = 11 in the middle of tap 1, last chunk 10
    KS('ks-conv-S3',        260,  65, 128, 200, 3, 1, 0, 3, 3, 3, 'ksplit.S3'),     # one chunk per tap, K tail (200 = 6 * 32 + 8) in each
    KS('ks-conv-S5-ignored', 260, 65, 128, 200, 3, 1, 0, 5, 5, 3, 'ksplit.S3'),     # nit / 6 = 3: the model's choice runs
    KS('ks-conv-slab-bound', 260, 65, 128, 200, 3, 1, 3, 3, 2, 2, 'ksplit.S2'),     # two slabs only: the forced 3 is ignored
    KS('ks-dense-S2',       130, 130, 132, 516, 1, 0, 3, 2, 2, 2, 'ksplit.S2'),     # per 9 of 17: last chunk 8, K tail 4
    KS('ks-conv-S5',        130,  65, 128, 324, 3, 1, 0, 5, 5, 5, 'ksplit.S5'),     # per 7 of 33: cuts at 7, 14, 21, 28 (taps at 11, 22), last chunk 5
]

# (f) gemm_tn.  acc: accumulate onto random prior content; det: TACO_DETERMINISTIC; merge: TACO_TN_MERGE_TAPS.
#     `merged`, `splits`: what plan_gemm_tn must decide (read back from the launch's profile label).
TNC = namedtuple('TNC', 'id M T N K taps pad_l lda ldy ldw offA offY offW acc bx merge det merged splits path')
#        id                  M   T    N     K  taps pad lda  ldy   ldw  oA oY oW  acc    bx   merge det  merged spl path
TN_PATH_CASES = [
    TNC('tn-f3-bx',          77, 77,  20,   36, 1,  0,  36,   20,   20, 0, 0, 0, False, '1', '1', '0', False, 2, 'tn.t64.f3.bx'),
    TNC('tn-f3-f32',        360, 36, 128,  128, 3,  1, 128,  128,  128, 0, 0, 0, False, '0', '1', '0', False, 6, 'tn.t64.f3.f32'),
    TNC('tn-f3-bx-merged',  360, 36,  20,   36, 3,  1,  36,   20,   23, 0, 0, 1, False, '1', '1', '0', True,  6, 'tn.t64.f3.bx'),
    TNC('tn-f3-f32-merged', 360, 36, 128,   80, 8,  3,  84,  132,  128, 4, 4, 0, True,  '0', '1', '0', True,  6, 'tn.t64.f3.f32'),
    TNC('tn-f3-unmerged',   360, 36,  20,   36, 3,  1,  36,   20,   20, 0, 0, 0, False, '1', '0', '0', False, 6, 'tn.t64.f3.bx'),
    TNC('tn-f3-shift-out',   77, 77,  20,   80, 2,  3,  80,   20,   23, 0, 0, 0, True,  '1', '1', '0', True,  2, 'tn.t64.f3.bx'),
    TNC('tn-f3-neg-det',    360, 36, 128,   36, 3, -1,  36,  128,  131, 0, 0, 1, False, '1', '1', '1', True,  1, 'tn.t64.f3.bx'),
    TNC('tn-f1-ldy',         77, 77,  20,   36, 1,  0,  36,   21,   20, 0, 0, 0, False, '1', '1', '0', False, 2, 'tn.t64.f1'),
    TNC('tn-f1-offY',       360, 36, 128,   80, 3,  1,  80,  128,  131, 0, 1, 0, True,  '1', '1', '0', True,  6, 'tn.t64.f1'),
    TNC('tn-f1-N21',         77, 77,  21,  128, 2,  3, 128,   24,   21, 0, 0, 0, False, '1', '1', '0', False, 2, 'tn.t64.f1'),
    TNC('tn-f1-N22-merged', 360, 36,  22,   36, 8,  3,  36,   22,   25, 0, 0, 1, False, '1', '1', '0', True,  6, 'tn.t64.f1'),
    TNC('tn-f2-lda',         77, 77,  20,   36, 1,  0,  37,   20,   20, 0, 0, 0, False, '1', '1', '0', False, 2, 'tn.t64.f2'),
    TNC('tn-f2-offA',       360, 36, 128,   80, 3,  1,  80,  128,  128, 2, 0, 0, True,  '1', '1', '0', False, 6, 'tn.t64.f2'),
    TNC('tn-f2-K37',         77, 77,  20,   37, 3, -1,  40,   20,   23, 0, 0, 1, False, '1', '1', '0', False, 2, 'tn.t64.f2'),
    TNC('tn-f2-K38',        360, 36, 128,   38, 8,  3,  38,  128,  128, 0, 0, 0, False, '1', '1', '1', False, 1, 'tn.t64.f2'),
    TNC('tn-f0-K37-N21',     77, 77,  21,   37, 2,  3,  37,   21,   24, 0, 0, 0, True,  '1', '1', '0', False, 2, 'tn.t64.f0'),
    TNC('tn-f0-offs',       360, 36, 128,   36, 3,  1,  36,  128,  131, 1, 3, 1, False, '1', '1', '0', False, 6, 'tn.t64.f0'),
    TNC('tn-f0-pitches',    360, 36,  22,   38, 3, -1,  39,   23,   22, 0, 0, 0, False, '1', '1', '0', False, 6, 'tn.t64.f0'),
    # 128 x 128 tile: 8 x 16 = 128 tiles of one tap, or 4 x 4 x 8 taps
    TNC('tn-big-f3-bx',      48, 48, 2048, 1024, 1, 0, 1024, 2048, 2048, 0, 0, 0, False, '1', '1', '0', False, 1, 'tn.t128.f3.bx'),
    TNC('tn-big-f3-f32',     48, 48, 2048, 1024, 1, 0, 1024, 2048, 2051, 0, 0, 1, True,  '0', '1', '0', False, 1, 'tn.t128.f3.f32'),
    TNC('tn-big-f1',         48, 48, 2046, 1024, 1, 0, 1024, 2046, 2046, 0, 0, 0, False, '1', '1', '0', False, 1, 'tn.t128.f1'),
    TNC('tn-big-f2',         48, 48, 2048, 1022, 1, 0, 1022, 2048, 2048, 0, 0, 0, False, '1', '1', '0', False, 1, 'tn.t128.f2'),
    TNC('tn-big-f0',         48, 48, 2046, 1022, 1, 0, 1024, 2048, 2049, 1, 1, 0, False, '1', '1', '0', False, 1, 'tn.t128.f0'),
    TNC('tn-big-taps8',      64, 32,  512,  512, 8, 3,  512,  512,  512, 0, 0, 0, False, '1', '1', '0', False, 1, 'tn.t128.f3.bx'),
]


def all_nn_rows():
    return (NN_LOAD_CASES + NN_BIG_CASES + [epi_as_nn(e, g) for e in EPI_CASES for g in EPI_ENGINES])


def host_ptr(off_floats):
    """a pointer as the restatement sees it for a buffer that starts 256-byte aligned (tests/poison.py carve)"""
    return 1 << 20 | 4 * off_floats


def nn_row_path(c, a_ptr=None, w_ptr=None, c_ptr=None, cpre_ptr=None, res_ptr=None, keep_ptr=None):
    """label of NN row `c` from the restated predicates; pointers default to the host's aligned-buffer model"""
    a_ptr = host_ptr(c.offA) if a_ptr is None else a_ptr
    w_ptr = host_ptr(c.offW) if w_ptr is None else w_ptr
    c_ptr = host_ptr(c.offC) if c_ptr is None else c_ptr
    if 'p' in c.opts and cpre_ptr is None:
        cpre_ptr = host_ptr(c.offP)
    if 'r' in c.opts and res_ptr is None:
        res_ptr = host_ptr(c.offR)
    if 'k' in c.opts and keep_ptr is None:
        keep_ptr = (1 << 20) + c.offK
    return nn_path(c.M, c.N, c.K, c.taps, c.lda, c.ldw, c.ldc, a_ptr, w_ptr, c_ptr, cpre_ptr, res_ptr, c.ldr, keep_ptr,
                   min_tiles=GEMM2_MIN_TILES if c.g2 == '' else int(c.g2), bf16x=c.bx != '0')


def nld_path(c, a_ptr=None, w_ptr=None, c_ptr=None):
    s = NLD_SHAPE
    a_ptr, w_ptr, c_ptr = (host_ptr(0) if p is None else p for p in (a_ptr, w_ptr, c_ptr))
    return nn_path(s['M'], c.N, s['K'], 1, s['K'], c.ldw, c.ldc, a_ptr, w_ptr, c_ptr, nld=c.nld, min_tiles=int(c.g2), bf16x=c.bx != '0')


def tn_case_plan(c, a_ptr=None, y_ptr=None):
    a_ptr = host_ptr(c.offA) if a_ptr is None else a_ptr
    y_ptr = host_ptr(c.offY) if y_ptr is None else y_ptr
    return tn_plan(a_ptr, c.lda, y_ptr, c.ldy, c.M, c.N, c.K, c.taps, c.pad_l, merge=c.merge != '0', deterministic=c.det == '1',
                   bf16x=c.bx != '0')
