"""GPU: op-level parity of the HIP kernels (through the C ABI) against NumPy fp64 restatements.
Tolerances (fp32 kernel vs fp64 oracle): rel-L2 <= 2e-6 * sqrt(K)-ish, stated per test.

Every output and scratch buffer is carved from a guarded arena (tests/poison.py `Guarded`) and starts poisoned -- NaN (`qnan`) for
what a kernel overwrites, 7.0 / 7.5 where a test needs a finite fill, `noise` for scratch, `ones` for byte outputs; buffers the
header wants zeroed (Adam's m, v) are zeroed.  After the call the guard bands are bytewise intact, written buffers hold no
poison, and the margins of strided outputs kept their fill bytewise."""
import numpy as np
import pytest
import torch

from oracle import taco_numpy as on
from tests.gemm_paths import conv_ref
from tests.poison import Guarded
from tests.util import report

pytestmark = pytest.mark.gpu


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to('cuda', dtype).contiguous()


def test_naive_gemm_plumbing(built_lib):
    rng = np.random.default_rng(0)
    M, N, K = 37, 24, 19
    A, W, b = rng.standard_normal((M, K)), rng.standard_normal((1, K, N)), rng.standard_normal(N)
    G = Guarded({'C': ((M, N), torch.float32, 'qnan')})
    C = G['C']
    built_lib.debug_gemm_naive(dev(A), dev(W), C, M, N, K, bias=dev(b), act=1)
    G.check('C')
    ref, _ = conv_ref(A, W, b, M, 0, 1)
    r, m = report('naive gemm', C.cpu().numpy(), ref)
    assert r < 1e-6


CASES = [
    # M, T, N, K, taps, pad_l, act, extras
    (128, 128, 128, 128, 1, 0, 0, ''),
    (256, 64, 128, 64, 3, 1, 1, 'bias'),
    (70, 35, 80, 20, 3, 1, 1, 'bias,scale,residual,pre'),
    (90, 9, 128, 128, 16, 7, 1, 'bias'),
    (90, 9, 128, 80, 8, 3, 1, 'bias'),
    (64, 64, 1025, 256, 1, 0, 0, 'bias'),
    (200, 200, 256, 256, 1, 0, 1, 'bias,keep'),
    (6400, 200, 256, 256, 1, 0, 2, 'bias'),        # 100 tiles of 128 x 128: still the 64 x 64 kernel (tests/gemm_paths.py nn_tile)
    (3000, 3000, 384, 136, 1, 0, 3, 'bias'),       # 72 tiles, ragged edges; the 128 x 128 kernel: tests/test_gpu_gemm_paths.py
    (36, 9, 128, 128, 5, 2, 0, 'residual'),
    (36, 9, 80, 128, 6, 3, 0, ''),                 # backward-style pad (k-1 - (k-1)//2)
]


@pytest.mark.parametrize('case', CASES, ids=[str(c[:6]) for c in CASES])
def test_conv_gemm(built_lib, case):
    M, T, N, K, taps, pad_l, act, extras = case
    rng = np.random.default_rng(hash(case[:6]) % 2**31)
    A = rng.standard_normal((M, K))
    W = rng.standard_normal((taps, K, N)) / np.sqrt(K * taps)
    bias = rng.standard_normal(N) if 'bias' in extras else None
    keep = rng.integers(0, 2, (M, N)).astype(np.uint8) if 'keep' in extras else None
    scale = rng.standard_normal(N) if 'scale' in extras else None
    shift = rng.standard_normal(N) if 'scale' in extras else None
    res = rng.standard_normal((M, N)) if 'residual' in extras else None
    G = Guarded({'C': ((M, N), torch.float32, 'qnan'), 'Cpre': ((M, N), torch.float32, 'qnan')})
    C = G['C']
    Cpre = G['Cpre'] if 'pre' in extras else None
    built_lib.conv_gemm(dev(A), dev(W), C, M, N, K, taps=taps, T=T, pad_l=pad_l, act=act,
                        bias=None if bias is None else dev(bias), scale=None if scale is None else dev(scale),
                        shift=None if shift is None else dev(shift), residual=None if res is None else dev(res),
                        keep=None if keep is None else dev(keep, torch.uint8), Cpre=Cpre)
    G.check(*(('C', 'Cpre') if Cpre is not None else ('C',)))      # (an unused Cpre keeps its poison: nothing wrote there)
    assert Cpre is not None or G.margin_intact('Cpre', torch.ones(M, N, dtype=torch.bool))
    ref, pre = conv_ref(A, W, bias, T, pad_l, act, keep, scale, shift, res)
    r, m = report('conv_gemm %s' % (case[:7],), C.cpu().numpy(), ref)
    assert r < 5e-6
    if Cpre is not None:
        assert report('  Cpre', Cpre.cpu().numpy(), pre)[0] < 5e-6


V2_CASES = [c for c in CASES if c[2] % 4 == 0 and c[3] % 4 == 0] + [
    (1000, 200, 300, 132, 3, 1, 1, 'bias,keep,scale,residual,pre'),   # every ragged edge at once: M, N, K tails, 5 sequences
    (640, 40, 128, 128, 16, 7, 1, 'bias'),                            # widest conv-bank problem
    (720, 360, 1024, 256, 3, 1, 0, ''),                               # post-net dpool-like: many n-tiles
    (520, 520, 260, 2048, 1, 0, 0, 'bias'),                           # deep K (64 k-tiles of 32)
]


# (MFMA form, k-tile depth x ring stages): 'f32' = v_mfma_f32_32x32x2_f32 (rounds 2-4), 'bx' = the bf16x3 form of round 5
V2_VARIANTS = [('0', '32x2'), ('0', '32x3'), ('0', '16x3'), ('0', '16x4'), ('0', '16x5'), ('1', '16x3'), ('1', '16x4'), ('1', '16x5')]
V2_IDS = ['%s-%s' % ('bx' if b == '1' else 'f32', v) for b, v in V2_VARIANTS]


@pytest.mark.parametrize('variant', V2_VARIANTS, ids=V2_IDS)
@pytest.mark.parametrize('case', V2_CASES, ids=[str(c[:6]) for c in V2_CASES])
def test_conv_gemm_v2(built_lib, case, variant, monkeypatch):
    """gemm2.hip (DMA-staged, swizzled kernel) forced for every shape that meets its contract, in all its instantiations -- the
    fp32 MFMA form in five (k-tile depth x ring stages) shapes and the bf16x3 form (fp32 operands split into three bf16 planes in
    registers, six v_mfma_f32_32x32x16_bf16 per sub-tile, TACO_GEMM2_BF16X) in three: K / N / M tails as out-of-range buffer
    offsets (zeros), tap shifts across sequence boundaries, the float4 and the scalar epilogue.  Same tolerance for both forms."""
    monkeypatch.setenv('TACO_GEMM2_MIN_TILES', '1')
    monkeypatch.setenv('TACO_GEMM2_BF16X', variant[0])
    monkeypatch.setenv('TACO_GEMM2_VARIANT', variant[1])
    test_conv_gemm(built_lib, case)


WIMG_CASES = [c for c in V2_CASES if c[7] in ('', 'bias')] + [
    (1000, 200, 300, 132, 3, 1, 1, 'bias'),      # ragged: N and K tails are zeros of the image
    (640, 40, 80, 128, 8, 4, 0, ''),             # N = 80 (post-net bank gather's width)
    (384, 384, 1028, 256, 1, 0, 0, 'bias'),      # nine n-tiles, the last one 4 columns wide
]


@pytest.mark.parametrize('ns', ['3', '4'])
@pytest.mark.parametrize('case', WIMG_CASES, ids=[str(c[:6]) for c in WIMG_CASES])
def test_conv_gemm_weight_image(built_lib, case, ns, monkeypatch):
    """Round 6: the bf16x3 form with the weight operand read from a pre-split plane image (csrc/kernels.h "weight images": planes
    formed once per weight tensor by weight_image_kernel, DMA'd as 12 KB fragment-ordered tiles, no B split in the GEMM).  The
    image holds exactly the planes the in-register split forms and the MFMAs run in the same order, so the result must be BIT
    IDENTICAL to the in-register bf16x3 form (TACO_GEMM2_BSPLIT=0) -- and within the suite's 5e-6 of fp64.  Three- and four-stage
    rings; K / N tails, taps, several n-tiles."""
    M, T, N, K, taps, pad_l, act, extras = case
    monkeypatch.setenv('TACO_GEMM2_MIN_TILES', '1')
    monkeypatch.setenv('TACO_GEMM2_BF16X', '1')
    monkeypatch.setenv('TACO_GEMM2_BI_NS', ns)
    rng = np.random.default_rng(hash(case[:6]) % 2**31)
    A = rng.standard_normal((M, K))
    W = rng.standard_normal((taps, K, N)) / np.sqrt(K * taps)
    bias = rng.standard_normal(N) if 'bias' in extras else None
    dA, dW, db = dev(A), dev(W), (None if bias is None else dev(bias))
    ref, _ = conv_ref(A, W, bias, T, pad_l, act)
    built_lib.weight_image(None)
    G = Guarded({'C0': ((M, N), torch.float32, 'qnan'), 'C1': ((M, N), torch.float32, 'qnan'),
                 'img': ((built_lib.weight_image_bytes(dW, taps, K, N) // 2,), torch.int16, 'qnan')})
    C0 = G['C0']
    built_lib.conv_gemm(dA, dW, C0, M, N, K, taps=taps, T=T, pad_l=pad_l, act=act, bias=db)      # no image registered: in-register split
    assert built_lib.weight_image(None) == 0
    img = built_lib.weight_image(dW, taps=taps, K=K, N=N, img=G['img'])
    C1 = G['C1']
    built_lib.conv_gemm(dA, dW, C1, M, N, K, taps=taps, T=T, pad_l=pad_l, act=act, bias=db)
    torch.cuda.synchronize()
    assert built_lib.weight_image(None) == 1, 'the launch did not take the image form'
    del img
    G.check('C0', 'C1')
    assert report('conv_gemm image form %s' % (case[:7],), C1.cpu().numpy(), ref)[0] < 5e-6
    assert torch.equal(C0, C1), 'image form differs from the in-register split: max |d| = %g' % float((C0 - C1).abs().max())


def test_model_weight_images_do_not_outlive_the_call(built_lib, monkeypatch):
    """The weight images a model-level call builds are keyed by its parameter pointers and live in its workspace: they must leave
    this thread's table when the call returns.  After one train step (forward, backward, clip + Adam) an op-level conv_gemm on a
    parameter slice that the forward pass registered an image for (the encoder bi-GRU's x-side gate kernel: taps 1, K 128) must
    compute with the UPDATED parameters, not read the pre-Adam image."""
    from tacotron_amd.config import Config
    from tacotron_amd.data import synthetic_batch
    from tacotron_amd.model import Tacotron
    monkeypatch.setenv('TACO_GEMM2_MIN_TILES', '1')
    monkeypatch.setenv('TACO_GEMM2_BF16X', '1')
    c = Config()
    c.r, c.vocab_size = 2, 20
    batch = synthetic_batch(2, 12, 6, c.r, c.vocab_size, seed=3, min_len=6)
    m = Tacotron(c, batch, train=True, seed=0)
    Wfull = m.params.view('encoder/cbhg/bigru/fw/gates/kernel')   # (256, 256): rows [0, 128) are the x-side part
    W0 = Wfull[:128].double().cpu().numpy()
    built_lib.weight_image(None)
    m.step(lr=1e-3)
    torch.cuda.synchronize()
    W1 = Wfull[:128].double().cpu().numpy()
    assert np.abs(W1 - W0).max() > 1e-4, 'the Adam step did not move the parameters: the test would not see a stale image'
    M, K, N = 256, 128, 256
    A = np.random.default_rng(5).standard_normal((M, K))
    G = Guarded({'C': ((M, N), torch.float32, 'qnan')})
    C = G['C']
    built_lib.conv_gemm(dev(A), Wfull[:128], C, M, N, K)
    torch.cuda.synchronize()
    G.check('C')
    ref, _ = conv_ref(A, W1[None], None, M, 0, 0)
    assert report('conv_gemm after a train step', C.cpu().numpy(), ref)[0] < 5e-6


@pytest.mark.parametrize('scale', [1.0, 1e-12, 3e7], ids=['unit', 'tiny', 'huge'])
def test_bf16x3_products_are_fp32_grade(built_lib, scale, monkeypatch):
    """The bf16x3 form of gemm2.hip against the fp32 MFMA form of the same kernel and an fp64 product: a deep reduction (K = 2048
    x 3 taps) over heavy-tailed operands (log-normal magnitudes over ~5 decades; gradient-like scales included).  The split is
    exact (x = h + m + l) and the six retained plane products cover everything above 2^-24 of a product; what the bf16
    instruction adds is its 16-term internal sum (one alignment per 16 products instead of per 2).  Measured on MI355X: rel-L2
    1.8e-7 vs 1.4e-7 of the fp32 form on these operands.  Asserted: <= 2 x the fp32 form's error, and both <= the suite's 5e-6
    (i.e. 25 x below the tolerance every GEMM test of this file states)."""
    monkeypatch.setenv('TACO_GEMM2_MIN_TILES', '1')
    monkeypatch.setenv('TACO_GEMM2_VARIANT', '16x4')
    rng = np.random.default_rng(11)
    M, T, N, K, taps = 512, 128, 256, 2048, 3
    A = (rng.standard_normal((M, K)) * np.exp(rng.standard_normal((M, K)) * 3)).astype(np.float32) * np.float32(scale)
    W = (rng.standard_normal((taps, K, N)) * np.exp(rng.standard_normal((taps, K, N)) * 3) / np.sqrt(K * taps)).astype(np.float32)
    ref, _ = conv_ref(A.astype(np.float64), W.astype(np.float64), None, T, 1, 0)
    err = {}
    for bx in ('0', '1'):
        monkeypatch.setenv('TACO_GEMM2_BF16X', bx)
        G = Guarded({'C': ((M, N), torch.float32, 'qnan')})
        C = G['C']
        before = built_lib.debug_gemm2_window(0, 1 << 30)
        built_lib.conv_gemm(dev(A), dev(W), C, M, N, K, taps=taps, T=T, pad_l=1, act=0)
        assert built_lib.debug_gemm2_window(0, 1 << 30) == 1, 'the launch did not go to gemm2.hip'
        G.check('C')
        err[bx] = report('gemm2 %s scale=%g' % ('bf16x3' if bx == '1' else 'fp32  ', scale), C.cpu().numpy(), ref)
    assert err['0'][0] < 5e-6 and err['1'][0] < 5e-6
    assert err['1'][0] <= 2.0 * err['0'][0] and err['1'][1] <= 2.5 * err['0'][1]


def _ones_mantissa(rng, shape, spread=2):
    """Same-signed fp32 values with ALL mantissa bits set, (2 - 2^-23) * 2^e with e ~ U{-spread..spread}: each of the three bf16
    planes of the split is as large as it can be relative to the one above, and with one sign the three dropped plane products
    (m l, l m, l l) of the bf16x3 form cannot cancel -- its coherent worst case."""
    e = rng.integers(-spread, spread + 1, shape)
    return (np.float32(2.0 - 2.0 ** -23) * np.exp2(e).astype(np.float32)).astype(np.float32)


def _adversarial_case(rng, kernel, kind, depth):
    """(run, ref): the NN kernel of gemm2.hip (M x depth @ depth x N) or the weight-gradient kernel of gemm.hip (dW = A^T dY over
    `depth` rows) on same-signed all-ones-mantissa or heavy-tailed operands."""
    def operand(shape, norm):
        if kind == 'heavy-tailed':
            return (rng.standard_normal(shape) * np.exp(rng.standard_normal(shape) * 3) / norm).astype(np.float32)
        return _ones_mantissa(rng, shape)
    if kernel == 'nn':
        M, N, K = 512, 256, depth
        A, W = operand((M, K), 1.0), operand((1, K, N), np.sqrt(K))
        ref = A.astype(np.float64) @ W[0].astype(np.float64)

        def run(built_lib):
            G = Guarded({'C': ((M, N), torch.float32, 'qnan')})
            C = G['C']
            built_lib.debug_gemm2_window(0, 1 << 30)
            built_lib.conv_gemm(dev(A), dev(W), C, M, N, K, taps=1, T=M, pad_l=0, act=0)
            assert built_lib.debug_gemm2_window(0, 1 << 30) == 1, 'the launch did not go to gemm2.hip'
            G.check('C')
            return C.cpu().numpy()
    else:
        M, N, K = depth, 256, 512          # dW (K, N) = A^T (K, M) dY (M, N): the reduction runs over the M = depth rows
        A, dY = operand((M, K), 1.0), operand((M, N), np.sqrt(M))
        ref = A.astype(np.float64).T @ dY.astype(np.float64)

        def run(built_lib):
            G = Guarded({'dW': ((1, K, N), torch.float32, 'qnan')})
            dW = G['dW']
            built_lib.gemm_tn(dev(A), dev(dY), dW, M, N, K, taps=1, T=M, pad_l=0, accumulate=False)
            G.check('dW')
            return dW[0].cpu().numpy()
    return run, ref


@pytest.mark.parametrize('kind', ['ones-mantissa-same-sign', 'heavy-tailed'])
@pytest.mark.parametrize('kernel,depth', [('nn', 6144), ('nn', 2048), ('tn', 6144), ('tn-deterministic', 6144)],
                         ids=['nn-6144', 'nn-2048-deepest-bf16x3-chain', 'tn-6144', 'tn-6144-one-workgroup-per-tile'])
def test_bf16x3_adversarial_operands(built_lib, kernel, depth, kind, monkeypatch):
    """Worst-case rather than statistical evidence for the products of the big GEMM kernels (VERDICT r5 #9 / next #7a), on BOTH
    kernels that have a bf16x3 form: the NN kernel of gemm2.hip and the weight-gradient kernel of gemm.hip (gemm_tn).
    `ones-mantissa-same-sign`: every operand positive with all 23 mantissa bits set -- no cancellation anywhere: the three dropped
    plane products (m l, l m, l l) are one-signed, and the accumulator grows linearly, which is what exposes how the matrix pipe adds
    (it rounds every product by itself onto the accumulator's grid: tools/micro/mfma_bf16_probe.hip); `heavy-tailed`: log-normal
    magnitudes over ~5 decades.  What the library does about it (bf16x3.h): the low-order plane products have an accumulator of
    their own (`mfma6_2`), and the bf16x3 form is used for accumulation chains of at most 2048 products (`bf16x_max_chain`); deeper
    ones run the fp32 MFMA instruction.  Asserted, default settings against an fp64 product: **rel-L2 <= 4e-7** (the verdict's bar)
    in every case -- depth 6144 (encoder proj1's depth: NN routed to the fp32 instruction, gemm_tn's split row ranges of 384 rows
    on bf16x3, its single-workgroup form routed) and depth 2048, the deepest chain the bf16x3 form is used for (measured 3.2e-7 on
    same-signed full mantissas, 2.0e-7 heavy-tailed) -- and <= 3 x the error of the forced fp32 MFMA form with a floor of 1.2e-7
    (on same-signed full mantissas the fp32 instruction itself measures 2e-8, a level the split form does not reach: the ratio is
    printed; heavy-tailed NN at depth 6144: the fp32 instruction measures 4.3e-7 and is what runs)."""
    monkeypatch.setenv('TACO_GEMM2_MIN_TILES', '1')
    monkeypatch.setenv('TACO_GEMM2_VARIANT', '16x4')
    if kernel == 'tn-deterministic':
        monkeypatch.setenv('TACO_DETERMINISTIC', '1')
    run, ref = _adversarial_case(np.random.default_rng(23), kernel[:2], kind, depth)
    err = {}
    for bx in ('0', '1'):
        monkeypatch.setenv('TACO_GEMM2_BF16X', bx)
        err[bx] = report('%s depth %d %s %s' % (kernel, depth, kind, 'default' if bx == '1' else 'fp32  '), run(built_lib), ref)
    print('  %s depth %d / %s: rel-L2 default %.2e vs forced fp32 MFMA %.2e (ratio %.2f); 4e-7 bar: default %s, fp32 MFMA %s'
          % (kernel, depth, kind, err['1'][0], err['0'][0], err['1'][0] / max(err['0'][0], 1e-30),
             'met' if err['1'][0] <= 4e-7 else 'NOT met', 'met' if err['0'][0] <= 4e-7 else 'NOT met'))
    assert err['0'][0] < 5e-6 and err['1'][0] < 5e-6
    assert err['1'][0] <= max(4e-7, 1.05 * err['0'][0])       # the 4e-7 bar (or the fp32 instruction's own error where that is what runs)
    assert err['1'][0] <= 3.0 * max(err['0'][0], 1.2e-7)


def test_bf16x3_chain_bound_is_what_keeps_deep_same_signed_sums_fp32_grade(built_lib, monkeypatch):
    """The reason for `bf16x_max_chain` (bf16x3.h), kept executable: with the bound lifted, a 6144-deep sum of same-signed
    full-mantissa products on the bf16x3 form measures 2.4e-6 (two accumulators; 1.7e-5 with one) against 5e-8 of the fp32
    instruction -- outside the 4e-7 bar the bounded path meets -- while mixed-sign operands are MORE accurate than the fp32
    instruction at any depth (0.3-0.4 x; tools/bf16x3_chain_probe.py, profiles/r06_bf16x3_acc2.txt).  If this test ever FAILS
    because the forced form has become accurate, the bound can go."""
    monkeypatch.setenv('TACO_GEMM2_MIN_TILES', '1')
    monkeypatch.setenv('TACO_GEMM2_VARIANT', '16x4')
    monkeypatch.setenv('TACO_GEMM2_BF16X', '1')
    run, ref = _adversarial_case(np.random.default_rng(23), 'nn', 'ones-mantissa-same-sign', 6144)
    bounded = report('nn 6144 same-signed, default bound', run(built_lib), ref)[0]
    monkeypatch.setenv('TACO_BF16X_MAX_CHAIN', str(1 << 30))
    forced = report('nn 6144 same-signed, bf16x3 forced ', run(built_lib), ref)[0]
    assert bounded <= 4e-7 and forced > 10 * bounded and forced > 4e-7


@pytest.mark.parametrize('case', [(1000, 200, 128, 2048, 3, 1, 1), (520, 130, 256, 1024, 3, 1, 0), (300, 300, 132, 516, 1, 0, 3)],
                         ids=['enc-proj1-like', 'post-proj1-like', 'ragged'])
def test_conv_gemm_ksplit(built_lib, case):
    """Tall-skinny projections: (tap, k) chunks as independent workgroups of the gemm2 kernel + ordered slab sum; twice, to
    pin run-to-run bit reproducibility (no atomics anywhere on this path)."""
    M, T, N, K, taps, pad_l, act = case
    rng = np.random.default_rng(7)
    A = rng.standard_normal((M, K))
    W = rng.standard_normal((taps, K, N)) / np.sqrt(K * taps)
    bias = rng.standard_normal(N)
    outs = []
    for fill in ('noise', 'qnan'):         # what the partial slabs hold before the call must not matter
        G = Guarded({'slabs': ((4 * M * N,), torch.float32, fill), 'C': ((M, N), torch.float32, 'qnan')})
        slabs, C = G['slabs'], G['C']
        built_lib.conv_gemm_ksplit(dev(A), dev(W), C, M, N, K, slabs, taps=taps, T=T, pad_l=pad_l, act=act, bias=dev(bias))
        G.check('C')
        outs.append(C.clone())
    ref, _ = conv_ref(A, W, bias, T, pad_l, act)
    assert report('conv_gemm_ksplit %s' % (case,), outs[0].cpu().numpy(), ref)[0] < 5e-6
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize('variant', ['16x4', '32x2', 'bx'])
@pytest.mark.parametrize('N,ldc,act', [(1025, 1025, 0), (1025, 1027, 1), (514, 518, 0), (131, 133, 3), (1024, 1025, 0), (1025, 1030, 0), (133, 135, 0),
                                       (262, 263, 0)],
                         ids=['dense-1025', 'pitch-3mod4', 'pitch-2mod4', 'narrow', 'full-tiles', 'pitch-2mod4-odd-N', 'tail-5-of-a-tile',
                              'tail-6-of-a-tile'])
def test_conv_gemm_v2_shifted_rows(built_lib, N, ldc, act, variant, monkeypatch):
    """gemm2.hip's shifted float4 epilogue: output rows whose pitch is not a multiple of 4 floats (the final dense layer writes
    (B*F, 1025) from a weight copy padded to 1028 columns, tacotron.py:148 / model.hip).  Every pitch residue, the N tail inside
    a tile, an M tail; nothing may land outside the N columns of a row (sentinel in the pitch padding and behind the last row),
    and the kernel must really be the DMA one (the old kernel is switched off for the call)."""
    monkeypatch.setenv('TACO_GEMM2_MIN_TILES', '1')
    monkeypatch.setenv('TACO_GEMM2_BF16X', '1' if variant == 'bx' else '0')
    monkeypatch.setenv('TACO_GEMM2_VARIANT', '16x4' if variant == 'bx' else variant)
    rng = np.random.default_rng(N * 7 + ldc)
    M, K = 333, 96
    nld = (N + 3) // 4 * 4
    A = rng.standard_normal((M, K))
    W = rng.standard_normal((1, K, N)) / np.sqrt(K)
    Wp = np.zeros((K, nld)); Wp[:, :N] = W[0]
    bias = rng.standard_normal(N)
    G = Guarded({'flat': ((M * ldc + 64,), torch.float32, 7.5)})
    flat = G['flat']
    before = built_lib.debug_gemm2_window(0, 1 << 30)
    built_lib.conv_gemm_nld(dev(A), dev(Wp), flat, M, N, K, nld, nld, ldc, act=act, bias=dev(bias))
    assert built_lib.debug_gemm2_window(0, 1 << 30) == 1, 'the launch did not go to gemm2.hip'
    ref, _ = conv_ref(A, W, bias, M, 0, act)
    C = flat[:M * ldc].view(M, ldc)
    assert report('shifted rows N=%d ldc=%d %s' % (N, ldc, variant), C[:, :N].cpu().numpy(), ref)[0] < 5e-6
    assert bool((C[:, N:] == 7.5).all()) and bool((flat[M * ldc:] == 7.5).all())
    G.check()


def test_conv_gemm_strided_unaligned(built_lib):
    """lda not a multiple of 4 (1025-wide rows) exercises the scalar-load path; ldc > N exercises column offsets."""
    rng = np.random.default_rng(5)
    M, K, N = 96, 1025, 256
    A = rng.standard_normal((M, K))
    W = rng.standard_normal((1, K, N)) / 32
    G = Guarded({'flat': ((M * 300 + 20,), torch.float32, 'qnan')})
    flat = G['flat']                                         # C = flat[20:] viewed with ldc = 300
    built_lib.conv_gemm(dev(A), dev(W), flat[20:], M, N, K, lda=1025, ldc=300)
    C = flat[:M * 300].view(M, 300)
    ref, _ = conv_ref(A, W, None, M, 0, 0)
    assert report('unaligned lda', C[:, 20:276].cpu().numpy(), ref)[0] < 5e-6
    # the margins keep their fill BYTEWISE (the stricter form of `== 0` on a zeroed buffer), the 20 floats behind the last row too
    margin = torch.ones(M * 300 + 20, dtype=torch.bool)
    margin[:M * 300].view(M, 300)[:, 20:276] = False
    assert G.margin_intact('flat', margin) and not bool(torch.isnan(C[:, 20:276]).any())
    G.check()


TN_CASES = [(128, 128, 128, 128, 1, 0), (360, 36, 80, 128, 3, 1), (5760, 180, 256, 512, 1, 1), (400, 40, 128, 128, 1, -1),
            (90, 9, 128, 128, 16, 7), (512, 512, 1025, 256, 1, 0), (77, 77, 20, 36, 1, 0),
            # second-generation kernel (gemm2.hip gemm_tn2: M >= 512, K, N >= 96, vector contract)
            (1600, 200, 128, 128, 16, 7), (1200, 40, 132, 260, 3, 1), (1440, 360, 256, 1024, 3, 1), (2000, 2000, 100, 96, 1, 0),
            (640, 20, 128, 128, 8, 4),
            # K no multiple of the 64-row tile: the taps are merged into K (GemmTnArgs::ktap); post-net conv bank shapes
            (720, 360, 128, 80, 8, 3), (800, 200, 128, 80, 5, 2), (360, 90, 80, 36, 2, 0)]


@pytest.mark.parametrize('tn2', ['0', '1'], ids=['gemm_tn', 'opt-in-tn2'])
@pytest.mark.parametrize('case', TN_CASES, ids=[str(c) for c in TN_CASES])
def test_gemm_tn(built_lib, case, tn2, monkeypatch):
    """Weight-gradient GEMM; with TACO_TN2=1 the eligible shapes run on the opt-in second-generation kernel (gemm2.hip)."""
    monkeypatch.setenv('TACO_TN2', tn2)
    M, T, N, K, taps, pad_l = case
    rng = np.random.default_rng(hash(case) % 2**31)
    A = rng.standard_normal((M, K))
    dY = rng.standard_normal((M, N))
    B = M // T
    ref = np.zeros((taps, K, N))
    x = A.reshape(B, T, K)
    y = dY.reshape(B, T, N)
    for j in range(taps):
        sh = j - pad_l
        for t in range(T):
            st = t + sh
            if 0 <= st < T:
                ref[j] += x[:, st].T @ y[:, t]
    G = Guarded({'dW': ((taps, K, N), torch.float32, 7.0)})
    dW = G['dW']
    built_lib.gemm_tn(dev(A), dev(dY), dW, M, N, K, taps=taps, T=T, pad_l=pad_l, accumulate=False)
    assert report('gemm_tn %s' % (case,), dW.cpu().numpy(), ref)[0] < 5e-6
    G.check()
    built_lib.gemm_tn(dev(A), dev(dY), dW, M, N, K, taps=taps, T=T, pad_l=pad_l, accumulate=True)
    assert report('  accumulate', dW.cpu().numpy(), 2 * ref)[0] < 5e-6
    G.check()


@pytest.mark.parametrize('B,T', [(2, 9), (3, 50), (32, 200)])
def test_bigru_fwd(built_lib, B, T):
    rng = np.random.default_rng(B * 100 + T)
    p = {}
    for d in ('fw', 'bw'):
        p['g/%s/gates/kernel' % d] = rng.uniform(-0.15, 0.15, (256, 256))
        p['g/%s/gates/bias' % d] = 1 + rng.uniform(-0.3, 0.3, 256)
        p['g/%s/candidate/kernel' % d] = rng.uniform(-0.15, 0.15, (256, 128))
        p['g/%s/candidate/bias' % d] = rng.uniform(-0.3, 0.3, 128)
    x = rng.standard_normal((B, T, 128))
    ref = on.bigru(x, p, 'g/')
    w = {k[2:]: dev(v) for k, v in p.items()}
    for fill in ('qnan', 'noise') if (B, T) == (3, 50) else ('qnan',):
        G = Guarded({'xg': ((B, T, 768), torch.float32, fill), 'out': ((B, T, 256), torch.float32, fill),
                     'ruc': ((B, T, 768), torch.float32, fill)})
        xg, out, ruc = G['xg'], G['out'], G['ruc']
        built_lib.bigru_fwd(dev(x), w, xg, out, ruc, B, T)
        r, m = report('bigru_fwd B=%d T=%d (%s)' % (B, T, fill), out.cpu().numpy(), ref)
        assert r < 2e-5 and m < 1e-4
        G.check('out', 'ruc')            # (xg is scratch: bounds only)
        assert bool(torch.isfinite(ruc).all())


def test_bernoulli(built_lib):
    G = Guarded({'out': ((1 << 20,), torch.uint8, 'ones'), 'odd': ((1001,), torch.uint8, 'ones')})
    out = G['out']
    built_lib.fill_bernoulli(out, 0.5, 123)
    G.check('out')
    a = out.cpu().numpy().copy()
    assert set(np.unique(a)) == {0, 1} and abs(a.mean() - 0.5) < 3e-3
    built_lib.fill_bernoulli(out, 0.5, 123)
    assert np.array_equal(a, out.cpu().numpy())
    built_lib.fill_bernoulli(out, 0.5, 124)
    b = out.cpu().numpy()
    assert abs((a == b).mean() - 0.5) < 3e-3           # independent streams
    built_lib.fill_bernoulli(out, 0.25, 9)
    assert abs(out.float().mean().item() - 0.25) < 3e-3
    odd = G['odd']
    built_lib.fill_bernoulli(odd, 1.0, 1)
    assert int(odd.sum()) == 1001
    G.check('out', 'odd')      # (the three bytes behind element 1000 kept their 255)


@pytest.mark.parametrize('gscale', [0.01, 30.0], ids=['noclip', 'clip'])
def test_clip_adam_step(built_lib, gscale):
    """Three steps.  Each step is held per element to the bounds tests/glue_ops.py derives (adam_ref: fp64 on the state the device
    holds before the step, with the kernel's fp32 constants 0.9f, 0.999f, 1 - 0.999f, 1e-8f and the host's float lr_t), each proved
    tighter here than the bar it replaces: 1e-4 (norm), 1e-5 (m, rel-L2), 1e-4 (v, rel-L2), 2e-6 (params, max abs).  The three-step
    chain is still compared with the independent fp64 oracle (fp64 constants) under those old bars."""
    from tests import glue_ops as go
    rng = np.random.default_rng(1)
    n = 100003
    p0 = rng.standard_normal(n)
    p = {'w': p0.copy()}
    m = {'w': np.zeros(n)}
    v = {'w': np.zeros(n)}
    G = Guarded({'P': ((n,), torch.float32, 'qnan'), 'm': ((n,), torch.float32, 'zeros'), 'v': ((n,), torch.float32, 'zeros'),
                 'scratch': ((256,), torch.float32, 'noise'), 'gnorm': ((1,), torch.float32, 'noise')})
    P, Mm, Vv, scratch, gn_out = G['P'], G['m'], G['v'], G['scratch'], G['gnorm']   # (m, v: the caller zeroes them)
    P.copy_(dev(p0))
    for step in (1, 2, 3):
        g = rng.standard_normal(n) * gscale
        before = [t.cpu().numpy().copy() for t in (P, Mm, Vv)]
        gn = on.clip_adam_step(p, {'w': g}, m, v, step, 5e-4)
        built_lib.clip_adam_step(P, dev(g), Mm, Vv, 5e-4, 5.0, step, scratch, gn_out)
        G.check('gnorm')
        r = go.adam_ref(before[0], g.astype(np.float32), before[1], before[2], 5e-4, 5.0, step)
        assert r['clipped'] == (gscale > 1) and abs(r['gn'] - gn) < 1e-6 * gn
        assert r['b_gn'] < 1e-4 * gn and np.linalg.norm(r['b_m']) < 1e-5 * np.linalg.norm(r['m'])
        assert np.linalg.norm(r['b_v']) < 1e-4 * np.linalg.norm(r['v']) and r['b_p'].max() < 2e-6
        for name, got, ref, bound in (('norm', gn_out.cpu().numpy().astype(np.float64), np.array([r['gn']]), np.array([r['b_gn']])),
                                      ('m', Mm.cpu().numpy().astype(np.float64), r['m'], r['b_m']),
                                      ('v', Vv.cpu().numpy().astype(np.float64), r['v'], r['b_v']),
                                      ('params', P.cpu().numpy().astype(np.float64), r['p'], r['b_p'])):
            err = np.abs(got - ref)
            print('  adam step %d %-6s worst |err| / bound %.3e' % (step, name, float((err / np.maximum(bound, 1e-300)).max())))
            assert (err <= bound).all(), 'adam step %d %s: %d elements outside their bound' % (step, name, int((err > bound).sum()))
    assert report('adam params', P.cpu().numpy(), p['w'])[1] < 2e-6
    assert report('adam m', Mm.cpu().numpy(), m['w'])[0] < 1e-5
    assert report('adam v', Vv.cpu().numpy(), v['w'])[0] < 1e-4
