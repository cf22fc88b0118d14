"""GPU: every load path, tile and epilogue of the GEMM kernels (gemm.hip, gemm2.hip) through the C ABI, against the fp64
references of tests/gemm_paths.py.  The case lists, the path each case must take and the error bound live there.

Every tensor is a flat buffer of one guarded arena (tests/poison.py), viewed at `base offset + pitch`.  Outputs start as NaN
(`qnan`; gemm_tn's dW as 7.0, or as random prior content where the call accumulates); the pitch padding of every INPUT is NaN
too, so a read past a row's extent poisons the result (exception: columns N..nld of the zero-padded weight rows of
taco_debug_conv_gemm_nld are zeros by contract).  After each call the whole arena outside the written region -- guard bands,
inputs, the pitch padding of C / Cpre / dW and the words in front of a base offset -- is bytewise what it was.

Bars: rel-L2 <= 5e-6 against fp64 (the bar of every GEMM test of tests/test_gpu_ops.py), and per element
gemm_paths.element_bound.  The worst figures per path are collected and, when GEMM_PATHS_ERRORS_OUT names a file, written there
(profiles/gemm_paths_errors.txt is such a file)."""
import os

import numpy as np
import pytest
import torch

from tests import gemm_forms as gf
from tests import gemm_paths as gp
from tests.poison import Guarded

pytestmark = pytest.mark.gpu

STATS = {}      # path label -> [cases, worst rel-L2, worst |err| / element bound]


def write_error_table():
    """The whole table from STATS, the one place that writes it: the rows of this file, then those of tests/test_gpu_gemm_forms.py
    under a comment line of their own.  Both modules call it when they end, so the file is complete after whichever ends last."""
    out = os.environ.get('GEMM_PATHS_ERRORS_OUT')
    if not out or not STATS:
        return
    row = lambda k: '%-18s %6d %12.3e %12.3e\n' % (k, STATS[k][0], STATS[k][1], STATS[k][2])
    forms = [k for k in sorted(STATS) if k in gf.FORM_LABELS]
    with open(out, 'w') as f:
        f.write('# tests/test_gpu_gemm_paths.py: per path label, cases run, worst rel-L2 against fp64 (bar 5e-6) and worst\n'
                '# |got - ref| / element bound (bar 1; tests/gemm_paths.py element_bound)\n')
        f.write('%-18s %6s %12s %12s\n' % ('path', 'cases', 'rel-L2', 'elem-ratio'))
        f.writelines(row(k) for k in sorted(STATS) if k not in gf.FORM_LABELS)
        if forms:
            f.write('# tests/test_gpu_gemm_forms.py: the forms only the model reaches, same columns\n')
            f.writelines(row(k) for k in forms)


@pytest.fixture(scope='module', autouse=True)
def _error_table():
    yield
    write_error_table()


def judge(label, what, got, ref, n, S, g):
    """both bars; prints the figures before it asserts"""
    got = got.astype(np.float64)
    assert np.isfinite(got).all(), '%s: the written region holds poison (%d non-finite)' % (what, int((~np.isfinite(got)).sum()))
    rel = float(np.linalg.norm(got - ref) / (np.linalg.norm(ref) + 1e-300))
    bound = gp.element_bound(n, S, g, ref)
    ratio = np.abs(got - ref) / np.maximum(bound, 1e-300)
    worst = float(ratio.max())
    at = np.unravel_index(int(ratio.argmax()), ratio.shape)
    print('  %-34s %-16s rel-L2 %.3e  worst element %.3e of its bound at %s' % (what, label, rel, worst, (at,)))
    s = STATS.setdefault(label, [0, 0.0, 0.0])
    s[0], s[1], s[2] = s[0] + 1, max(s[1], rel), max(s[2], worst)
    assert rel <= 5e-6, '%s: rel-L2 %.3e' % (what, rel)
    assert worst <= 1.0, '%s: element %s is off by %.3e, %.2f x its bound' % (what, at, float(np.abs(got - ref)[at]), worst)


class Flat:
    """Flat buffers of one guarded arena.  spec: name -> (floats, fill) for float buffers, (bytes, 'ones', 'u8') for bytes."""

    def __init__(self, spec, device='cuda'):
        self.device = device
        gs = {}
        for name, s in spec.items():
            gs[name] = ((s[0],), torch.uint8 if len(s) > 2 else torch.float32, s[1])
        self.G = Guarded(gs, device=device)
        self.spec = spec
        self.written = torch.zeros(self.G.arena.total, dtype=torch.bool, device=device)

    def buf(self, name):
        return self.G[name]

    def put(self, name, a, off, ld):
        """rows of `a` (R, C) at float offset `off`, pitch `ld`"""
        R, C = a.shape
        t = torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(self.device)
        self.G[name][off:off + R * ld].view(R, ld)[:, :C] = t
        return self.G[name][off:]

    def put_vec(self, name, a, off):
        self.G[name][off:off + a.size] = torch.as_tensor(np.ascontiguousarray(a).reshape(-1)).to(self.device, self.G[name].dtype)
        return self.G[name][off:]

    def out(self, name, off, R, C, ld):
        """marks (R, C) at `off`, pitch `ld`, as the region the call may write; returns the base pointer view"""
        o, n = self.G.arena.spans[name]
        assert off + (R - 1) * ld + C <= n
        self.written[o + off:o + off + (R - 1) * ld + C].as_strided((R, C), (ld, 1)).fill_(True)
        return self.G[name][off:]

    def get(self, name, off, R, C, ld):
        return self.G[name][off:off + (R - 1) * ld + C].as_strided((R, C), (ld, 1)).cpu().numpy()

    def _sync(self):
        if self.device == 'cuda':
            torch.cuda.synchronize()

    def snapshot(self):
        self._sync()
        self.snap = self.G.arena.raw.clone()

    def check_untouched(self):
        self._sync()
        self.G.check()                                                      # guard bands, with the place of the damage
        keepm = ~self.written
        same = self.G.arena.raw[keepm] == self.snap[keepm]
        if not bool(same.all()):
            idx = torch.nonzero(keepm)[~same][0].item()
            where = [(n, idx - o) for n, (o, sz) in self.G.arena.spans.items() if o <= idx < o + sz]
            raise AssertionError('a word outside the written region changed: %s (arena word %d)' % (where, idx))


def _operands(c_id, M, N, K, taps):
    rng = np.random.default_rng(gp.seed_of(c_id))
    f = np.float32
    return dict(A=rng.standard_normal((M, K)).astype(f), W=(rng.standard_normal((taps, K, N)) / np.sqrt(K * taps)).astype(f),
                bias=rng.standard_normal(N).astype(f), scale=rng.standard_normal(N).astype(f), shift=rng.standard_normal(N).astype(f),
                res=rng.standard_normal((M, N)).astype(f), keep=rng.integers(0, 2, (M, N)).astype(np.uint8))


def run_nn(lib, c, monkeypatch, ref_cache=None):
    """one taco_conv_gemm call for row `c` (gemm_paths.NN) with both bars, the route and the arena checks"""
    if c.g2 != '':
        monkeypatch.setenv('TACO_GEMM2_MIN_TILES', c.g2)
    monkeypatch.setenv('TACO_GEMM2_BF16X', c.bx)
    M, T, N, K, taps = c.M, c.T, c.N, c.K, c.taps
    d = _operands(c.id.split('/')[0], M, N, K, taps)
    on = {o: o in c.opts for o in 'bkshrp'}
    F = Flat({'A': (c.offA + M * c.lda, 'qnan'), 'W': (c.offW + taps * K * c.ldw, 'qnan'), 'bias': (c.offB + N, 'qnan'),
              'scale': (c.offB + N, 'qnan'), 'shift': (c.offB + N, 'qnan'), 'res': (c.offR + M * c.ldr, 'qnan'),
              'keep': (c.offK + M * N, 'ones', 'u8'), 'C': (c.offC + M * c.ldc, 'qnan'), 'Cpre': (c.offP + M * c.ldc, 'qnan')})
    A = F.put('A', d['A'], c.offA, c.lda)
    W = F.put('W', d['W'].reshape(taps * K, N), c.offW, c.ldw)
    bias = F.put_vec('bias', d['bias'], c.offB) if on['b'] else None
    scale = F.put_vec('scale', d['scale'], c.offB) if on['s'] else None
    shift = F.put_vec('shift', d['shift'], c.offB) if on['h'] else None
    res = F.put('res', d['res'], c.offR, c.ldr) if on['r'] else None
    keep = F.put_vec('keep', d['keep'], c.offK) if on['k'] else None
    C = F.out('C', c.offC, M, N, c.ldc)
    Cpre = F.out('Cpre', c.offP, M, N, c.ldc) if on['p'] else None
    label = gp.nn_row_path(c, A.data_ptr(), W.data_ptr(), C.data_ptr(), None if Cpre is None else Cpre.data_ptr(),
                           None if res is None else res.data_ptr(), None if keep is None else keep.data_ptr())
    assert label == c.path, '%s: the restated dispatch gives %s for the real pointers, the case list says %s' % (c.id, label, c.path)
    F.snapshot()
    lib.weight_image(None)
    lib.debug_gemm2_window(0, 1 << 30)
    lib.conv_gemm(A, W, C, M, N, K, taps=taps, T=T, pad_l=c.pad_l, act=c.act, bias=bias, scale=scale, shift=shift, residual=res,
                  keep=keep, Cpre=Cpre, lda=c.lda, ldw=c.ldw, ldc=c.ldc, ldr=c.ldr)
    took = lib.debug_gemm2_window(0, 1 << 30)
    assert took == (1 if label.startswith('g2.') else 0), '%s: %d launches went to gemm2.hip' % (c.id, took)
    F.check_untouched()
    key = (c.id.split('/')[0], 'ref')
    if ref_cache is not None and key in ref_cache:
        ref, pre, S = ref_cache[key]
    else:
        ref, pre, S = gp.nn_ref(d['A'], d['W'], d['bias'] if on['b'] else None, T, c.pad_l, c.act, d['keep'] if on['k'] else None,
                                d['scale'].astype(np.float64) if on['s'] else None, d['shift'].astype(np.float64) if on['h'] else None,
                                d['res'].astype(np.float64) if on['r'] else None)
        if ref_cache is not None:
            ref_cache[key] = (ref, pre, S)
    gk = 2.0 if on['k'] else 1.0
    g = gk * (np.abs(d['scale'].astype(np.float64)) if on['s'] else 1.0)
    judge(label, c.id + ' C', F.get('C', c.offC, M, N, c.ldc), ref, taps * K, S, g)
    if on['p']:
        judge(label, c.id + ' Cpre', F.get('Cpre', c.offP, M, N, c.ldc), pre, taps * K, S, gk)


@pytest.mark.parametrize('c', gp.NN_LOAD_CASES, ids=[c.id for c in gp.NN_LOAD_CASES])
def test_nn_load_paths(built_lib, c, monkeypatch):
    """(a) conv_gemm_kernel<1, 1, VA, VW>: each way to lose the vector contract of A or of W by itself, both, neither; tap shifts
    that leave the sequence on one side for every row (taps 2, pad_l 3) and a negative pad.  Measured on an MI355X: rel-L2 <=
    2.2e-7, elements within 0.18 of their bound except one at 0.98 (`v-neg-pad`, row 25: every tap falls outside the sequence, the
    output is tanh(bias) of a bias of -0.0034, and tanh_f's absolute error of ~1e-7 is many units in the last place there)."""
    run_nn(built_lib, c, monkeypatch)


@pytest.mark.parametrize('c', gp.NN_BIG_CASES, ids=[c.id for c in gp.NN_BIG_CASES])
def test_nn_big_tile(built_lib, c, monkeypatch):
    """(b) conv_gemm_kernel<2, 2, VA, VW>: 24 x 16 = 384 tiles of 128 x 128, one case per flags class"""
    assert gp.nn_tile(c.M, c.N) == 128
    run_nn(built_lib, c, monkeypatch)


_EPI_REFS = {}


@pytest.mark.parametrize('engine', gp.EPI_ENGINES, ids=[g[0] for g in gp.EPI_ENGINES])
@pytest.mark.parametrize('e', gp.EPI_CASES, ids=[e.id for e in gp.EPI_CASES])
def test_nn_epilogue_options(built_lib, e, engine, monkeypatch):
    """(c) bias / activation / keep / affine (scale only, shift only, both) / residual / Cpre on gemm.hip's epilogue and on the
    float4, shifted and scalar epilogues of gemm2.hip in both MFMA forms.  Cpre is written with the pitch of C (ldc), keep is
    read with pitch N (include/taco_hip.h taco_conv_gemm)."""
    run_nn(built_lib, gp.epi_as_nn(e, engine), monkeypatch, _EPI_REFS)


@pytest.mark.parametrize('c', gp.NLD_CASES, ids=[c.id for c in gp.NLD_CASES])
def test_nn_padded_weight_rows(built_lib, c, monkeypatch):
    """(d) taco_debug_conv_gemm_nld: weight rows zero-padded to nld columns, nld == ldw and nld < ldw (columns nld..ldw are NaN:
    never loaded), every ldc % 4, activation with the bias off"""
    monkeypatch.setenv('TACO_GEMM2_MIN_TILES', c.g2)
    monkeypatch.setenv('TACO_GEMM2_BF16X', c.bx)
    M, K, N = gp.NLD_SHAPE['M'], gp.NLD_SHAPE['K'], c.N
    d = _operands(c.id, M, N, K, 1)
    F = Flat({'A': (M * K, 'qnan'), 'W': (K * c.ldw, 'qnan'), 'bias': (N, 'qnan'), 'C': (M * c.ldc, 'qnan')})
    A = F.put('A', d['A'], 0, K)
    Wp = np.zeros((K, c.nld), np.float32)
    Wp[:, :N] = d['W'][0]
    W = F.put('W', Wp, 0, c.ldw)
    bias = F.put_vec('bias', d['bias'], 0) if c.bias else None
    C = F.out('C', 0, M, N, c.ldc)
    label = gp.nld_path(c, A.data_ptr(), W.data_ptr(), C.data_ptr())
    assert label == c.path
    F.snapshot()
    built_lib.weight_image(None)
    built_lib.debug_gemm2_window(0, 1 << 30)
    built_lib.conv_gemm_nld(A, W, C, M, N, K, c.nld, c.ldw, c.ldc, act=c.act, bias=bias)
    assert built_lib.debug_gemm2_window(0, 1 << 30) == (1 if label.startswith('g2.') else 0)
    F.check_untouched()
    ref, _, S = gp.nn_ref(d['A'], d['W'], d['bias'] if c.bias else None, M, 0, c.act)
    judge(label, c.id, F.get('C', 0, M, N, c.ldc), ref, K, S, 1.0)


def _gemm_labels(lib, call):
    """profile labels (ring 2: the GEMM family) of the launches `call` makes"""
    lib.profile_read(2)
    lib.profile_enable(4)
    try:
        call()
        torch.cuda.synchronize()
        return lib.profile_labels(2)
    finally:
        lib.profile_enable(0)
        lib.profile_read(2)


@pytest.mark.parametrize('c', gp.KSPLIT_CASES, ids=[c.id for c in gp.KSPLIT_CASES])
def test_nn_forced_ksplit(built_lib, c, monkeypatch):
    """(e) TACO_KSPLIT: chunk edges in the middle of a tap, a short last chunk, a K tail inside a chunk.  The S that runs is read
    from the launch's profile label and must be what the restatement says (a forced S out of range is ignored); `noise` and
    `qnan` slabs give bit-equal results."""
    monkeypatch.setenv('TACO_KSPLIT', str(c.force))
    M, T, N, K, taps = c.M, c.T, c.N, c.K, c.taps
    d = _operands(c.id, M, N, K, taps)
    S_plan = gp.ksplit_plan(M, N, K, taps, c.slabs * M * N, c.force)[0]
    assert S_plan == c.S
    outs = []
    for fill in ('noise', 'qnan'):
        F = Flat({'A': (M * K, 'qnan'), 'W': (taps * K * N, 'qnan'), 'bias': (N, 'qnan'), 'slabs': (c.slabs * M * N, fill), 'C': (M * N, 'qnan')})
        A, W, bias = F.put('A', d['A'], 0, K), F.put('W', d['W'].reshape(taps * K, N), 0, N), F.put_vec('bias', d['bias'], 0)
        C = F.out('C', 0, M, N, N)
        slabs = F.out('slabs', 0, 1, c.slabs * M * N, c.slabs * M * N)
        assert gp.nn_flags(A.data_ptr(), K, W.data_ptr(), N, N, K) == 3
        F.snapshot()
        built_lib.weight_image(None)
        labels = _gemm_labels(built_lib, lambda: built_lib.conv_gemm_ksplit(A, W, C, M, N, K, slabs, taps=taps, T=T, pad_l=c.pad_l, act=c.act, bias=bias))
        assert labels == ['nn-ksplit S=%d M=%d N=%d K=%d taps=%d' % (c.S, M, N, K, taps)], labels
        F.check_untouched()
        outs.append(F.get('C', 0, M, N, N))
    ref, _, S = gp.nn_ref(d['A'], d['W'], d['bias'], T, c.pad_l, c.act)
    # the slab sum adds S partial sums in fp32: S - 1 more roundings of the running sum, inside the (n + 16) of the bound
    judge(c.path, c.id, outs[0], ref, taps * K, S, 1.0)
    assert np.array_equal(outs[0].view(np.int32), outs[1].view(np.int32)), 'the result depends on what the slabs held'


@pytest.mark.parametrize('c', gp.TN_PATH_CASES, ids=[c.id for c in gp.TN_PATH_CASES])
def test_tn_paths(built_lib, c, monkeypatch):
    """(f) gemm_tn_kernel<1, 1, ..> and <2, 2, ..> in its five forms each: pitches and base offsets of A, dY and dW, K and N
    tails, merged and unmerged taps, one split and several with a short last chunk, a 7.0 fill that the call must zero first
    and random prior content that it must add to.  splits and bm are read from the launch's profile label."""
    monkeypatch.setenv('TACO_TN2', '0')
    monkeypatch.setenv('TACO_GEMM2_BF16X', c.bx)
    monkeypatch.setenv('TACO_TN_MERGE_TAPS', c.merge)
    monkeypatch.setenv('TACO_DETERMINISTIC', c.det)
    M, T, N, K, taps = c.M, c.T, c.N, c.K, c.taps
    rng = np.random.default_rng(gp.seed_of(c.id))
    A = rng.standard_normal((M, K)).astype(np.float32)
    dY = rng.standard_normal((M, N)).astype(np.float32)
    dW0 = rng.standard_normal((taps * K, N)).astype(np.float32)
    F = Flat({'A': (c.offA + M * c.lda, 'qnan'), 'Y': (c.offY + M * c.ldy, 'qnan'), 'dW': (c.offW + taps * K * c.ldw, 7.0)})
    At, Yt = F.put('A', A, c.offA, c.lda), F.put('Y', dY, c.offY, c.ldy)
    if c.acc:       # prior content everywhere, the pitch padding included (it must survive bytewise)
        F.buf('dW').copy_(torch.as_tensor(rng.standard_normal(F.buf('dW').numel()).astype(np.float32)).cuda())
        F.put('dW', dW0, c.offW, c.ldw)
    dWt = F.out('dW', c.offW, taps * K, N, c.ldw)
    plan = gp.tn_case_plan(c, At.data_ptr(), Yt.data_ptr())
    assert (plan['label'], plan['merged'], plan['splits']) == (c.path, c.merged, c.splits)
    F.snapshot()
    labels = _gemm_labels(built_lib, lambda: built_lib.gemm_tn(At, Yt, dWt, M, N, K, taps=taps, T=T, pad_l=c.pad_l, accumulate=c.acc,
                                                               lda=c.lda, ldy=c.ldy, ldw=c.ldw))
    assert labels == ['tn M=%d N=%d K=%d taps=%d batch=1 splits=%d bm=%d' % (M, N, plan['K'], plan['taps'], plan['splits'], plan['bm'])], labels
    F.check_untouched()
    ref, S = gp.tn_ref(A, dY, taps, T, c.pad_l)
    ref, S = ref.reshape(taps * K, N), S.reshape(taps * K, N)
    if c.acc:       # the prior content is one more term of every sum
        ref, S = ref + dW0, S + np.abs(dW0)
    judge(c.path, c.id, F.get('dW', c.offW, taps * K, N, c.ldw), ref, M, S, 1.0)
