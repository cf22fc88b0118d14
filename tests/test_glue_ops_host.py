"""CPU: what tests/glue_ops.py claims, proved without a GPU -- the backward references against torch fp64 autograd, the case lists
against the restated launch geometry (every label reached, every seam with matching ids on both sides), the planted ties, zeros and
clamps, and the new doors' names, argument checks and documents."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import glue_ops as go

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOORS = ('embedding', 'embedding_bwd', 'highway_combine', 'highway_combine_bwd', 'act_bwd', 'affine_act_bwd', 'colsum_batched', 'mask_rows',
         'center_rows', 'mask_pos', 'zero_tail_rows', 'add', 'l1_loss', 'transpose_batch', 'sumsq')
t64 = lambda a, grad=False: torch.tensor(np.asarray(a, np.float64), requires_grad=grad)


# ------------------------------------------------------------------------------------------------------------------
# references against autograd

def test_embedding_bwd_ref_is_the_gradient_of_index_select():
    c = go.EMB_CASES[5]
    rng = go.rng_of(c.id)
    ids, dout = go.emb_ids(c), rng.standard_normal((c.rows, c.width))
    prior = rng.standard_normal((c.V, c.width))
    table = t64(rng.standard_normal((c.V, c.width)), True)
    out = table.index_select(0, torch.tensor(go.clamp_ids(ids, c.V)))
    assert np.array_equal(out.detach().numpy(), go.embedding_ref(table.detach().numpy(), ids))
    out.backward(t64(dout))
    ref, tot, n, S = go.embedding_bwd_ref(dout, ids, prior)
    assert np.allclose(tot, table.grad.numpy(), rtol=1e-12, atol=1e-12) and np.array_equal(ref, prior + tot)
    assert n.sum() == c.rows and n[go.EMB_NEVER(c.V)] == 0 and (S >= np.abs(tot) - 1e-9).all()
    # the chain form of n: never above the row count + passes, 0 where no row names the id, far below the count where one id owns most rows
    big = go.EMB_CASES[10]
    ids_b, geo = go.emb_ids(big), go.emb_geometry(big.rows, big.det)
    z = np.zeros((big.V, 4))
    n_rows, n_chain = go.embedding_bwd_ref(np.zeros((big.rows, 4)), ids_b, z)[2], go.embedding_bwd_ref(np.zeros((big.rows, 4)), ids_b, z, geo)[2]
    assert big.rows == go.EMB_BIG_ROWS and (n_chain <= n_rows + 2).all() and ((n_chain == 0) == (n_rows == 0)).all()
    assert n_rows[0] > 100000 and n_chain[0] < 1100 and n_rows[go.EMB_SEAM(big.V)] < 1000


def test_highway_refs_against_autograd():
    th, x, dy = go.highway_operands(33)
    tht, xt = t64(th, True), t64(x, True)
    t, h_pre = tht[:, :128], tht[:, 128:]
    # the stored candidate is a ReLU output: dh goes through the ReLU that produced it (H > 0); sigmoid' = T (1 - T) on the stored gate
    y = h_pre * t + xt * (1 - t)
    ref_y, S = go.highway_ref(th, x)
    assert np.allclose(y.detach().numpy(), ref_y, rtol=1e-13, atol=1e-13) and (S >= np.abs(ref_y) - 1e-12).all()
    y.backward(t64(dy))
    r = go.highway_bwd_ref(th, x, dy)
    tt, hh = th[:, :128].astype(np.float64), th[:, 128:].astype(np.float64)
    assert np.allclose(r['dx'], xt.grad.numpy(), rtol=1e-13, atol=1e-13)
    assert np.allclose(r['dt'], tht.grad.numpy()[:, :128] * tt * (1 - tt), rtol=1e-12, atol=1e-13)
    assert np.allclose(r['dh'], tht.grad.numpy()[:, 128:] * (hh > 0), rtol=1e-13, atol=1e-13)
    assert (r['dh'][r['zero']] == 0).all() and r['zero'][:, 2:5].all() and not r['zero'][:, 0:2].any()


@pytest.mark.parametrize('act', go.ACTS)
def test_act_bwd_ref_against_autograd(act):
    rng = np.random.default_rng(3)
    z = rng.standard_normal(501)
    z[::9] = -abs(z[::9])
    zt = t64(z, True)
    y = {'none': zt, 'relu': torch.relu(zt), 'sigmoid': torch.sigmoid(zt), 'tanh': torch.tanh(zt)}[act]
    keep = (rng.random(501) < 0.5).astype(np.uint8)
    dy = rng.standard_normal(501)
    (y * t64(keep) * 2).backward(t64(dy))
    dz, S, zero = go.act_bwd_ref(y.detach().numpy(), dy, keep, act)
    assert np.allclose(dz, zt.grad.numpy(), rtol=1e-12, atol=1e-14) and (dz[zero] == 0).all() and (S >= np.abs(dz) - 1e-12).all()
    assert np.allclose(go.act_bwd_ref(y.detach().numpy(), dy, None, act)[0] * keep * 2, dz, rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize('act', ('none', 'relu'))
def test_affine_act_bwd_ref_against_autograd(act):
    c = go.AffCase('host', 33, 80, act, False)
    pre, gamma, dy, pg, pb = go.aff_operands(c)
    rs = 1.0 / np.sqrt(1.0 + 1e-3)
    # forward: pre = act(z); out = pre gamma rs + beta.  dz is the gradient at z, through the activation that produced pre
    z = t64(np.where(pre > 0, pre, -1.0) if act == 'relu' else pre, True)
    g, b = t64(gamma, True), t64(np.zeros(c.N), True)
    p = torch.relu(z) if act == 'relu' else z
    (p * g * rs + b).backward(t64(dy))
    r = go.affine_act_bwd_ref(np.where(pre > 0, pre, 0) if act == 'relu' else pre, gamma, dy, act, pg, pb)
    assert np.allclose(r['dz'], z.grad.numpy(), rtol=1e-12, atol=1e-14)
    assert np.allclose(r['sum_g'], g.grad.numpy(), rtol=1e-12, atol=1e-12) and np.allclose(r['sum_b'], b.grad.numpy(), rtol=1e-12, atol=1e-12)
    assert np.array_equal(r['dgamma'], pg + r['sum_g']) and r['n'] == c.M
    assert abs(float(go.RS32) - rs) <= go.K_RS * go.U * rs


def test_center_rows_removes_exactly_what_the_softmax_backward_ignores():
    """d alignments[s] = <memory[s], q> enters the softmax backward ds = a (da - sum a da), which ignores a constant added to da over s:
    centring the memory rows over s < n changes da by exactly such a constant, and leaves no common component behind"""
    c = go.RowCase('host', 37, 260)
    x, length = go.row_operands(c)
    out, bound, zero = go.center_rows_ref(x, length)
    rng = np.random.default_rng(5)
    q = rng.standard_normal(c.C)
    for b in range(go.ROW_B):
        n = int(np.clip(length[b], 1, c.T))
        assert (out[b, n:] == 0).all() and zero[b, n:].all() and not zero[b, :n].any()
        assert np.abs(out[b, :n].mean(0)).max() <= 1e-12 * np.abs(x[b, :n]).max()
        a = np.exp(rng.standard_normal(n))
        a /= a.sum()
        da0, da1 = x[b, :n].astype(np.float64) @ q, out[b, :n] @ q
        ds = lambda da: a * (da - (a * da).sum())
        assert np.allclose(da0 - da1, (da0 - da1)[0], rtol=0, atol=1e-9 * np.abs(da0).max())      # a constant over s
        assert np.allclose(ds(da0), ds(da1), rtol=0, atol=1e-9 * np.abs(da0).max())
    big = go.ROW_BIG_MEAN[1]
    assert np.abs(x[big]).min() > 900 and np.abs(out[big]).max() < 0.1 and (bound[big] < 2e-3).all() and (bound[big] > 5e-5).all()


def test_l1_transpose_colsum_and_adam_references():
    a, b = go.l1_operands('host', 0, 37, 160)
    s, g = go.l1_ref(a, b)
    d = a.astype(np.float64) - b
    assert s == np.abs(d).sum() and set(np.unique(g)) == {-1.0, 0.0, 1.0} and not np.signbit(g[d == 0]).any()
    src = np.arange(3 * 4 * 5, dtype=np.float32).reshape(3, 4, 5)
    tr = go.transpose_ref(src)
    assert tr.shape == (3, 5, 4) and all(np.array_equal(tr[t], src[2 - t].T) for t in range(3))
    x = np.arange(2 * 3 * 6, dtype=np.float32).reshape(6, 6)
    out, S = go.colsum_ref(x, 2, 3, 4)
    assert np.array_equal(out[1], x[3:6, :4].sum(0)) and np.array_equal(S, out)
    # Adam: the reference is the textbook update (torch.optim.Adam's algebra in the TF form), and its constants are the fp32 ones
    c = go.ADAM_CASES[4]
    p, gr, m, v, cap = go.adam_operands(c)
    r = go.adam_ref(p, gr, m, v, go.ADAM_LR, cap, c.step)
    gn = np.linalg.norm(gr.astype(np.float64))
    gi = gr.astype(np.float64) * cap / gn
    m1, v1 = 0.9 * m + 0.1 * gi, 0.999 * v + 0.001 * gi * gi
    lr_t = go.ADAM_LR * np.sqrt(1 - 0.999 ** c.step) / (1 - 0.9 ** c.step)
    assert r['clipped'] and abs(r['gn'] - gn) < 1e-9 and np.allclose(r['m'], m1, rtol=1e-6) and np.allclose(r['v'], v1, rtol=1e-4, atol=1e-12)
    assert np.allclose(r['p'], p - lr_t * m1 / (np.sqrt(v1) + 1e-8), rtol=0, atol=1e-6)
    # the fp32 constants: both differences are exact in fp32, and 1 - 0.999f is 1.3e-5 away from 0.001 (a constant's rounding the old 1e-4 bar of v paid for)
    assert float(np.float32(1) - np.float32(0.999)) == 1.0 - float(np.float32(0.999)) and float(np.float32(1) - np.float32(0.9)) == 1.0 - float(np.float32(0.9))
    assert 1e-5 < abs(float(np.float32(1) - np.float32(0.999)) / 0.001 - 1) < 5e-5
    # derived bounds are tighter than the bars they replace: 1e-4 (norm), 1e-5 (m, rel-L2), 1e-4 (v, rel-L2), 2e-6 (params, max abs)
    for cc in go.ADAM_CASES:
        p, gr, m, v, cap = go.adam_operands(cc)
        r = go.adam_ref(p, gr, m, v, go.ADAM_LR, cap, cc.step)
        assert r['b_gn'] <= 1e-5 * max(r['gn'], 1e-30) and np.linalg.norm(r['b_m']) < 1e-5 * np.linalg.norm(r['m'])
        assert np.linalg.norm(r['b_v']) < 1e-4 * np.linalg.norm(r['v']) and r['b_p'].max() < 2e-6


# ------------------------------------------------------------------------------------------------------------------
# the case lists against the restated geometry

def _all_labels():
    labels = set()
    for c in go.EMB_CASES:
        labels |= go.emb_labels(c.rows, c.det)
    for c in go.AFF_CASES:
        labels |= go.col_labels(c.M, c.det)
    for c in go.ROW_CASES:
        labels |= go.center_labels(c.T, c.C)
    for c in go.L1_CASES:
        for t in c.terms:
            if t:
                labels |= go.l1_labels(t[0], t[1], t[2] if t[3] else t[1])
    for n in go.SUMSQ_N:
        labels |= go.sumsq_labels(n)
    return labels


def test_case_lists_reach_every_geometry_label():
    assert _all_labels() == go.GEOMETRY_LABELS
    assert {n for c in go.ADAM_CASES for n in go.sumsq_labels(c.n)} >= {'sumsq.tail-only', 'sumsq.rem', 'sumsq.rem+tail', 'sumsq.unroll+tail', 'sumsq.unroll+rem+tail'}


def test_geometry_restatement_on_known_points():
    g = go.emb_geometry(go.EMB_BIG_ROWS, False)
    assert g['segs'] == 32 and g['rps'] == 4097 and g['passes'] == [2] * 31 + [1] and len(g['seams']) == 31 and len(g['pass_seams']) == 31
    assert go.emb_geometry(8200, True)['passes'] == [3] and go.emb_geometry(4096, True)['passes'] == [1] and go.emb_geometry(257, False)['segs'] == 2
    assert go.emb_geometry(256, False)['segs'] == 1 and go.emb_geometry(1000, False)['rps'] == 250
    assert go.col_geometry(1000, False) == dict(chunks=32, rpb=32, lane_rows=8, ragged=True) and go.col_geometry(1000, True)['chunks'] == 1
    assert go.col_geometry(33, False)['rpb'] == 17 and go.col_geometry(64, False) == dict(chunks=2, rpb=32, lane_rows=8, ragged=False)
    assert go.center_geometry(5, 260) == dict(per=2, quarters=[(0, 2), (2, 4), (4, 5), (6, 5)], empty=1, inactive_quads=63)
    assert go.center_geometry(37, 512)['quarters'] == [(0, 10), (10, 20), (20, 30), (30, 37)] and go.center_geometry(3, 256)['empty'] == 1
    assert go.l1_geometry(9001, 5, 8) == dict(rows_per_wave=2, busy_blocks=512, pieces=1, lane_terms=8)
    assert go.l1_geometry(37, 1025, 1028) == dict(rows_per_wave=1, busy_blocks=3, pieces=5, lane_terms=20)
    s = go.sumsq_geometry(4 * 262145 + 2)
    assert (s['unrolled'], s['rem'], s['both'], s['tail']) == (1, 1, 1, 2) and go.sumsq_geometry(4 * 196607 + 3)['unrolled'] == 0
    assert go.sumsq_geometry(4 * 196609 + 1)['unrolled'] == 1 and go.sumsq_geometry(4 * 196609 + 1)['both'] == 0


@pytest.mark.parametrize('c', go.EMB_CASES, ids=[c.id for c in go.EMB_CASES])
def test_embedding_cases_hold_what_they_say(c):
    ids = go.emb_ids(c)
    cid = go.clamp_ids(ids, c.V)
    g = go.emb_geometry(c.rows, c.det)
    assert ids.dtype == np.int32 and len(ids) == c.rows
    for s in g['seams'] + g['pass_seams']:            # a seam has the same id on both sides: both sides add to the same table row
        assert 0 < s < c.rows and cid[s - 1] == cid[s]
    if c.pattern == 'one':
        assert (ids == go.EMB_ONE(c.V)).all()
    else:
        if c.rows > 2:
            assert (ids < 0).any() and (ids >= c.V).any()
        if c.V > 1:
            assert not (cid == go.EMB_NEVER(c.V)).any()
        if c.pattern == 'pad90' and c.rows >= 255:
            assert 0.85 < (cid == 0).mean() < 0.97
    if g['segs'] > 1:
        assert all(p >= 1 for p in g['passes'])        # no empty segment: every seam is a real one


def test_the_case_lists_cover_what_the_issue_lists():
    assert {c.V for c in go.EMB_CASES} == {1, 33} and {c.width for c in go.EMB_CASES} == {16, 256, 260, 1024}
    assert {c.rows for c in go.EMB_CASES if not c.det} >= {1, 255, 256, 257, 1000, 131078}
    assert {c.rows for c in go.EMB_CASES if c.det} >= {4096, 4097, 8200} and {c.pattern for c in go.EMB_CASES} == {'one', 'pad90', 'mixed'}
    assert {(c.n, c.act, c.keep, c.inplace) for c in go.ACT_CASES} >= {(n, a, k, i) for n in (1, 1001) for a in go.ACTS for k in (0, 1) for i in (0, 1)}
    assert {(c.act, c.keep) for c in go.ACT_CASES if c.n == go.ACT_BIG} == {(a, k) for a in go.ACTS for k in (False, True)}
    assert {(c.M, c.N, c.act) for c in go.AFF_CASES} >= {(M, N, a) for M in (1, 31, 33, 129, 1000) for N in (80, 128, 132, 256) for a in ('none', 'relu')}
    assert {c.det for c in go.AFF_CASES} == {False, True}
    assert {c.T for c in go.COLSUM_CASES} == {1, 3, 4, 5, 32, 41} and {c.N for c in go.COLSUM_CASES} >= {16, 80, 130} and any(c.ld > c.N for c in go.COLSUM_CASES)
    assert {(c.B, c.T, c.N) for c in go.COLSUM_CASES} >= {(1, 5, 512), (1, 32, 256)}
    assert {(c.T, c.C) for c in go.ROW_CASES} == {(T, C) for T in (1, 2, 3, 5, 37) for C in (256, 260, 512)}
    assert list(go.row_lengths(5)) == [-1, 0, 1, 4, 5, 8]
    assert all(c.ldg != c.ldy and c.ldy != c.cols for c in go.MASK_POS_CASES[1:4]) and {c.scale for c in go.MASK_POS_CASES} == {1, 2}
    assert {c.C0 for c in go.ZERO_TAIL_CASES} == {160, 2050} and {c.C1 for c in go.ZERO_TAIL_CASES} == {None, 160, 2050}
    assert set(go.TAIL_LEN) >= {0, 1, go.TAIL_TD} and (go.TAIL_LEN > go.TAIL_TD).any()
    shapes = {t[:3] for c in go.L1_CASES for t in c.terms if t}
    assert shapes == {(1, 1025, 1028), (37, 1025, 1028), (37, 160, 160), (9001, 5, 8), (3, 400, 400)}
    assert {(t[:3], t[3]) for c in go.L1_CASES for t in c.terms if t} >= {(s, g) for s in shapes for g in (True, False)}
    jobs = [j for js in go.TRANSPOSE_CASES.values() for j in js]
    assert {j.taps for j in jobs} == {1, 3} and {(j.K, j.N) for j in jobs} == {(1, 1), (31, 33), (80, 1025), (256, 128)}
    assert any(j.ldi for j in jobs) and any(not j.ldi for j in jobs) and {len(js) for js in go.TRANSPOSE_CASES.values()} == {1, go.MAX_TRANSPOSE_BATCH}
    assert all(j.taps == 1 for j in jobs if j.ldi or j.ldo)
    assert set(go.SUMSQ_N) == {1, 3, 4, 5, 100003, 4 * 196607 + 3, 4 * 196609 + 1, 4 * 262145 + 2}
    assert {c.mode for c in go.ADAM_CASES} == {'off', 'below', 'above', 'zero'} and {c.step for c in go.ADAM_CASES} == {1, 2, 100000}


def test_planted_zeros_ties_and_decisions():
    th, x, dy = go.highway_operands(33)
    t, h = th[:, :128], th[:, 128:]
    assert (t[:, 0] == 0).all() and (t[:, 1] == 1).all() and (h[:, 2] == 0).all() and not np.signbit(h[:, 2]).any() and np.signbit(h[:, 3]).all()
    assert (h[:, 3] == 0).all() and (t[:, 2:4] != 0).all() and (dy != 0).all() and (h[:, 4] == 0).all() and (t[:, 4] == 0).all()
    for c in (next(c for c in go.ACT_CASES if c.n == 1001 and c.act == 'relu'), next(c for c in go.AFF_CASES if c.M == 33 and c.act == 'relu')):
        ops = go.act_operands(c) if isinstance(c, go.ActCase) else go.aff_operands(c)
        y, g = (ops[0], ops[1]) if isinstance(c, go.ActCase) else (ops[0], ops[2])
        z = y.reshape(-1)
        assert ((z == 0) & ~np.signbit(z)).any() and ((z == 0) & np.signbit(z)).any() and (z < 0).any() and (g != 0).all()
    a, b = go.l1_operands('x', 1, 37, 1025)
    d = a.astype(np.float64) - b
    assert (d == 0).mean() > 0.2 and ((a == 0) & np.signbit(b) & ~np.signbit(a)).any() and ((b == 0) & np.signbit(a) & ~np.signbit(b)).any()
    for c in go.ADAM_CASES:
        p, g, m, v, cap = go.adam_operands(c)
        gn = np.linalg.norm(g.astype(np.float64))
        assert (v >= 0).all() and {'off': cap == 0, 'below': 0 < gn < cap / 4, 'above': gn > 4 * cap, 'zero': gn == 0 and cap > 0}[c.mode]


# ------------------------------------------------------------------------------------------------------------------
# the doors: names, documents, refusals

def test_door_names_are_in_the_header_the_wrappers_and_the_documents(built_lib):
    hdr = open(os.path.join(ROOT, 'include', 'taco_hip.h')).read()
    integ = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    src = open(os.path.join(ROOT, 'tacotron_amd', 'csrc', 'elementwise.hip')).read()
    for d in DOORS:
        name = 'taco_debug_' + d
        assert re.search(r'^int %s\(' % name, hdr, re.M), name
        assert re.search(r'^extern "C" int %s\(' % name, src, re.M), name
        assert name in built_lib.EXPORTS and callable(getattr(built_lib, 'debug_' + d)) and name in integ, name
        assert getattr(built_lib._lib, name).argtypes == built_lib.EXPORTS[name][1]
    assert (built_lib.LOSS_PARTS, built_lib.SUMSQ_PARTS, built_lib.MAX_TRANSPOSE_BATCH) == (go.LOSS_PARTS, go.SUMSQ_PARTS, go.MAX_TRANSPOSE_BATCH)
    k = open(os.path.join(ROOT, 'tacotron_amd', 'csrc', 'kernels.h')).read()
    for name, v in (('kLossParts', go.LOSS_PARTS), ('kSumsqParts', go.SUMSQ_PARTS), ('kMaxTransposeBatch', go.MAX_TRANSPOSE_BATCH)):
        assert re.search(r'constexpr int %s = %d;' % (name, v), k)
    assert 'constexpr int kEmbSeg = %d;' % go.EMB_PASS in src


def test_the_c_doors_refuse_bad_arguments_before_anything_is_enqueued(built_lib):
    """the C ABI's own checks (no GPU is touched: every call here is refused): TACO_EINVAL with a message that names the argument"""
    L, P = built_lib._lib, C.c_void_p
    a = [P(0x100000 * (i + 1)) for i in range(12)]           # never dereferenced
    two = lambda p, q: (C.c_void_p * 2)(p.value, q.value)
    ints = lambda *v: (C.c_int * len(v))(*v)
    calls = (
        (lambda: L.taco_debug_embedding(a[0], None, a[2], 4, 3, 16, None), 'ids is null'),
        (lambda: L.taco_debug_embedding(a[0], a[1], a[2], 4, 3, 18, None), 'width must be a multiple of 4'),
        (lambda: L.taco_debug_embedding(a[0], a[1], a[0], 4, 3, 16, None), 'out may not overlap table'),
        (lambda: L.taco_debug_embedding_bwd(a[0], a[1], a[2], 4, 3, 1028, None), r'width must be a multiple of 4 in \[4, 1024\]'),
        (lambda: L.taco_debug_embedding_bwd(a[0], a[1], a[2], 0, 3, 16, None), r'rows must be in \[1, 2\^22\]'),
        (lambda: L.taco_debug_embedding_bwd(a[0], a[1], None, 4, 3, 16, None), 'dtable is null'),
        (lambda: L.taco_debug_highway_combine(a[0], a[1], a[1], 4, None), 'y may not overlap x'),
        (lambda: L.taco_debug_highway_combine_bwd(a[0], a[1], a[2], a[3], None, 4, None), 'dx is null'),
        (lambda: L.taco_debug_act_bwd(a[0], a[1], None, a[2], 0, 1, None), r'n must be in \[1, 2\^31\)'),
        (lambda: L.taco_debug_act_bwd(a[0], a[1], None, a[2], 8, 4, None), 'act must be one of'),
        (lambda: L.taco_debug_act_bwd(a[0], a[1], None, P(a[1].value + 4), 8, 1, None), 'dz may not overlap dy'),
        (lambda: L.taco_debug_act_bwd(a[0], a[1], None, a[0], 8, 1, None), 'dz may not overlap y'),
        (lambda: L.taco_debug_affine_act_bwd(a[0], a[1], a[2], a[3], a[4], a[4], 4, 8, 1, None), 'dgamma may not overlap dbeta'),
        (lambda: L.taco_debug_affine_act_bwd(a[0], a[1], a[2], a[3], a[4], a[5], 4, 8, 2, None), 'act must be TACO_ACT_NONE or TACO_ACT_RELU'),
        (lambda: L.taco_debug_colsum_batched(a[0], 7, a[1], 2, 3, 8, None), 'ld must be >= 8'),
        (lambda: L.taco_debug_mask_rows(a[0], a[1], a[2], 2, 3, 6, None), 'C must be a multiple of 4'),
        (lambda: L.taco_debug_center_rows(a[0], None, a[2], 2, 3, 8, None), 'len is null'),
        (lambda: L.taco_debug_mask_pos(a[0], 8, a[1], 7, 4, 8, 2.0, None), 'ldy must be >= 8'),
        (lambda: L.taco_debug_mask_pos(a[0], 8, a[0], 8, 4, 8, 2.0, None), 'g may not overlap y'),
        (lambda: L.taco_debug_zero_tail_rows(a[0], 8, a[0], 8, a[2], 2, 3, None), 'x0 may not overlap x1'),
        (lambda: L.taco_debug_add(a[0], a[1], None, 8, None), 'y is null'),
        (lambda: L.taco_debug_l1_loss(a[0], None, None, 0, 2, 4, None, None, None, 0, 0, 0, a[3], a[4], None, None), 'a0 and b0 must both be given'),
        (lambda: L.taco_debug_l1_loss(a[0], a[1], a[2], 3, 2, 4, None, None, None, 0, 0, 0, a[3], a[4], None, None), 'ldg0 must be >= 4'),
        (lambda: L.taco_debug_l1_loss(a[0], a[1], a[2], 4, 2, 4, None, None, None, 0, 0, 0, None, a[4], None, None), 'parts is null'),
        (lambda: L.taco_debug_transpose_batch(97, None, None, None, None, None, None, None, None), r'n must be in \[1, 96\]'),
        (lambda: L.taco_debug_transpose_batch(1, two(a[0], a[0]), two(a[1], a[1]), ints(3), ints(4), ints(5), ints(8), ints(4), None), 'a pitched job has one tap'),
        (lambda: L.taco_debug_transpose_batch(1, two(a[0], a[0]), two(a[0], a[0]), ints(1), ints(4), ints(5), None, None, None), r'out\[0\] may not overlap in\[0\]'),
        (lambda: L.taco_debug_sumsq(None, 8, a[1], None), 'x is null'),
    )
    for call, msg in calls:
        assert call() == -1, msg                             # TACO_EINVAL
        got = built_lib.last_error()
        assert re.search(msg, got) and got.startswith('taco_debug_'), (msg, got)
    assert {n for call, _ in calls for n in call.__code__.co_names if n.startswith('taco_debug_')} == {'taco_debug_' + d for d in DOORS}


def test_the_wrappers_refuse_bad_arguments_by_name(built_lib):
    """every check runs on tensors of any device and the device check comes last: CPU tensors reach it only when all else is right"""
    lib, z = built_lib, torch.zeros
    zi, zb = lambda n: torch.zeros(n, dtype=torch.int32), lambda n: torch.zeros(n, dtype=torch.uint8)
    em = dict(table=z(3 * 16), ids=zi(4), out=z(4 * 16), rows=4, V=3, width=16)
    eb = dict(dout=z(4 * 16), ids=zi(4), dtable=z(3 * 16), rows=4, V=3, width=16)
    hw = dict(th=z(2 * 256), x=z(2 * 128), y=z(2 * 128), M=2)
    hb = dict(th=z(2 * 256), x=z(2 * 128), dy=z(2 * 128), dth=z(2 * 256), dx=z(2 * 128), M=2)
    ab = dict(y=z(8), dy=z(8), dz=z(8), n=8, act='relu', keep=zb(8))
    af = dict(pre=z(32), gamma=z(8), dy=z(32), dz=z(32), dgamma=z(8), dbeta=z(8), M=4, N=8, act='relu')
    cs = dict(x=z(6 * 10), out=z(2 * 8), B=2, T=3, N=8, ld=10)
    mr = dict(x=z(48), length=zi(2), y=z(48), B=2, T=3, C_cols=8)
    cr = dict(x=z(48), length=zi(2), out=z(48), B=2, T=3, C_cols=8)
    mp = dict(g=z(4 * 12), y=z(4 * 10), rows=4, cols=8, scale=2.0, ldg=12, ldy=10)
    zt = dict(x0=z(6 * 8), C0=8, length=zi(2), B=2, Td=3, x1=z(6 * 4), C1=4)
    ad = dict(a=z(8), b=z(8), y=z(8), n=8)
    l1 = dict(terms=[dict(a=z(8), b=z(8), grad=z(2 * 6), M=2, N=4, ldg=6), None], parts=z(1024), loss=z(3))
    tb = dict(jobs=[dict(src=z(3 * 4 * 5), dst=z(3 * 5 * 4), taps=3, K=4, N=5)])
    sq = dict(x=z(8), n=8, out=z(256))
    for fn, args, first in ((lib.debug_embedding, em, 'table'), (lib.debug_embedding_bwd, eb, 'dout'), (lib.debug_highway_combine, hw, 'th'),
                            (lib.debug_highway_combine_bwd, hb, 'th'), (lib.debug_act_bwd, ab, 'y'), (lib.debug_affine_act_bwd, af, 'pre'),
                            (lib.debug_colsum_batched, cs, 'x'), (lib.debug_mask_rows, mr, 'x'), (lib.debug_center_rows, cr, 'x'), (lib.debug_mask_pos, mp, 'y'),
                            (lib.debug_zero_tail_rows, zt, 'length'), (lib.debug_add, ad, 'a'), (lib.debug_l1_loss, l1, 'a0'),
                            (lib.debug_transpose_batch, tb, r'src\[0\]'), (lib.debug_sumsq, sq, 'x')):
        with pytest.raises(ValueError, match=r'^%s: %s must be on the GPU' % (fn.__name__, first)):
            fn(**args)
    same = z(8)
    with pytest.raises(ValueError, match=r'^debug_act_bwd: y must be on the GPU'):        # in place is no overlap
        lib.debug_act_bwd(z(8), same, same, 8, 'tanh')
    for fn, args, change, msg in (
            (lib.debug_embedding, em, dict(ids=z(4)), r'ids must be a contiguous int32 tensor'),
            (lib.debug_embedding, em, dict(width=18), r'width must be a multiple of 4, got 18'),
            (lib.debug_embedding, em, dict(out=z(63)), r'out must hold at least 64 elements, got 63'),
            (lib.debug_embedding_bwd, eb, dict(width=1028), r'width must be an integer in \[4, 1024\]'),
            (lib.debug_embedding_bwd, eb, dict(dtable=eb['dout']), r'dtable may not overlap dout'),
            (lib.debug_highway_combine, hw, dict(M=0), r'M must be an integer in \[1, 4194304\]'),
            (lib.debug_highway_combine_bwd, hb, dict(dx=hb['dy']), r'dx may not overlap dy'),
            (lib.debug_act_bwd, ab, dict(act='gelu'), r'act must be one of'),
            (lib.debug_act_bwd, ab, dict(dz=ab['y']), r'dz may not overlap y'),
            (lib.debug_act_bwd, ab, dict(dy=z(16), dz=None), r'dz must be'),
            (lib.debug_act_bwd, ab, dict(keep=z(8)), r'keep must be a contiguous uint8 tensor'),
            (lib.debug_affine_act_bwd, af, dict(act='tanh'), r"act must be 'none' or 'relu'"),
            (lib.debug_affine_act_bwd, af, dict(dbeta=af['dgamma']), r'dgamma may not overlap dbeta'),
            (lib.debug_colsum_batched, cs, dict(ld=7), r'ld must be >= 8, got 7'),
            (lib.debug_colsum_batched, cs, dict(x=z(57)), r'x must hold at least 58 elements, got 57'),
            (lib.debug_mask_rows, mr, dict(C_cols=6), r'C must be a multiple of 4'),
            (lib.debug_center_rows, cr, dict(length=zi(1)), r'length must hold at least 2 elements, got 1'),
            (lib.debug_mask_pos, mp, dict(ldy=7), r'ldy must be >= 8, got 7'),
            (lib.debug_mask_pos, mp, dict(y=mp['g']), r'g may not overlap y'),
            (lib.debug_zero_tail_rows, zt, dict(x1=zt['x0']), r'x0 may not overlap x1'),
            (lib.debug_add, ad, dict(y=ad['a']), r'y may not overlap a'),
            (lib.debug_l1_loss, l1, dict(terms=[None, None]), r'terms must be a list of two dicts'),
            (lib.debug_l1_loss, l1, dict(terms=[dict(l1['terms'][0], ldg=3), None]), r'terms\[0\]: ldg must be >= 4, got 3'),
            (lib.debug_l1_loss, l1, dict(parts=z(1023)), r'parts must hold at least 1024 elements'),
            (lib.debug_transpose_batch, tb, dict(jobs=[]), r'jobs must be a list of 1 to 96 dicts'),
            (lib.debug_transpose_batch, tb, dict(jobs=[dict(tb['jobs'][0], ldi=8)]), r'jobs\[0\]: a job with a pitch has taps == 1'),
            (lib.debug_sumsq, sq, dict(out=z(255)), r'out must hold at least 256 elements')):
        with pytest.raises(ValueError, match='^%s: %s' % (fn.__name__, msg)):
            fn(**dict(args, **change))
