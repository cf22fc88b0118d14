"""Host (no GPU): the references, the restated dispatch predicates and the case lists of tests/gemm_paths.py.
The case lists must reach every label of PATH_TABLE; the references are held against a literal triple loop and against
torch.nn.functional.conv1d in fp64; the predicates against the known routes of tests/test_gpu_ops.py's CASES."""
import numpy as np
import torch

from tests import gemm_forms as gf
from tests import gemm_paths as gp


def _labels():
    out = {}
    for c in gp.all_nn_rows():
        out.setdefault(gp.nn_row_path(c), []).append(c.id)
    for c in gp.NLD_CASES:
        out.setdefault(gp.nld_path(c), []).append(c.id)
    for c in gp.KSPLIT_CASES:
        S = gp.ksplit_plan(c.M, c.N, c.K, c.taps, c.slabs * c.M * c.N, c.force)[0]
        out.setdefault('ksplit.S%d' % S, []).append(c.id)
    for c in gp.TN_PATH_CASES:
        out.setdefault(gp.tn_case_plan(c)['label'], []).append(c.id)
    for label, ids in gf.form_labels().items():         # the forms of tests/gemm_forms.py
        out.setdefault(label, []).extend(ids)
    return out


def test_case_lists_reach_every_path_label():
    got = _labels()
    assert set(got) == set(gp.PATH_TABLE), 'missing: %s, not in the table: %s' % (sorted(set(gp.PATH_TABLE) - set(got)),
                                                                                  sorted(set(got) - set(gp.PATH_TABLE)))
    assert len(gp.PATH_TABLE) == 8 + 6 + 3 + 10 + len(gf.FORM_LABELS) and set(gf.FORM_LABELS) <= set(got)


def test_every_case_states_the_path_the_restatement_gives():
    ids = []
    for c in gp.all_nn_rows():
        assert gp.nn_row_path(c) == c.path, c.id
        assert c.M % c.T == 0 and c.lda >= c.K and c.ldw >= c.N and c.ldc >= c.N and c.ldr >= c.N, c.id
        ids.append(c.id)
    for c in gp.NLD_CASES:
        assert gp.nld_path(c) == c.path, c.id
        assert c.nld % 4 == 0 and c.N <= c.nld <= c.ldw and c.ldc >= c.N and c.nld - (c.N + 3) // 4 * 4 in (0, 4), c.id
        ids.append(c.id)
    for c in gp.KSPLIT_CASES:
        S, per, chunks = gp.ksplit_plan(c.M, c.N, c.K, c.taps, c.slabs * c.M * c.N, c.force)
        assert S == c.S and 'ksplit.S%d' % S == c.path and len(chunks) == S, c.id
        assert chunks[0][0] == 0 and chunks[-1][1] == c.taps * gp.cdiv(c.K, 32) and all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))
        ids.append(c.id)
    for c in gp.TN_PATH_CASES:
        p = gp.tn_case_plan(c)
        assert (p['label'], p['merged'], p['splits']) == (c.path, c.merged, c.splits), (c.id, p)
        assert c.M % c.T == 0 and c.lda >= c.K and c.ldy >= c.N and c.ldw >= c.N, c.id
        ids.append(c.id)
    assert len(ids) == len(set(ids)), 'duplicate case ids'


def test_load_path_cases_break_each_bit_in_each_way_separately():
    """(a): lda % 4, A base offset and K % 4 = 1, 2, 3 each as the ONLY breach of bit 0 with bit 1 intact; the same for the W
    operand; every flags class has a k-tile tail and an M tail, and the five (taps, pad_l) pairs all occur."""
    def causes(c):
        return (('lda', c.lda % 4) if c.lda % 4 else None, ('offA', c.offA % 4) if c.offA % 4 else None, ('K', c.K % 4) if c.K % 4 else None,
                ('ldw', c.ldw % 4) if c.ldw % 4 else None, ('offW', c.offW % 4) if c.offW % 4 else None, ('N', c.N % 4) if c.N % 4 else None)
    single = set()
    for c in gp.NN_LOAD_CASES:
        cs = [x for x in causes(c) if x]
        if len(cs) == 1:
            single.add(cs[0])
        assert c.M in (70, 130) and c.N in (61, 62, 63, 64, 80) and c.K in (17, 18, 19, 20, 36), c.id
    assert single == {(w, r) for w in ('lda', 'offA', 'K', 'ldw', 'offW', 'N') for r in (1, 2, 3)}
    for f in range(4):
        rows = [c for c in gp.NN_LOAD_CASES if c.path == 'nn.t64.f%d' % f]
        assert any(c.K % 16 for c in rows) and any(c.M % 64 for c in rows)
    assert {(c.taps, c.pad_l) for c in gp.NN_LOAD_CASES} == {(1, 0), (3, 1), (4, 0), (2, 3), (3, -1)}


def test_epilogue_cases_give_every_gemm2_form_every_option_it_accepts():
    by = {}
    for e in gp.EPI_CASES:
        by.setdefault(e.form, []).append(e)
    for form, accepts in (('vec', 'bkshrp'), ('scalar', 'bkshrp'), ('shifted', 'bsh')):
        rows = by[form]
        assert set(''.join(e.opts for e in rows)) == set(accepts), form
        assert {e.act for e in rows} == {0, 1, 2, 3}, form
        assert any('b' not in e.opts for e in rows), form
        assert any('s' in e.opts and 'h' not in e.opts for e in rows) and any('h' in e.opts and 's' not in e.opts for e in rows) and \
            any('s' in e.opts and 'h' in e.opts for e in rows), form
        assert any(e.offB == 1 for e in rows), form
        assert {e.N for e in rows} == {128, 132, 260}, form
    assert {e.ldc - e.N for e in gp.EPI_CASES} >= {0, 1, 2, 4}
    # each cause of the scalar form by itself: C off alignment, ldr % 4, residual / keep / Cpre pointer off alignment, a pitch the shifted form cannot take
    sc = by['scalar']
    assert any(e.offC == 1 and e.ldc % 4 == 0 for e in sc) and any(e.ldr % 4 and 'r' in e.opts and e.offC == 0 and e.ldc % 4 == 0 for e in sc)
    assert any(e.offR == 1 and 'r' in e.opts and e.ldr % 4 == 0 and e.offC == 0 for e in sc)
    assert any(e.offK == 1 and 'k' in e.opts and e.offC == 0 and e.ldc % 4 == 0 for e in sc)
    assert any(e.offP == 1 and 'p' in e.opts and e.offC == 0 and e.ldc % 4 == 0 for e in sc)
    assert any(e.ldc % 4 and 'p' in e.opts for e in sc) and any(e.ldc % 4 and 'k' in e.opts for e in sc) and any(e.ldc % 4 and 'r' in e.opts for e in sc)


def test_ksplit_cases_cut_where_the_issue_asks():
    """a chunk edge in the middle of a tap, a last chunk shorter than `per`, a K tail inside a chunk, and a forced S that is ignored"""
    mid_tap = short_last = ignored = False
    for c in gp.KSPLIT_CASES:
        S, per, chunks = gp.ksplit_plan(c.M, c.N, c.K, c.taps, c.slabs * c.M * c.N, c.force)
        ktiles = gp.cdiv(c.K, 32)
        assert c.K % 32 != 0 and c.K % 4 == 0 and c.N % 4 == 0
        mid_tap |= any(lo % ktiles for lo, _ in chunks)
        short_last |= chunks[-1][1] - chunks[-1][0] < per
        ignored |= S != c.force
        if S == c.force:
            assert S <= c.taps * ktiles // 6 and S <= c.slabs
    assert mid_tap and short_last and ignored
    assert {c.S for c in gp.KSPLIT_CASES} == {2, 3, 5}


def test_tn_cases_cover_merge_pitch_accumulate_and_split_variants():
    rows = gp.TN_PATH_CASES
    plans = {c.id: gp.tn_case_plan(c) for c in rows}
    multi = [c for c in rows if c.taps > 1 and c.K % 64 != 0]
    assert any(plans[c.id]['merged'] for c in multi)
    assert any(not plans[c.id]['merged'] and c.merge == '0' and plans[c.id]['flags'] & 1 for c in multi)        # switched off
    assert any(not plans[c.id]['merged'] and c.merge != '0' and not plans[c.id]['flags'] & 1 for c in multi)    # bit 0 clear
    assert any(c.ldw == c.N + 3 for c in rows) and any(c.ldw == c.N for c in rows) and any(c.offW == 1 for c in rows)
    assert any(c.acc for c in rows) and any(not c.acc for c in rows)
    assert any(c.det == '1' and plans[c.id]['splits'] == 1 for c in rows)
    assert any(plans[c.id]['splits'] > 1 and c.M % plans[c.id]['chunk'] for c in rows)                          # short last chunk
    assert any(c.pad_l > c.taps - 1 for c in rows) and any(c.pad_l < 0 for c in rows)
    assert {(c.taps, c.pad_l) for c in rows if plans[c.id]['bm'] == 64} == {(1, 0), (3, 1), (2, 3), (3, -1), (8, 3)}
    # each cause by itself, 64 tile
    def causes(c):
        return [x for x in (('lda', c.lda % 4), ('offA', c.offA % 4), ('K', c.K % 4), ('ldy', c.ldy % 4), ('offY', c.offY % 4), ('N', c.N % 4)) if x[1]]
    single = {causes(c)[0][0] for c in rows if len(causes(c)) == 1 and plans[c.id]['bm'] == 64}
    assert single == {'lda', 'offA', 'K', 'ldy', 'offY', 'N'}


def _loop_nn(A, W, bias, T, pad_l):
    M, K = A.shape
    taps, _, N = W.shape
    y, S = np.zeros((M, N)), np.zeros((M, N))
    for m in range(M):
        t = m % T
        for n in range(N):
            for j in range(taps):
                st = t + j - pad_l
                if 0 <= st < T:
                    for k in range(K):
                        y[m, n] += A[m + j - pad_l, k] * W[j, k, n]
                        S[m, n] += abs(A[m + j - pad_l, k] * W[j, k, n])
            if bias is not None:
                y[m, n] += bias[n]
                S[m, n] += abs(bias[n])
    return y, S


def _loop_tn(A, dY, taps, T, pad_l):
    M, K = A.shape
    N = dY.shape[1]
    dW, S = np.zeros((taps, K, N)), np.zeros((taps, K, N))
    for j in range(taps):
        for m in range(M):
            st = m % T + j - pad_l
            if 0 <= st < T:
                for k in range(K):
                    for n in range(N):
                        dW[j, k, n] += A[m + j - pad_l, k] * dY[m, n]
                        S[j, k, n] += abs(A[m + j - pad_l, k] * dY[m, n])
    return dW, S


TINY = [(6, 3, 4, 5, 3, 1), (8, 4, 3, 2, 2, 3), (5, 5, 2, 3, 3, -1)]       # M, T, N, K, taps, pad_l


def test_references_agree_with_a_literal_triple_loop():
    for i, (M, T, N, K, taps, pad_l) in enumerate(TINY):
        rng = np.random.default_rng(i)
        A, W, b = rng.standard_normal((M, K)), rng.standard_normal((taps, K, N)), rng.standard_normal(N)
        dY = rng.standard_normal((M, N))
        keep = rng.integers(0, 2, (M, N)).astype(np.uint8)
        sc, sf, res = rng.standard_normal(N), rng.standard_normal(N), rng.standard_normal((M, N))
        y, S = _loop_nn(A, W, b, T, pad_l)
        C, pre, S1 = gp.nn_ref(A, W, b, T, pad_l, 0)
        assert np.allclose(C, y, rtol=1e-13, atol=1e-13) and np.allclose(S1, S, rtol=1e-13, atol=1e-13) and np.array_equal(C, pre)
        C, pre, _ = gp.nn_ref(A, W, b, T, pad_l, 1, keep, sc, sf, res)
        p = np.maximum(y, 0) * keep * 2
        assert np.allclose(pre, p, rtol=1e-13, atol=1e-13) and np.allclose(C, p * sc + sf + res, rtol=1e-13, atol=1e-13)
        assert np.allclose(gp.nn_ref(A, W, None, T, pad_l, 3, shift=sf)[0], np.tanh(y - b) + sf, rtol=1e-12, atol=1e-13)
        assert np.allclose(gp.nn_ref(A, W, None, T, pad_l, 2, scale=sc)[0], sc / (1 + np.exp(-(y - b))), rtol=1e-12, atol=1e-13)
        cr = gp.conv_ref(A, W, b, T, pad_l, 1, keep, sc, sf, res)
        assert len(cr) == 2 and np.array_equal(cr[0], C) and np.array_equal(cr[1], pre)
        dW, St = gp.tn_ref(A, dY, taps, T, pad_l)
        dWl, Sl = _loop_tn(A, dY, taps, T, pad_l)
        assert np.allclose(dW, dWl, rtol=1e-13, atol=1e-13) and np.allclose(St, Sl, rtol=1e-13, atol=1e-13)


def test_nn_ref_is_conv1d_for_odd_and_even_tap_counts():
    rng = np.random.default_rng(4)
    B, T, K, N = 3, 11, 5, 7
    for taps, pad_l in ((3, 1), (4, 1), (4, 2)):
        A, W, b = rng.standard_normal((B * T, K)), rng.standard_normal((taps, K, N)), rng.standard_normal(N)
        x = torch.from_numpy(A).view(B, T, K).transpose(1, 2)                        # (B, K, T)
        x = torch.nn.functional.pad(x, (pad_l, taps - 1 - pad_l))
        y = torch.nn.functional.conv1d(x, torch.from_numpy(W).permute(2, 1, 0).contiguous(), torch.from_numpy(b))   # (B, N, T)
        ref = y.transpose(1, 2).reshape(B * T, N).numpy()
        assert np.allclose(gp.nn_ref(A, W, b, T, pad_l, 0)[0], ref, rtol=1e-12, atol=1e-12)


def test_restated_predicates_on_the_routes_of_test_gpu_ops_cases():
    import tests.test_gpu_ops as ops          # (module import: its tests are not collected a second time under this file)
    route = {}
    for M, T, N, K, taps, pad_l, act, extras in ops.CASES:
        route[(M, T, N, K, taps, pad_l)] = gp.nn_path(M, N, K, taps, K, N, N, 256, 512, 768)
    assert route[(6400, 200, 256, 256, 1, 0)] == 'nn.t64.f3'          # 100 tiles: below gemm2's 160 and below the 384 of the big tile
    assert route[(3000, 3000, 384, 136, 1, 0)] == 'nn.t64.f3'         # 72 tiles
    assert route[(64, 64, 1025, 256, 1, 0)] == 'nn.t64.f1'
    assert set(route.values()) == {'nn.t64.f3', 'nn.t64.f1'}
    assert gp.nn_flags(256, 1025, 512, 256, 256, 1025) == 2           # test_conv_gemm_strided_unaligned
    # forced through gemm2.hip (test_conv_gemm_v2): dense aligned rows take the float4 epilogue
    assert gp.nn_path(1000, 300, 132, 3, 132, 300, 300, 256, 512, 768, cpre_ptr=1024, res_ptr=2048, ldr=300, keep_ptr=4096, min_tiles=1) == 'g2.bx.vec'
    assert gp.nn_path(520, 260, 2048, 1, 2048, 260, 260, 256, 512, 768, min_tiles=1) == 'g2.bx.vec'
    assert gp.nn_path(1000, 128, 2048, 3, 2048, 128, 128, 256, 512, 768, min_tiles=1) == 'g2.f32.vec'      # chain 6144 > 2048
    # test_conv_gemm_v2_shifted_rows
    assert gp.nn_path(333, 1025, 96, 1, 96, 1028, 1027, 256, 512, 768, nld=1028, min_tiles=1, bf16x=False) == 'g2.f32.shifted'
    assert gp.nn_path(333, 1024, 96, 1, 96, 1024, 1025, 256, 512, 768, nld=1024, min_tiles=1) == 'g2.bx.shifted'
    # TN_CASES: the largest op-level case stays on the 64 tile, flags 3 throughout
    plans = [gp.tn_plan(256, K, 512, N, M, N, K, taps, pad_l) for M, T, N, K, taps, pad_l in ops.TN_CASES]
    assert {p['bm'] for p in plans} == {64} and {p['flags'] for p in plans if p['flags'] != 3} == {1}      # (N = 1025: flags 1)
    big = gp.tn_plan(256, 512, 512, 256, 5760, 256, 512, 1, 1)
    assert (big['bm'], big['splits'], big['chunk']) == (64, 18, 320)
    assert gp.tn_plan(256, 80, 512, 128, 720, 128, 80, 8, 3)['merged'] and not gp.tn_plan(256, 128, 512, 128, 90, 128, 128, 16, 7)['merged']
    # the model's k-split choice for test_conv_gemm_ksplit's encoder-proj1-like shape with four slabs
    assert gp.ksplit_plan(1000, 128, 2048, 3, 4 * 1000 * 128)[0] == 4
