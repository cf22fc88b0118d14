"""GPU: the backward pass stage by stage, row by row.  Every activation-gradient buffer that persists in the workspace after
taco_backward is compared with the gradient of the matching intermediate in the fp64 oracle (oracle.taco_torch.Recorder):
as a whole tensor (rel-L2 <= TENSOR_BAR) and per row -- one (b, t) frame or text position, one
(b, t) step record of bwd.gstash field by field -- against ROW_BAR (tests/stage_bars.py).  A parameter gradient is a sum
over all rows, so a mistake confined to one utterance or one decoder step is diluted below its bar; the row bar is not.
Where the math makes a value zero it must be exactly zero.

The buffer map (taken from the code that writes each buffer, model.hip taco_backward, decoder.hip / decoder3.hip):
  bwd.gstash (B, Td, kGsRec) per step t:
    kGsG + 512 l       d gates pre-activation of GRU l           [r | u]
    kGsC + 256 l       d candidate pre-activation of GRU l
    kGsX               d x (in-proj output; x also feeds out_proj)
    kGsQ               d q                                       exactly 0 at the last step (its context is never used)
    kGsP1S             d pre-net-1 pre-activation of step t+1 if step t+1 was fed cell_output[t], else exactly 0 (and at
                       the last step)
    kGsP2, kGsP1       d pre-net pre-activations of step t       exactly 0 where dropout dropped the unit
    kGsO               d cell_output_t minus its q and pre-net-feed parts (the kernel carries those as factors; the GEMM
                       that fills the slot adds d x_{t+1} Wx_o^T to the direct term): compared with
                       d o - d q Wq^T - [fed] d p1pre_{t+1} W1^T (last-frame columns), formed in fp64 from the oracle
    (kGsCtx is written by neither kernel: the context gradient travels as E below)
  bwd.dkeys_e (B Tt, 512): [:, :256] d keys, exactly 0 at text positions >= text_length; [:, 256:] the factor
    E[b] = sum_t al[b, t-1]^T d x[b, t], compared as E Wx_c^T (Wx_c = Wa[80r:] Wi[128:]) with the oracle's context part of
    d values, sum_t al_t^T d ctx_t; E rows past text_length exactly 0
  bwd.dattv_rows (B, 256): each batch row's part of d attention_v
  bwd.ds2s (B Td, 80r): sign(seq2seq_output - mel), the L1 term
  bwd.post.dx (B Td r, 80): d seq2seq_output in total -- on this path the post-net's input-gradient accumulator starts from
    bwd.ds2s (bwd.ds2s_tot is written only when it does not)
  bwd.{post,enc}.dpj1 / dz1 / dpool / dx: d of proj1 after its ReLU and BN (the proj2 input), of proj1 before its ReLU, of
    the max-pool output (written only where the GEMM does not take the pooled epilogue, which never forms it) and of the
    CBHG input (encoder: the pre-net output)
  bwd.pre.dz2 / dz1 / demb: d encoder pre-net pre-activations (exactly 0 where dropout dropped the unit), d embedding output

Discrete decisions (tests/decisions.py): the HIP path's ReLU / max-pool decisions are read back from the workspace, the flips
against fp64 are bounded (count, each fp64 margin <= 1e-5) and the oracle runs with the HIP decisions forced; the L1 loss's
sign ties go through l1_tie_adjusted.  S2 and B = 64 at S1 size also get the whole-model parity of test_full_size_vs_oracle.

Measured on MI355X (each test prints its full table):
  shape                      worst tensor rel-L2     worst row                         decision flips  L1 ties
  golden r=2, r=5, spk       1.4e-6, 2.0e-6, 1.5e-6  5.1e-6, 1.0e-5, 3.6e-6 (gstash.q) 0               0
  ragged medium              2.0e-6 (gstash.q)       1.6e-5 (d keys, b 1, s 7)         0               0
  decoder3 B=11, 40, 70      1.9e-6, 2.0e-6, 1.9e-6  2.4e-5, 3.1e-5, 7.7e-5 (d keys)   0, 1, 0         0
  agent B=12, decoder.hip    1.7e-6, 2.1e-6, 2.0e-6  3.0e-5, 1.3e-5, 1.8e-5 (d keys)   0               0
    B=5, r=3 B=4
  S1                         9.0e-6 (gstash.q)       4.6e-4 (d keys, b 2, s 138)       5               0
  S2                         9.1e-6 (gstash.q)       5.6e-4 (d keys, b 15, s 68)       12              2
  B=64 at S1 size            9.3e-6 (gstash.q)       4.3e-4 (d keys, b 36, s 158)      13              1
  The worst tensor is d q everywhere; the worst row is a d keys row (one text position, summed over every decoder step) at
  every shape but the fixtures, and every other buffer's worst row is <= 7e-5.  Every exact-zero site was exactly zero.
"""
import os

import numpy as np
import pytest
import torch

from oracle import taco_numpy as on
from oracle import taco_torch as ot
from tests.decisions import as_force, flips, hip_decisions
from tests.stage_bars import compare, exact_zero_failures, failures
from tests.test_gpu_model import (Runner, _argmax_check, _full_case, check_grads, f64, golden, l1_tie_adjusted, report)
from tests.util import small_case

pytestmark = pytest.mark.gpu

K_GS = {'G': 0, 'C': 1536, 'X': 2304, 'Q': 2560, 'P1S': 2816, 'P2': 3328, 'P1': 3456, 'O': 3712, 'REC': 4112}   # csrc/kernels.h


def _pool_fused(M, KC):
    """Does the d pool GEMM take gemm2.hip's pooled epilogue (which never writes d pool)?  gemm2.hip: pooled m-tiles advance
    by 127 rows, 128-column tiles, taken from TACO_GEMM2_MIN_TILES (default 160) tiles on."""
    min_tiles = int(os.environ.get('TACO_GEMM2_MIN_TILES', '160'))
    return min_tiles > 0 and -(-max(M - 1, 1) // 127) * -(-KC // 128) >= min_tiles and not os.environ.get('TACO_NO_POOL_FUSE')


def _oracle_torch_inputs(p, inp, masks):
    pt = ot.to_torch(p, torch.float64)
    ti = {'text': torch.tensor(inp['text'], dtype=torch.int64),
          'text_length': torch.tensor(inp['text_length'], dtype=torch.int64),
          'mel': torch.tensor(inp['mel'], dtype=torch.float64), 'stft': torch.tensor(inp['stft'], dtype=torch.float64)}
    if 'speaker' in inp:
        ti['speaker'] = torch.tensor(inp['speaker'], dtype=torch.int64)
    tm = {k: torch.tensor(np.asarray(v), dtype=torch.float64) for k, v in masks.items()}
    return pt, ti, tm


def run_stages(lib, tag, p, inp, masks, B, Tt, Td, r, V, S=1, max_flips=16, parity=False, last_cluster=None):
    """Forward + backward on the HIP path, the fp64 oracle with a Recorder and the HIP decisions forced, then every mapped
    buffer against its reference.  p = None: the library's own initialisation (seed 0).  Returns the list of compare()
    results; asserts at the end, after printing everything."""
    R = Runner(lib, B, Tt, Td, r, V, S=S)
    if p is None:
        R.pb.init_(seed=0)
        p = R.pb.to_dict()
    R.set(p, inp, masks)
    R.forward()
    R.backward()
    if last_cluster is not None:
        assert lib.last_cluster(1) == last_cluster
    adj, n_ties = l1_tie_adjusted(R, p, inp, masks, r, Td)
    # the HIP path's discrete decisions against fp64's: flips bounded, then imposed on the oracle
    hip, ok, how = hip_decisions(R, p, masks, B, Tt, Td, r, S)
    dec = ot.Decisions()
    with torch.no_grad():
        pt, ti, tm = _oracle_torch_inputs(p, adj, masks)
        ot.forward(pt, ti, r, Td, True, tm, dec)
        del pt, ti, tm
    fl = flips(hip, ok, dec)
    del dec
    print('  %s: %d L1 ties, %d decision flips vs fp64 (BN affine as %s)%s' % (tag, n_ties, len(fl), how['enc'],
                                                                               ''.join('\n    %-34s %-16s fp64 margin %.2e' % f for f in fl[:20])))
    assert len(fl) <= max_flips and all(mg <= 1e-5 for _, _, mg in fl), fl
    rec = ot.Recorder()
    lt, s2, o2, a2, ref = ot.loss_and_grads(p, f64(adj), r, Td, f64(masks), dec=ot.Decisions(as_force(hip)), rec=rec)
    G = rec.grad
    del rec
    bad = []
    if parity:   # the whole-model parity of test_full_size_vs_oracle (SURVEY 8c bars; gradients at the small cases' 2e-4)
        r1, m1 = report('%s seq2seq_output' % tag, R.s2s.cpu().numpy(), s2)
        r2, m2 = report('%s output' % tag, R.out.cpu().numpy(), o2)
        r3, m3 = report('%s alignments' % tag, R.al.cpu().numpy(), a2)
        assert r1 < 1e-4 and m1 < 1e-3 and r2 < 1e-4 and m2 < 1e-3 and m3 < 1e-5
        loss = R.loss.cpu().numpy()
        print('  loss hip %.3f oracle %.3f' % (loss[0], lt))
        assert abs(loss[0] - lt) <= 1e-5 * lt
        _argmax_check(R.al.cpu().numpy(), a2, inp['text_length'])
        gbad = check_grads(R, ref, tol=2e-4)
        assert not gbad, gbad

    res = []

    def cmp(name, hip_arr, ref_arr, lead):
        st = compare(name, hip_arr, ref_arr, lead)
        res.append(st)
        bad.extend(failures(st))
        return st

    L = np.asarray(inp['text_length'])
    smp = np.asarray(masks['sample']) > 0                    # (Td, B): step t + 1 fed cell_output[t]
    k1, k2 = np.asarray(masks['dec_keep1']) > 0, np.asarray(masks['dec_keep2']) > 0
    R80 = 80 * r

    # ---- decoder: bwd.gstash, field by field, per (b, t) ----
    gs = R.wsget('bwd.gstash').reshape(B, Td, K_GS['REC'])

    def steps(name, width):
        out = np.zeros((B, Td, width))
        for t in range(Td):
            g = G.get(name % t)
            if g is not None:
                out[:, t] = g
        return out

    d_q, d_p1 = steps('decoder/q@%d', 256), steps('decoder/pre_net/l1pre@%d', 256)
    d_p1s = np.zeros_like(d_p1)
    d_p1s[:, :-1] = d_p1[:, 1:] * smp[:-1].T[:, :, None]
    d_o = steps('decoder/o@%d', R80) - d_q @ p['decoder/query_layer/kernel'].T.astype(np.float64)
    d_o[:, :, R80 - 80:] -= d_p1s @ p['decoder/pre_net/dense/kernel'].T.astype(np.float64)
    fields = [('gates%d' % l, K_GS['G'] + 512 * l, steps('decoder/gru_%d/gates@%%d' % l, 512)) for l in range(3)]
    fields += [('cand%d' % l, K_GS['C'] + 256 * l, steps('decoder/gru_%d/candidate@%%d' % l, 256)) for l in range(3)]
    fields += [('x', K_GS['X'], steps('decoder/x@%d', 256)), ('q', K_GS['Q'], d_q), ('p1s', K_GS['P1S'], d_p1s),
               ('p2', K_GS['P2'], steps('decoder/pre_net/l2pre@%d', 128)), ('p1', K_GS['P1'], d_p1), ('o', K_GS['O'], d_o)]
    for name, off, refv in fields:
        got = gs[:, :, off:off + refv.shape[2]]
        st = cmp('gstash.' + name, got, refv, (B, Td))
        worst_t = st['rows'].max(0)
        worst_b = st['rows'].max(1)
        st['note'] = 'worst step %d (%.2e), worst batch row %d (%.2e)' % (int(worst_t.argmax()), worst_t.max(), int(worst_b.argmax()),
                                                                         worst_b.max())
    bad += exact_zero_failures('gstash.p1s (successor teacher-forced, or last step)', gs[:, :, K_GS['P1S']:K_GS['P1S'] + 256],
                               np.concatenate([~smp[:-1].T, np.ones((B, 1), bool)], 1)[:, :, None])
    bad += exact_zero_failures('gstash.p1s (successor unit dropped)', gs[:, :-1, K_GS['P1S']:K_GS['P1S'] + 256], ~k1[:, 1:])
    bad += exact_zero_failures('gstash.p1 (unit dropped)', gs[:, :, K_GS['P1']:K_GS['P1'] + 256], ~k1)
    bad += exact_zero_failures('gstash.p2 (unit dropped)', gs[:, :, K_GS['P2']:K_GS['P2'] + 128], ~k2)
    bad += exact_zero_failures('gstash.q (last step)', gs[:, -1:, K_GS['Q']:K_GS['Q'] + 256], True)

    # ---- attention memory ----
    dke = R.wsget('bwd.dkeys_e').reshape(B, Tt, 512).astype(np.float64)
    past = (np.arange(Tt)[None, :] >= L[:, None])[:, :, None]
    cmp('dkeys', dke[:, :, :256], G['decoder/keys'], (B, Tt))
    bad += exact_zero_failures('dkeys (past text_length)', dke[:, :, :256], past)
    wxc = p['decoder/attention_layer/kernel'][R80:].astype(np.float64) @ p['decoder/in_proj/kernel'][128:].astype(np.float64)
    cmp('E Wx_c^T', dke[:, :, 256:] @ wxc.T, G['decoder/values@ctx'], (B, Tt))
    bad += exact_zero_failures('E (past text_length)', dke[:, :, 256:], past)
    cmp('dattv_rows', R.wsget('bwd.dattv_rows'), G['decoder/attention_v@row'], (B,))

    # ---- the L1 term and d seq2seq_output ----
    cmp('ds2s', R.wsget('bwd.ds2s').reshape(B, Td, R80), np.sign(s2 - np.asarray(adj['mel'], np.float64)), (B, Td))
    F_ = Td * r
    cmp('post.dx (d s2s total)', R.wsget('bwd.post.dx').reshape(B, F_, 80), G['seq2seq_output'].reshape(B, F_, 80), (B, F_))

    # ---- the two CBHGs and the encoder pre-net ----
    for pre, prefix, T, KC in (('post', 'post/cbhg/', F_, 1024), ('enc', 'encoder/cbhg/', Tt, 2048)):
        cmp(pre + '.dpj1', R.wsget('bwd.%s.dpj1' % pre).reshape(B, T, -1), G[prefix + 'proj1'], (B, T))
        cmp(pre + '.dz1', R.wsget('bwd.%s.dz1' % pre).reshape(B, T, -1), G[prefix + 'proj1pre'], (B, T))
        dpool = R.wsget('bwd.%s.dpool' % pre).reshape(B, T, -1)
        if _pool_fused(B * T, KC):
            assert not dpool.any(), '%s: the pooled epilogue was expected to leave d pool unwritten' % pre
            print('  %s.dpool: not formed (the d pool GEMM took the pooled epilogue)' % pre)
        else:
            cmp(pre + '.dpool', dpool, G[prefix + 'pool'], (B, T))
    cmp('enc.dx', R.wsget('bwd.enc.dx').reshape(B, Tt, -1), G['encoder/cbhg/in'], (B, Tt))
    ek1, ek2 = np.asarray(masks['enc_keep1']) > 0, np.asarray(masks['enc_keep2']) > 0
    dz2 = R.wsget('bwd.pre.dz2').reshape(B, Tt, -1)
    dz1 = R.wsget('bwd.pre.dz1').reshape(B, Tt, -1)
    cmp('pre.dz2', dz2, G['encoder/pre_net/l2pre'], (B, Tt))
    cmp('pre.dz1', dz1, G['encoder/pre_net/l1pre'], (B, Tt))
    bad += exact_zero_failures('pre.dz2 (unit dropped)', dz2, ~ek2)
    bad += exact_zero_failures('pre.dz1 (unit dropped)', dz1, ~ek1)
    cmp('pre.demb', R.wsget('bwd.pre.demb').reshape(B, Tt, -1), G['encoder/emb'], (B, Tt))

    print('  %-24s %10s %10s  %-12s %s' % (tag, 'rel-L2', 'worst row', 'at', ''))
    for st in res:
        print('  %-24s %10.3e %10.3e  %-12s %s' % (st['name'], st['rel'], st['row'], st['at'], st.get('note', '')))
    w = max(res, key=lambda s: s['rel'])
    wr = max(res, key=lambda s: s['row'])
    print('  STAGES %s: worst tensor %.3e (%s), worst row %.3e (%s at %s), flips %d, ties %d' %
          (tag, w['rel'], w['name'], wr['row'], wr['name'], wr['at'], len(fl), n_ties))
    assert not bad, bad
    return res


@pytest.mark.parametrize('r', [2, 5])
def test_stages_golden(built_lib, r):
    g, p, inp, masks = golden(r)
    run_stages(built_lib, 'golden r=%d' % r, p, inp, masks, int(g['B']), int(g['Tt']), int(g['Td']), r, int(g['V']))


def test_stages_golden_multi_speaker_fused(built_lib):
    g, p, inp, masks = golden(2, spk=True)
    run_stages(built_lib, 'golden spk', p, inp, masks, int(g['B']), int(g['Tt']), int(g['Td']), 2, int(g['V']),
               S=int(g['num_speakers']))


def test_stages_ragged_medium(built_lib):
    """B=4, Tt=37, Td=12 with one text_length of 1."""
    r, V, B, Tt, Td = 2, 40, 4, 37, 12
    p = on.init_params(V, r, seed=4, perturb=0.2)
    inp, masks = small_case(r=r, V=V, B=B, Tt=Tt, Td=Td, seed=8)
    inp['text_length'][2] = 1
    inp['text'][2, 1:] = 0
    run_stages(built_lib, 'ragged medium', p, inp, masks, B, Tt, Td, r, V)


@pytest.mark.parametrize('B,mode,r', [(11, 'default', 2), (40, 'default', 5), (70, 'default', 5), (12, 'agent', 2),
                                      (5, 'v3_off', 2), (4, 'r3', 3)])
def test_stages_decoder_geometries(built_lib, B, mode, r, monkeypatch):
    """Both BPTT kernels per step: decoder3 with a partly filled last cluster (B=11), second and third 32-row launches
    (B=40, 70 at r=5), the agent-scope exchange (B=12), decoder.hip as the fall-back (TACO_DEC_V3=0) and at r=3 (outside
    decoder3's instantiations)."""
    if mode == 'agent':
        monkeypatch.setenv('TACO_DEC_V3_AGENT', '1')
    if mode == 'v3_off':
        monkeypatch.setenv('TACO_DEC_V3', '0')
    V, Tt, Td = 33, 41, 9
    p = on.init_params(V, r, seed=8, perturb=0.2)
    inp, masks = small_case(r=r, V=V, B=B, Tt=Tt, Td=Td, seed=40 + B)
    run_stages(built_lib, 'B=%d %s r=%d' % (B, mode, r), p, inp, masks, B, Tt, Td, r, V,
               last_cluster=32 if mode in ('default', 'agent') else 8)   # (decoder.hip trains on 8 peers per row)


def _full_size(lib, tag, B, Tt, Td, parity):
    r, V = 2, 60
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    inp, masks = _full_case(B, Tt, Td, r, V)
    run_stages(lib, tag, None, inp, masks, B, Tt, Td, r, V, max_flips=64, parity=parity)


def test_stages_s1(built_lib):
    _full_size(built_lib, 'S1', 32, 200, 180, parity=False)


def test_s2_parity_and_stages(built_lib):
    """S2 (B=32, Tt=200, Td=500): outputs, alignments, loss, arg-max and every parameter gradient against fp64 (the bars of
    test_full_size_vs_oracle), then the stage map."""
    _full_size(built_lib, 'S2', 32, 200, 500, parity=True)


def test_b64_parity_and_stages(built_lib):
    """B=64 at S1 size (Tt=200, Td=180): decoder3 in two launches of 32 rows; same checks as S2."""
    _full_size(built_lib, 'B=64', 64, 200, 180, parity=True)
