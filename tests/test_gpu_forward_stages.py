"""GPU: the forward pass stage by stage, row by row.  Every buffer taco_forward (or taco_infer) leaves in the workspace, and its
three outputs, are compared with the value of the matching intermediate in the fp64 oracle (oracle.taco_torch.Recorder with
values=True): as a whole tensor (rel-L2 <= FWD_TENSOR_BAR) and per row -- one (b, t) frame, text position or decoder step,
dec.stash field by field -- against FWD_ROW_BAR (tests/stage_bars.py).  The forward pass itself never reads most of the decoder
stash (R, U, C, RH, H, Y feed the weight-gradient GEMMs only), so a mistake confined to one (b, t) record, one 32-row tile edge
of the post-net or one sampled row surfaces as a slightly wrong parameter gradient at best; here it is one row off.  Every
compared workspace tensor is filled with quiet NaN before the call: a row nobody wrote fails instead of reading as an old value.
Where the math makes a value zero, or a copy, it must be exactly that.

The buffer map (tests/forward_map.py; taken from the code that writes each buffer -- model.hip forward_impl / cbhg_fwd,
decoder3.hip / decoder.hip, highway.hip, bigru.hip, prenet.hip; offsets K_ST_* in tests/decisions.py = kSt* of csrc/kernels.h):
  enc.emb (B Tt, 256)       embedding rows, bit-identical
  enc.p1, enc.p2            encoder pre-net after ReLU and dropout; exactly 0 where dropout dropped the unit
  per CBHG (enc. over (B, Tt), post. over (B, Td r), the post-net's input being seq2seq_output read as (B, Td r, 80)):
    bank                    conv bank after its ReLU (kept for the backward pass: training only)
    pool                    max-pool(2, 1, same) of the BN affine of bank
    pj1pre, pj1             proj1 after its ReLU; after its BN affine (the proj2 input)
    pj2pre, res             proj2 before its BN affine; after it plus the CBHG input (= highway input h0)
    hx<l>                   highway layer l's input after its adapter, where it has one (post-net: l = 0; encoder: every layer
                            when S > 1, the speaker vector entering as a per-sequence bias)
    th<l> (M, 256)          [T | H]: layer l's sigmoid gate and ReLU candidate (training only)
    h<l+1>                  layer l's output H T + x (1 - T)
    out (M, 256)            bi-GRU output [fw | bw]
    ruc (M, 768)            [fw r | u | c | bw r | u | c] of the bi-GRU at the row's own time step (training only)
    xg                      scratch (x-side projections of the bi-GRU): not compared
  enc.spk_e (B, 16), enc.sv_h0 (5, B, 128)   S > 1: speaker embedding rows; ReLU'd speaker vectors of the four highway layers
                            and the bi-GRU's initial state
  dec.values, dec.keys      encoder output masked past text_length, and its memory-layer product; rows >= text_length exactly 0
  dec.vwx, dec.vwg          values Wx_c and values Wx_c Wg0_x with Wx_c = Wa[80r:] Wi[128:] (layout.hip), formed in fp64 from the
                            parameters
  dec.vcen, dec.vwxc        training only (model.hip forms them under `train`): values minus the mean of the row's first
                            text_length positions, and that times Wx_c; rows >= text_length exactly 0 in both
  dec.stash (B, Td, kStRec) training only, per step t:
    P1 (256), P2 (128)      pre-net of step t after ReLU and dropout: written for every step by two GEMMs over the teacher frames
                            (model.hip), overwritten by the decoder kernel in the record of step t + 1 where sample[t, b] feeds
                            the step its predecessor's output; exactly 0 where dec_keep1 / dec_keep2 is 0
    X                       in-proj output x
    H, R, U, C, RH (3x256)  per GRU layer: new state, gates r and u, candidate c, r * h_prev
    Q, Y                    query; x + h3 (the out-proj input)
    Ctx, Att (2x256)        written by neither decoder kernel: must still hold the poison
    (these twelve tile [0, kStRec) exactly, and kStRec is the record width of the workspace table: asserted)
  dec.prein (B Td, 80)      training only: the pre-net input frame step t used, bit-identical to the last frame of mel[b, t]
                            (step 0 and teacher-forced steps; one strided copy in model.hip, or decoder.hip itself) or of the HIP
                            path's own seq2seq_output[b, t - 1] (fed steps; written by the decoder kernel)
  seq2seq_output, output, alignments   per (b, t); alignment columns >= text_length exactly 0
Every other enc. / dec. / post. tensor of the workspace table must be in forward_map.NOT_COMPARED: a tensor added later cannot
go unnoticed.

Discrete decisions: a ReLU or max-pool decision taken differently in fp32 leaves the forward values continuous, so the oracle
runs unforced; the flips are still bounded as in the backward tests (count <= 16, each fp64 margin <= 1e-5) and printed.

Measured on MI355X (each test prints its full table); the bars are 4x the worst of each column, rounded up to one digit:
  shape                      worst tensor rel-L2        worst row                            decision flips
  golden r=2                 6.440e-7 (post.pj2pre)     1.183e-6 (dec.vcen, b 1, s 2)        0
  golden r=5                 6.471e-7 (post.pj2pre)     1.420e-6 (dec.vwxc, b 1, s 2)        0
  golden spk                 7.105e-7 (post.pj2pre)     1.381e-6 (dec.vcen, b 1, s 2)        0
  ragged medium              7.529e-7 (post.pj2pre)     1.931e-6 (dec.vwxc, b 1, s 7)        0
  decoder3 B=11 r=2          8.401e-7 (dec.vwxc)        1.983e-6 (dec.vwxc, b 4, s 8)        0
  decoder3 B=40 r=5          8.574e-7 (dec.vwxc)        2.134e-6 (dec.vwxc, b 12, s 9)       1 (post pool, margin 2.0e-7)
  decoder3 B=70 r=5          8.492e-7 (dec.vwxc)        2.210e-6 (dec.vwxc, b 45, s 10)      0
  agent B=12 r=2             8.263e-7 (dec.vwxc)        2.177e-6 (dec.vwxc, b 7, s 8)        0
  decoder.hip B=5 r=2        8.377e-7 (dec.vwxc)        1.769e-6 (dec.vcen, b 4, s 7)        0
  decoder.hip B=4 r=3        8.373e-7 (dec.vwxc)        2.103e-6 (dec.vwxc, b 2, s 9)        0
  infer golden r=2           5.290e-7 (post.pj2pre)     6.978e-7 (post.pj2pre, b 1, f 8)     0
  infer decoder.hip B=5      6.348e-7 (post.pj2pre)     8.123e-7 (post.pj2pre, b 4, f 12)    0
  The worst rows are the centred memory rows (a difference of two nearly equal fp32 numbers) and their fold; every dec.stash
  field is <= 1.1e-6 per row (P2 of a fed step), every encoder and post-net buffer <= 1.2e-6 (post.pj2pre).  Every exact-zero site was
  exactly zero, every copy bit-identical, the Ctx / Att slots still poisoned.  The twelve cases take 5 s together.
"""
import numpy as np
import pytest

from oracle import taco_numpy as on
from tests import forward_map as fm
from tests.decisions import flips, hip_decisions
from tests.test_gpu_model import Runner, golden
from tests.util import small_case

pytestmark = pytest.mark.gpu


def _decisions(R, p, masks, B, Tt, Td, r, S, train):
    """The HIP path's observable ReLU / max-pool decisions: all of them after taco_forward; at inference those whose buffers
    taco_infer keeps (no stash, no bank, no highway candidates)."""
    if train:
        return hip_decisions(R, p, masks, B, Tt, Td, r, S)[:2]
    d = {'encoder/pre_net/l1': (R.wsget('enc.p1') > 0).reshape(B, Tt, -1), 'encoder/pre_net/l2': (R.wsget('enc.p2') > 0).reshape(B, Tt, -1)}
    for pre, prefix, T in (('enc', 'encoder/cbhg/', Tt), ('post', 'post/cbhg/', Td * r)):
        d[prefix + 'proj1'] = (R.wsget(pre + '.pj1pre') > 0).reshape(B, T, -1)
    return d, {}


def run_forward_stages(lib, tag, p, inp, masks, B, Tt, Td, r, V, S=1, train=True, max_flips=16, last_cluster=None):
    """taco_forward (train) or taco_infer on poisoned buffers, one fp64 oracle forward with the value recorder, then every mapped
    buffer against its reference.  Returns the compare() results; asserts at the end, after printing everything."""
    if train:
        bad = fm.mask_coverage_failures(masks, B, Td)
        assert not bad, bad
    R = Runner(lib, B, Tt, Td, r, V, train=train, S=S)
    R.set(p, inp if train else {k: v for k, v in inp.items() if k in ('text', 'text_length', 'speaker')}, masks if train else None)
    V64, dec = fm.oracle_forward(p, inp, masks, r, Td, train)
    ref = fm.build_reference(V64, p, inp, B, Tt, Td, r, S, train)
    outs = {'seq2seq_output': R.s2s, 'output': R.out, 'alignments': R.al}
    names = [n for n in ref if n not in outs] + (['dec.prein'] if train else [])
    # the map and the workspace table account for each other
    missing = [n for n in names if n not in R.wtab]
    assert not missing, missing
    loose = [n for n in R.wtab if n.split('.')[0] in ('enc', 'dec', 'post') and n not in names and not n.startswith('dec.comp.')
             and n not in fm.NOT_COMPARED and n.split('.', 1)[1] not in fm.NOT_COMPARED
             and not (not train and n.split('.', 1)[1] in fm.TRAIN_ONLY)]
    assert not loose, 'forward workspace tensors neither compared nor listed in forward_map.NOT_COMPARED: %s' % loose
    if train:
        tiling = fm.stash_tiling_failures(R.wtab['dec.stash'][2][-1])
        assert not tiling, tiling
    for n in names:
        o, s, _ = R.wtab[n]
        R.ws[o:o + s] = float('nan')
    for t in outs.values():
        t.fill_(float('nan'))
    R.forward() if train else R.infer()
    if last_cluster is not None:
        assert lib.last_cluster(0) in last_cluster, lib.last_cluster(0)
    hip, ok = _decisions(R, p, masks, B, Tt, Td, r, S, train)
    fl = flips(hip, ok, dec)
    print('  %s: %d decision flips vs fp64%s' % (tag, len(fl), ''.join('\n    %-34s %-16s fp64 margin %.2e' % f for f in fl[:20])))
    bufs = {n: R.wsget(n) for n in names}
    bufs.update({k: v.cpu().numpy() for k, v in outs.items()})
    res, bad = fm.check_forward(bufs, ref, inp, masks, B, Tt, Td, r, train)
    fm.print_table(tag, res, ', flips %d' % len(fl))
    assert len(fl) <= max_flips and all(mg <= 1e-5 for _, _, mg in fl), fl
    assert not bad, bad
    return res


@pytest.mark.parametrize('r', [2, 5])
def test_forward_stages_golden(built_lib, r):
    g, p, inp, masks = golden(r)
    run_forward_stages(built_lib, 'golden r=%d' % r, p, inp, masks, int(g['B']), int(g['Tt']), int(g['Td']), r, int(g['V']))


def test_forward_stages_golden_multi_speaker(built_lib):
    g, p, inp, masks = golden(2, spk=True)
    # (the fixture's own sample mask has no row whose step t is fed and whose step t + 1 is teacher-forced)
    masks = dict(masks, sample=np.array([[1, 0], [0, 1], [1, 0], [0, 1], [0, 0]], np.uint8))
    run_forward_stages(built_lib, 'golden spk', p, inp, masks, int(g['B']), int(g['Tt']), int(g['Td']), 2, int(g['V']),
                       S=int(g['num_speakers']))


def ragged_medium_case():
    """B=4, Tt=37, Td=12 with one text_length of 1 (the n = 1 edge of center_rows)."""
    r, V, B, Tt, Td = 2, 40, 4, 37, 12
    p = on.init_params(V, r, seed=4, perturb=0.2)
    inp, masks = small_case(r=r, V=V, B=B, Tt=Tt, Td=Td, seed=8)
    inp['text_length'][2] = 1
    inp['text'][2, 1:] = 0
    return p, inp, masks, B, Tt, Td, r, V


def test_forward_stages_ragged_medium(built_lib):
    p, inp, masks, B, Tt, Td, r, V = ragged_medium_case()
    run_forward_stages(built_lib, 'ragged medium', p, inp, masks, B, Tt, Td, r, V)


def _geometry_case(B, r):
    V, Tt, Td = 33, 41, 9
    p = on.init_params(V, r, seed=8, perturb=0.2)
    inp, masks = small_case(r=r, V=V, B=B, Tt=Tt, Td=Td, seed=40 + B)
    return p, inp, masks, B, Tt, Td, r, V


@pytest.mark.parametrize('B,mode,r', [(11, 'default', 2), (40, 'default', 5), (70, 'default', 5), (12, 'agent', 2),
                                      (5, 'v3_off', 2), (4, 'r3', 3)])
def test_forward_stages_decoder_geometries(built_lib, B, mode, r, monkeypatch):
    """Both decoder kernels: decoder3 with a partly filled last cluster (B=11), second and third 32-row launches (B=40, 70 at
    r=5), the agent-scope exchange (B=12), decoder.hip as the fall-back (TACO_DEC_V3=0) and at r=3 (outside decoder3's
    instantiations)."""
    if mode == 'agent':
        monkeypatch.setenv('TACO_DEC_V3_AGENT', '1')
    if mode == 'v3_off':
        monkeypatch.setenv('TACO_DEC_V3', '0')
    p, inp, masks, B, Tt, Td, r, V = _geometry_case(B, r)
    run_forward_stages(built_lib, 'B=%d %s r=%d' % (B, mode, r), p, inp, masks, B, Tt, Td, r, V,
                       last_cluster=(32,) if mode in ('default', 'agent') else (8,))   # (decoder.hip trains on 8 peers per row)


@pytest.mark.parametrize('case', ['golden r=2', 'B=5 v3_off'])
def test_forward_stages_infer(built_lib, case, monkeypatch):
    """taco_infer: the inference workspace (no stash, no gate stashes) and the post-net over free-running output; decoder3 on
    the fixture, decoder.hip (8 or 16 peers per row at inference) with TACO_DEC_V3=0."""
    if case == 'golden r=2':
        g, p, inp, masks = golden(2)
        B, Tt, Td, r, V = int(g['B']), int(g['Tt']), int(g['Td']), 2, int(g['V'])
        cluster = (32,)
    else:
        monkeypatch.setenv('TACO_DEC_V3', '0')
        p, inp, masks, B, Tt, Td, r, V = _geometry_case(5, 2)
        cluster = (8, 16)
    run_forward_stages(built_lib, 'infer ' + case, p, inp, None, B, Tt, Td, r, V, train=False, last_cluster=cluster)
