"""GPU: the model at every reduction factor the ABI accepts (r = 1..5), against the fp64 restatements.

decoder3.hip is instantiated for r = 2 and 5 only (launch3_chunks); at r = 1, 3 and 4 the forward pass, BPTT and inference run
decoder.hip, whose r-dependent parts -- the feedback frame at column 80 (r - 1), the 128 + 80 r + 256 input segment, the
512 / 1024 output columns of dec_out_cols(r), the 128 / 256 / 512 wide FAN product of dec_fan_cols(r) -- are covered nowhere
else, and neither is the post-net on Td r rows of 1025 r floats.  r = 5 is also run on the fall-backs the decoder mode escalates
through after an exchange time-out (agent-scope decoder3, then decoder.hip).  Every case pins which decoder ran.

Tolerances are the suite's (tests/test_gpu_model.py): seq2seq_output / output rel-L2 <= 1e-5, alignments max-abs <= 1e-6, loss
rel <= 1e-5, every parameter gradient rel-L2 <= 2e-4 after the L1 sign ties are taken out; at the full corpus shape those of
test_full_size_vs_oracle (outputs rel-L2 <= 1e-4 / max-abs <= 1e-3, alignments max-abs <= 1e-5).  A gradient moved by a ReLU /
max-pool decision that fp32 and fp64 take differently is handled through tests/decisions.py as test_decoder3_cluster_geometries
handles it for B > 32 (B = 11 at r = 3 and at r = 5, and Tt = 300, each meet one such flip, within 6e-8 of its boundary)."""
import os

import numpy as np
import pytest
import torch

from oracle import taco_numpy as on
from oracle import taco_torch as ot
from tests.test_gpu_model import Runner, _argmax_check, _full_case, check_grads, f64, l1_tie_adjusted
from tests.util import report, small_case

pytestmark = pytest.mark.gpu

# last_cluster() after a launch: decoder3.hip runs clusters of 32 workgroups per row; decoder.hip 8 peers per row when training
# and 8 or 16 in inference (16 when B x 16 workgroups are co-resident)
DEC3, DEC = 'decoder3', 'decoder.hip'


def expect_route(lib, kernel, which, train):
    got = lib.last_cluster(which)
    what = ('forward', 'backward')[which] if train else 'inference'
    if kernel == DEC3:
        assert got == 32, '%s ran cluster width %d, expected decoder3.hip (32)' % (what, got)
    else:
        assert got in ((8,) if train else (8, 16)), '%s ran cluster width %d, expected decoder.hip' % (what, got)


def run_train(lib, p, inp, masks, B, Tt, Td, r, V, kernel, label, full=False):
    """forward + backward against ot.loss_and_grads, with the route pinned; prints the worst errors"""
    R = Runner(lib, B, Tt, Td, r, V)
    R.set(p, inp, masks)
    R.forward()
    expect_route(lib, kernel, 0, True)
    R.backward()
    expect_route(lib, kernel, 1, True)
    adj, n_ties = l1_tie_adjusted(R, p, inp, masks, r, Td)
    lt, s2, o2, a2, ref = ot.loss_and_grads(p, f64(adj), r, Td, f64(masks))
    r1, m1 = report('%s s2s' % label, R.s2s.cpu().numpy(), s2)
    r2, m2 = report('%s out' % label, R.out.cpu().numpy(), o2)
    _, m3 = report('%s align' % label, R.al.cpu().numpy(), a2)
    dl = abs(R.loss[0].item() - lt) / lt
    if full:
        assert r1 < 1e-4 and m1 < 1e-3 and r2 < 1e-4 and m2 < 1e-3 and m3 < 1e-5, (r1, m1, r2, m2, m3)
        n = _argmax_check(R.al.cpu().numpy(), a2, inp['text_length'])
        assert n > 1000
    else:
        assert r1 < 1e-5 and r2 < 1e-5 and m3 < 1e-6, (r1, r2, m3)
    assert dl <= 1e-5, dl
    bad = check_grads(R, ref)
    worst = _worst_grad(R, ref)
    n_flips = 0
    if bad:
        # a ReLU / max-pool pre-activation within fp32 rounding of its boundary may be decided differently by fp32 and fp64 (more
        # rows, more such decisions), which moves the tensors below it by ~1e-3.  Handled as test_decoder3_cluster_geometries does
        # for B > 32: the flips are read back from the workspace, each must sit within rounding of its boundary, every DECODER
        # tensor must meet the tolerance as it is, and with the HIP path's decisions imposed on the fp64 graph every tensor does.
        from tests.decisions import as_force, flips, hip_decisions
        hip, ok, _ = hip_decisions(R, p, masks, B, Tt, Td, r, 1)
        dec = ot.Decisions()
        ot.loss_and_grads(p, f64(adj), r, Td, f64(masks), dec=dec)
        fl = flips(hip, ok, dec)
        print('  %s: %d decision flip(s) vs fp64: %s; tensors off without forcing: %s' % (label, len(fl), fl[:6], bad))
        assert 1 <= len(fl) <= 16 and all(mg <= 1e-5 for _, _, mg in fl), fl
        assert not [n for n, _ in bad if n.startswith('decoder')], bad
        n_flips = len(fl)
        ref = ot.loss_and_grads(p, f64(adj), r, Td, f64(masks), dec=ot.Decisions(as_force(hip)))[4]
        bad = check_grads(R, ref)
        worst = _worst_grad(R, ref)
    assert not bad, bad
    print('  RESULT r=%d %-34s s2s %.2e out %.2e align %.2e loss %.2e grad %.2e (L1 ties %d, decision flips %d)' %
          (r, label, r1, r2, m3, dl, worst, n_ties, n_flips))


def _worst_grad(R, ref):
    got = R.pb.to_dict(R.grads)
    gmax = max(np.linalg.norm(v) for v in ref.values() if v is not None)
    w = 0.0
    for name, g in ref.items():
        g = np.zeros_like(got[name]) if g is None else g
        nr = np.linalg.norm(g)
        w = max(w, np.linalg.norm(got[name] - g) / (gmax if nr < 1e-6 * gmax else nr))
    return float(w)


def run_infer(lib, p, inp, B, Tt, Td, r, V, kernel, label):
    Ri = Runner(lib, B, Tt, Td, r, V, train=False)
    Ri.set(p, {'text': inp['text'][:B], 'text_length': inp['text_length'][:B]})
    Ri.infer()
    expect_route(lib, kernel, 0, False)
    si, oi, ai = on.forward(p, f64({'text': inp['text'][:B], 'text_length': inp['text_length'][:B]}), r, Td, train=False,
                            masks=None)[:3]
    r1, _ = report('%s infer s2s' % label, Ri.s2s.cpu().numpy(), si)
    r2, _ = report('%s infer out' % label, Ri.out.cpu().numpy(), oi)
    _, m3 = report('%s infer align' % label, Ri.al.cpu().numpy(), ai)
    assert r1 < 1e-5 and r2 < 1e-5 and m3 < 1e-6, (r1, r2, m3)
    print('  RESULT r=%d %-34s s2s %.2e out %.2e align %.2e' % (r, label + ' infer', r1, r2, m3))


@pytest.mark.parametrize('r,Tt,Td', [(1, 9, 5), (3, 23, 7), (4, 41, 9)])
def test_small_all_factors(built_lib, r, Tt, Td):
    """B = 2 with dropout and scheduled sampling: forward + backward + inference on decoder.hip."""
    V, B = 21, 2
    p = on.init_params(V, r, seed=50 + r, perturb=0.3)
    inp, masks = small_case(r=r, V=V, B=B, Tt=Tt, Td=Td, seed=60 + r)
    run_train(built_lib, p, inp, masks, B, Tt, Td, r, V, DEC, 'small')
    run_infer(built_lib, p, inp, B, Tt, Td, r, V, DEC, 'small')


@pytest.mark.parametrize('Td', [1, 2])
@pytest.mark.parametrize('r', [1, 4])
def test_shortest_decodes(built_lib, r, Td):
    """Td = 1 (no next step: no feedback frame is ever read) and Td = 2, as tests/test_gpu_model.py::test_shortest_decodes."""
    V, B, Tt = 19, 2, 9
    p = on.init_params(V, r, seed=4, perturb=0.3)
    inp, masks = small_case(r=r, V=V, B=B, Tt=Tt, Td=Td, seed=33)
    run_train(built_lib, p, inp, masks, B, Tt, Td, r, V, DEC, 'Td=%d' % Td)
    run_infer(built_lib, p, inp, B, Tt, Td, r, V, DEC, 'Td=%d' % Td)


@pytest.mark.parametrize('r,B', [(3, 1), (3, 11), (3, 20), (1, 20), (4, 20)])
def test_row_geometries(built_lib, r, B):
    """decoder.hip at several batch sizes (inference clusters of 16 while B x 16 workgroups fit, 8 beyond); B = 1 is the
    single-prompt inference shape (inference only)."""
    V, Tt, Td = 33, 41, 9
    p = on.init_params(V, r, seed=8, perturb=0.2)
    inp, masks = small_case(r=r, V=V, B=B, Tt=Tt, Td=Td, seed=40 + B)
    if B > 1:
        run_train(built_lib, p, inp, masks, B, Tt, Td, r, V, DEC, 'B=%d' % B)
    run_infer(built_lib, p, inp, B, Tt, Td, r, V, DEC, 'B=%d' % B)


@pytest.mark.parametrize('gemm2', ['default', 'forced'])
@pytest.mark.parametrize('r', [3, 4])
def test_medium_shape(built_lib, r, gemm2, monkeypatch):
    """B = 4, Tt = 37, Td = 12; `forced` (TACO_GEMM2_MIN_TILES=1) puts every eligible GEMM on the DMA kernel, the post-net's
    Td r row GEMMs and its 1025 r wide output rows included."""
    if gemm2 == 'forced':
        monkeypatch.setenv('TACO_GEMM2_MIN_TILES', '1')
    V, B, Tt, Td = 40, 4, 37, 12
    p = on.init_params(V, r, seed=4, perturb=0.2)
    inp, masks = small_case(r=r, V=V, B=B, Tt=Tt, Td=Td, seed=8)
    run_train(built_lib, p, inp, masks, B, Tt, Td, r, V, DEC, 'medium %s' % gemm2)
    run_infer(built_lib, p, inp, B, Tt, Td, r, V, DEC, 'medium %s' % gemm2)


def test_long_text_r3(built_lib):
    """Tt = 300 (> 256): decoder.hip's streamed attention rows at r = 3, forward + backward + B = 1 inference."""
    r, V, B, Tt, Td = 3, 25, 2, 300, 4
    p = on.init_params(V, r, seed=6, perturb=0.2)
    inp, masks = small_case(r=r, V=V, B=B, Tt=Tt, Td=Td, seed=12)
    inp['text_length'][:] = [300, 211]
    inp['text'][1, 211:] = 0
    run_train(built_lib, p, inp, masks, B, Tt, Td, r, V, DEC, 'Tt=300')
    run_infer(built_lib, p, inp, 1, Tt, Td, r, V, DEC, 'Tt=300 B=1')


@pytest.mark.parametrize('mode,B', [('v3_off', 11), ('v3_off', 20), ('agent', 11), ('agent', 20), ('decoder_mode(2)', 11)])
def test_r5_fallback_decoders(built_lib, mode, B, monkeypatch):
    """r = 5 on the decoders the process escalates to after an exchange time-out: decoder3's agent-scope exchange
    (TACO_DEC_V3_AGENT=1, mode 1) and decoder.hip (TACO_DEC_V3=0; and lib.decoder_mode(2), the route Tacotron.check() takes)."""
    r, V, Tt, Td = 5, 33, 41, 9
    if mode == 'agent':
        monkeypatch.setenv('TACO_DEC_V3_AGENT', '1')
    if mode == 'v3_off':
        monkeypatch.setenv('TACO_DEC_V3', '0')
    kernel = DEC3 if mode == 'agent' else DEC
    p = on.init_params(V, r, seed=8, perturb=0.2)
    inp, masks = small_case(r=r, V=V, B=B, Tt=Tt, Td=Td, seed=40 + B)
    prev = built_lib.decoder_mode(2) if mode == 'decoder_mode(2)' else None
    try:
        run_train(built_lib, p, inp, masks, B, Tt, Td, r, V, kernel, mode)
        run_infer(built_lib, p, inp, B, Tt, Td, r, V, kernel, mode)
    finally:
        if prev is not None:
            built_lib.decoder_mode(prev)


def test_full_corpus_shape_r3(built_lib):
    """What `preprocess --r 3` writes: B = 32, Tt = 200, Td = ((1 + 108000 // 300) // 12) * 4 = 120 -- 360 frames, a post-net
    over 3840 rows of 3075 floats -- forward + backward on decoder.hip against the fp64 restatement."""
    r, V, B, Tt = 3, 60, 32, 200
    Td = ((1 + 108000 // 300) // (4 * r)) * 4
    assert Td == 120
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    inp, masks = _full_case(B, Tt, Td, r, V)
    R = Runner(built_lib, B, Tt, Td, r, V)
    R.pb.init_(seed=0)
    p = R.pb.to_dict()
    del R
    run_train(built_lib, p, inp, masks, B, Tt, Td, r, V, DEC, 'full B=32 Tt=200 Td=120', full=True)
