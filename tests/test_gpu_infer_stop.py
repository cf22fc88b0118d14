"""taco_infer_stop: inference with end detection on the alignments (include/taco_hip.h, TacoStopRule).

Every check runs against a plain taco_infer of the same inputs: lengths equal the NumPy restatement of the rule
(tests/stop_ref.py) on that full decode's alignments, rows t < len_b of seq2seq_output / alignments are bit-identical to it,
every row from len_b on is exactly 0 in all three outputs, and `output` is the fp64 post-net of the zero-filled seq2seq_output.
In decoder modes 0 and 1 decoder3.hip evaluates the rule in its step loop and each cluster leaves the loop early; in mode 2
decoder.hip decodes all Td steps and a separate kernel applies the rule."""
import os
import wave

import numpy as np
import pytest
import torch

from oracle import taco_numpy as on
from tests.stop_ref import stop_lengths
from tests.util import rel_l2, small_case

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
MODES = {'default': {}, 'agent': {'TACO_DEC_V3_AGENT': '1'}, 'v3_off': {'TACO_DEC_V3': '0'}}


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


class Infer:
    """One inference workspace over the C ABI; every call gets fresh outputs pre-filled with NaN (a row nobody writes shows)."""

    def __init__(self, lib, p, text, text_length, Td, r, V):
        from tacotron_amd.params import ParamBuffer
        B, Tt = np.asarray(text).shape
        self.lib, self.B, self.Tt, self.Td, self.r = lib, B, Tt, Td, r
        self.shape = lib.make_shape(B, Tt, Td, r, V)
        self.pb = ParamBuffer(self.shape, 'cuda')
        self.pb.load_dict_(p)
        self.ws = torch.zeros(lib.workspace_bytes(self.shape, False) // 4, device='cuda')
        self.text = torch.as_tensor(np.asarray(text)).to('cuda', torch.int32).contiguous()
        self.tl = torch.as_tensor(np.asarray(text_length)).to('cuda', torch.int32).contiguous()
        self.err = [o for n, o, s, d in lib.workspace_table(self.shape, False) if n == 'dec.err'][0]

    def outputs(self):
        nan = float('nan')
        return (torch.full((self.B, self.Td, 80 * self.r), nan, device='cuda'),
                torch.full((self.B, self.Td, 1025 * self.r), nan, device='cuda'),
                torch.full((self.B, self.Td, self.Tt), nan, device='cuda'),
                torch.full((self.B,), -1, dtype=torch.int32, device='cuda'))

    def check_err(self):
        flags = self.ws[self.err:self.err + 2].view(torch.int32).cpu().numpy()
        assert flags[0] == 0 and flags[1] == 0, 'decoder cluster exchange timed out: %s' % flags

    def infer(self):
        s2s, out, al, _ = self.outputs()
        self.lib.infer(self.shape, self.pb.flat, self.text, self.tl, s2s, out, al, self.ws)
        torch.cuda.synchronize()
        self.check_err()
        return s2s.cpu().numpy(), out.cpu().numpy(), al.cpu().numpy()

    def infer_stop(self, rule):
        s2s, out, al, ln = self.outputs()
        self.lib.infer_stop(self.shape, self.pb.flat, self.text, self.tl, rule, s2s, out, al, ln, self.ws)
        torch.cuda.synchronize()
        self.check_err()
        return s2s.cpu().numpy(), out.cpu().numpy(), al.cpu().numpy(), ln.cpu().numpy()


def argmax_lengths(am, tl, Tt, end_offset, hold, min_steps):
    """the rule on precomputed argmaxes (B, Td), vectorised over rows (rule search only; tests/stop_ref.py is the yardstick)"""
    B, Td = am.shape
    target = np.maximum(0, np.clip(tl, 1, Tt) - 1 - end_offset)
    run = np.zeros(B, np.int64)
    out = np.full(B, Td, np.int64)
    done = np.zeros(B, bool)
    for t in range(Td):
        run = np.where(am[:, t] >= target, run + 1, 0)
        fire = ~done & (run >= hold) & (t + 1 >= min_steps)
        out[fire] = min(Td, 4 * ((t + 4) // 4))
        done |= fire
    return out


def spread_rule(lib, al, tl):
    """A rule whose lengths spread as widely as this (random-weight) decode allows: most distinct lengths, then most rows that
    stop strictly inside (4, Td)."""
    B, Td, Tt = al.shape
    am = al.argmax(-1)
    best, key = None, None
    for off in range(0, Tt):
        for hold in (1, 2, 3):
            for ms in (1, Td // 4):
                ln = argmax_lengths(am, np.asarray(tl), Tt, off, hold, ms)
                k = (len(set(ln.tolist())), int(((ln > 4) & (ln < Td)).sum()), -off)
                if key is None or k > key:
                    best, key = (off, hold, ms), k
    return lib.TacoStopRule(*best)


def check_stop(I, p64, full, rule, label):
    """taco_infer_stop against the full decode `full` (taco_infer on the same workspace and inputs); returns the lengths"""
    s2s_f, out_f, al_f = full
    s2s, out, al, ln = I.infer_stop(rule)
    want = stop_lengths(al_f, I.tl.cpu().numpy(), rule.end_offset, rule.hold, rule.min_steps)
    print('  %-28s %r lengths %s' % (label, rule, ln.tolist() if I.B <= 8 else sorted(set(ln.tolist()))))
    assert np.array_equal(ln, want), (ln, want)
    for b in range(I.B):
        L = int(ln[b])
        assert np.array_equal(bits(s2s[b, :L]), bits(s2s_f[b, :L])), 'seq2seq_output row %d differs before len_b' % b
        assert np.array_equal(bits(al[b, :L]), bits(al_f[b, :L])), 'alignments row %d differ before len_b' % b
        for name, x in (('seq2seq_output', s2s), ('output', out), ('alignments', al)):
            assert np.array_equal(bits(x[b, L:]), np.zeros_like(bits(x[b, L:]))), '%s row %d not 0 from len_b = %d' % (name, b, L)
    ref = on.postnet(p64, s2s.astype(np.float64), I.r)
    for b in range(I.B):
        ref[b, int(ln[b]):] = 0.0   # (the post-net runs over all Td steps; its rows from len_b on are then cleared)
    e = rel_l2(out, ref)
    print('  %-28s output vs fp64 post-net of the zero-filled decode: rel_l2 %.2e' % ('', e))
    assert e < 1e-5
    return ln


def _peaked():
    g = np.load(os.path.join(GOLD, 'model_r2_peaked.npz'))
    r, V, Td = int(g['r']), int(g['V']), int(g['Td'])
    p = on.init_params(V, r, seed=int(g['seed']), perturb=float(g['perturb']))
    for k, sc in zip(g['scaled_names'], g['scaled_by']):
        p[str(k)] = p[str(k)] * float(sc)
    return p, g['text'], g['text_length'], Td, r, V


def _random(B, Tt, Td, r, V, seed):
    p = on.init_params(V, r, seed=seed, perturb=0.2)
    inp, _ = small_case(r=r, V=V, B=B, Tt=Tt, Td=Td, seed=seed)
    return p, inp['text'], inp['text_length'], Td, r, V


def _full():
    from tacotron_amd.data import synthetic_batch
    b = synthetic_batch(32, 200, 180, 2, 60)
    return on.init_params(60, 2, seed=1, perturb=0.2), b['text'].numpy(), b['text_length'].numpy(), 180, 2, 60


CASES = {
    'peaked': _peaked,                                          # committed fixture: B=4, Tt=60, Td=40, r=2, peaked attention
    'r5': lambda: _random(6, 50, 24, 5, 33, 11),                # medium, r = 5
    'full': _full,                                              # B=32, Tt=200, Td=180, r=2
    'b1': lambda: _random(1, 30, 40, 2, 33, 12),
    'b48': lambda: _random(48, 41, 24, 2, 33, 13),              # two decoder3 launches (32 + 16 rows)
    'r3': lambda: _random(6, 50, 24, 3, 33, 14),                # r = 3 / 4: decoder.hip and the separate stop-rule kernel
    'r4': lambda: _random(6, 50, 24, 4, 33, 15),                #   in every mode (decoder3 has no r = 3 / 4 instantiation)
}


@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('case', list(CASES))
def test_prefix_identity_and_lengths(built_lib, case, mode, monkeypatch):
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    if case == 'full':
        torch.set_num_threads(min(os.cpu_count() or 1, 16))
    p, text, tl, Td, r, V = CASES[case]()
    p64 = {k: np.asarray(v, dtype=np.float64) for k, v in p.items()}
    I = Infer(built_lib, p, text, tl, Td, r, V)
    full = I.infer()
    assert (built_lib.last_cluster(0) == 32) == (mode != 'v3_off' and r in (2, 5))
    B = I.B
    # a rule chosen from this decode so that the lengths spread ...
    rule = spread_rule(built_lib, full[2], tl)
    ln = check_stop(I, p64, full, rule, '%s/%s spread' % (case, mode))
    if B > 1:
        assert len(set(ln.tolist())) >= 2, ln
    assert ln.min() < Td
    # ... and one that stops every row near Td / 2 (target 0: every step counts), so that every decoder3 cluster leaves early
    early = built_lib.TacoStopRule(end_offset=Tt_of(text), hold=1, min_steps=Td // 2)
    ln = check_stop(I, p64, full, early, '%s/%s early' % (case, mode))
    assert (ln == min(Td, 4 * ((Td // 2 + 3) // 4))).all()


def Tt_of(text):
    return int(np.asarray(text).shape[1])


@pytest.mark.parametrize('mode', ['default', 'v3_off'])
@pytest.mark.parametrize('case', ['r5', 'b48'])
def test_rule_that_never_fires_changes_nothing(built_lib, case, mode, monkeypatch):
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    p, text, tl, Td, r, V = CASES[case]()
    I = Infer(built_lib, p, text, tl, Td, r, V)
    s2s_f, out_f, al_f = I.infer()
    s2s, out, al, ln = I.infer_stop(built_lib.TacoStopRule(end_offset=0, hold=1, min_steps=Td + 1))
    assert (ln == Td).all(), ln
    for x, y in ((s2s, s2s_f), (out, out_f), (al, al_f)):
        assert np.array_equal(bits(x), bits(y))


def test_bad_arguments_enqueue_nothing(built_lib):
    p, text, tl, Td, r, V = CASES['b1']()
    I = Infer(built_lib, p, text, tl, Td, r, V)
    R = built_lib.TacoStopRule
    for rule, lengths, what in ((R(0, 0, 1), True, 'hold'), (R(-1, 1, 1), True, 'end_offset'), (R(0, 1, 0), True, 'min_steps'),
                                (R(0, 1, 1), False, 'lengths'), (None, True, 'rule')):
        s2s, out, al, ln = I.outputs()
        torch.cuda.synchronize()
        with pytest.raises(built_lib.TacoError) as ei:
            built_lib.infer_stop(I.shape, I.pb.flat, I.text, I.tl, rule, s2s, out, al, ln if lengths else None, I.ws)
        torch.cuda.synchronize()
        msg = str(ei.value)
        print('  %s: %s' % (what, msg))
        assert 'rc=-1' in msg and 'taco_infer_stop' in msg
        assert torch.isnan(s2s).all() and torch.isnan(out).all() and torch.isnan(al).all() and (ln == -1).all()


def _model(Td=12, B=2, Tt=24, seed=3):
    from tacotron_amd.config import Config
    from tacotron_amd.data import synthetic_batch
    from tacotron_amd.model import Tacotron
    c = Config()
    c.r, c.vocab_size, c.max_decode_iter = 2, 30, Td
    b = synthetic_batch(B, Tt, Td, 2, 30, seed=seed, min_len=8)
    return Tacotron(c, b, train=False, seed=5)


def test_inference_with_stop_is_graph_capturable(built_lib):
    """A captured taco_infer_stop replays to the eager outputs and lengths, bit for bit."""
    m = _model()
    rule = built_lib.TacoStopRule(end_offset=100, hold=1, min_steps=5)   # target 0: every row stops after step 4 -> len 8
    m.run(stop=rule)
    torch.cuda.synchronize()
    ref = (m.seq2seq_output.clone(), m.output.clone(), m.alignments.clone(), m.lengths.clone())
    assert (ref[3] == 8).all() and (ref[1][:, 8:] == 0).all() and (ref[1][:, :8] != 0).any()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m.run(stop=rule)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            m.run(stop=rule)
    torch.cuda.synchronize()
    for x in (m.seq2seq_output, m.output, m.alignments):
        x.fill_(float('nan'))
    m.lengths.fill_(-1)
    g.replay()
    torch.cuda.synchronize()
    for x, y in zip((m.seq2seq_output, m.output, m.alignments, m.lengths), ref):
        assert torch.equal(x, y)
    m.check()


def test_model_run_sets_lengths(built_lib):
    m = _model(Td=24, B=3, Tt=30, seed=4)
    out, al = m.run()
    assert m.lengths is None
    al_full = al.cpu().numpy()
    s2s_full = m.seq2seq_output.cpu().numpy()
    rule = spread_rule(built_lib, al_full, m.inputs['text_length'].cpu().numpy())
    out2, al2 = m.run(stop=rule)
    assert out2 is m.output and al2 is m.alignments
    ln = m.lengths.cpu().numpy()
    assert ln.dtype == np.int32 and ln.shape == (3,)
    assert np.array_equal(ln, stop_lengths(al_full, m.inputs['text_length'].cpu().numpy(), rule.end_offset, rule.hold, rule.min_steps))
    s2s = m.seq2seq_output.cpu().numpy()
    for b in range(3):
        assert np.array_equal(bits(s2s[b, :ln[b]]), bits(s2s_full[b, :ln[b]])) and not s2s[b, ln[b]:].any()
    m.run()
    assert m.lengths is None
    m.check()


def test_cli_stop_trims_and_default_is_unchanged(built_lib, tmp_path):
    """tacotron_amd.test.test: with a rule every file is cut to len_b; without one the WAVs are byte-identical to the path the
    driver takes without the option (taco_infer -> Griffin-Lim -> write_wav, restated here)."""
    from tacotron_amd import test as drv
    from tacotron_amd.config import Config
    from tacotron_amd.data import load_prompts
    from tacotron_amd.griffinlim import invert_spectrogram
    from tacotron_amd.model import Tacotron
    from tacotron_amd.params import ParamBuffer
    prompts = ['hello world.\n', 'a somewhat longer prompt, with punctuation!\n', 'short\n']

    def cfg():
        c = Config()
        c.data_path = str(tmp_path / 'no_data') + '/'
        c.max_decode_iter = 16
        return c

    plain, cut, ref = tmp_path / 'plain', tmp_path / 'cut', tmp_path / 'ref'
    assert drv.test(cfg(), prompts, out_dir=str(plain), n_iter=2) == 3
    rule = built_lib.TacoStopRule(end_offset=200, hold=1, min_steps=5)   # target 0: len_b = 8 for every prompt
    assert drv.test(cfg(), prompts, out_dir=str(cut), n_iter=2, stop=rule) == 3
    # the driver's path without the option, restated
    c = cfg()
    ivocab = {i + 1: ch for i, ch in enumerate("abcdefghijklmnopqrstuvwxyz '.,?!-")}
    ivocab[0] = '<pad>'
    c.vocab_size = len(ivocab)
    os.makedirs(ref)
    batch = next(load_prompts(prompts, ivocab))
    shape = built_lib.make_shape(3, batch['text'].shape[1], c.max_decode_iter, c.r, c.vocab_size, c.num_speakers)
    m = Tacotron(c, batch, train=False, params=ParamBuffer(shape, 'cuda').init_(0))
    out, _ = m.run()
    F = c.fft_size * c.r
    wav = invert_spectrogram(out, torch.zeros(F).cuda(), torch.ones(F).cuda(), c.r, n_iter=2, seed=0).cpu().numpy()
    for i in range(3):
        drv.write_wav(str(ref / ('prompt_%03d.wav' % i)), wav[i])
        a = open(plain / ('prompt_%03d.wav' % i), 'rb').read()
        assert a == open(ref / ('prompt_%03d.wav' % i), 'rb').read()
        assert not (plain / ('prompt_%03d_len.npy' % i)).exists()
        assert int(np.load(cut / ('prompt_%03d_len.npy' % i))) == 8
        with wave.open(str(cut / ('prompt_%03d.wav' % i))) as f:
            assert f.getnframes() == 300 * (8 * c.r - 1)
        with wave.open(str(plain / ('prompt_%03d.wav' % i))) as f:
            assert f.getnframes() == 300 * (16 * c.r - 1)
        assert np.load(cut / ('prompt_%03d_spec.npy' % i)).shape == (8 * c.r, 1025)
        assert np.load(cut / ('prompt_%03d_align.npy' % i)).shape == (8, batch['text'].shape[1])
