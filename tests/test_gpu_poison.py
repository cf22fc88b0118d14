"""GPU: the model-level entry points on POISONED workspaces and outputs, between guard bands (tests/poison.py).

The C ABI hands the library a workspace and outputs with arbitrary contents (include/taco_hip.h; tacotron_amd/model.py allocates
them with torch.empty); only `dec.err` is prepared by the caller (taco_clear_error, once on a fresh workspace).  Every other
test of the suite runs on memory that started as zeros.  Here each case runs once CLEAN -- a zero-filled `Runner`, the state the
oracle comparisons of the suite hold to fp64 at exactly these shapes -- and then in a guarded arena whose workspace, outputs,
loss, gradient buffer and lengths are filled with `qnan`, `ones`, `noise`, or carry a FOREIGN history: a complete forward +
backward (or infer + infer_stop) on the same workspace with other parameters, text, lengths, targets and masks.  Asserted:
  a. seq2seq_output, output, alignments, loss (and `lengths` of taco_infer_stop) are BIT-identical to the clean run; gradients are
     bit-identical under TACO_DETERMINISTIC=1 and in the default mode (fp32 atomics decide summation orders) within rel-L2 1e-5 of
     the whole flat buffer, the bar of test_deterministic_gradient_mode, with every element finite.  That two clean runs in two
     separately carved arenas agree in this way is established first, per case;
  b. no element of a documented output still holds poison (gradients of parameters that took no part and the rows
     taco_infer_stop clears included), the guard bands are bytewise intact, and so are the gaps of the workspace table;
  c. the same after a foreign history, and across shapes (one workspace arena used for two layouts in turn);
  d. at the smallest shape, poison in ONE family of workspace tensors at a time, so that a failure names the family.
Nothing here makes a kernel misbehave: the poison goes only where the contract allows arbitrary contents, `dec.err` is cleared
through taco_clear_error after every fill and before the first launch, and Runner.check_err() runs after every call.

Measured on MI355X (44 tests, 15 s; the whole GPU suite 148 s for 440 tests against 147 s for 396 of the parent commit on the
same box, same library build): every case below -- the golden fixtures r = 2 / r = 5 / multi-speaker, ragged lengths without
masks, Td = 1 and 2, r = 3 on decoder.hip, B = 11 / 40 / 70 (chunked launches at r = 5), B = 12 agent-scope exchange,
TACO_DEC_V3=0, taco_decoder_mode(2), the medium shape with gemm2 forced (32x2, 16x3) and with TACO_GEMM2_BSPLIT=0, the pooled
epilogue edges (3, 127, 64) and (2, 128, 9), inference at B = 1 and B = 48, S1 (qnan and foreign only) -- was BIT-identical to the
clean run in seq2seq_output, output, alignments, loss and lengths under qnan, ones, noise and a foreign history, for
taco_forward, taco_infer and taco_infer_stop; gradients bit-identical under TACO_DETERMINISTIC=1 and within rel-L2 1.2e-7 of the
clean run in the default mode (two clean runs in two arenas: the same 1e-7, and 0 at the smallest shapes); no output element was
left unwritten, no guard band or table gap touched.  No dependence on prior contents was found, so tests/poison.py lists no
exemption.  That the file can fail was checked with three scratch builds of the library that each lacked one of the init
fills of model.hip (pad rows of bwd.paramsT + pad columns of bwd.comp.fa; the bwd.dkeys_e accumulator; the gradient buffer):
each failed the train cases with non-finite gradients, and the first two failed test_localisation_by_workspace_family[bwd.] only.

Integer-typed readers of caller memory, and what writes each before it is read: dec.err words and census / trace words
(taco_clear_error; compared with 0 or added to, never an index); dec.xchg granule epochs and decoder3's placement table
(the init batch of taco_forward / taco_backward / the inference path zeroes the area in front of every decoder launch,
decoder.hip zeroes it for itself; values are compared, never an index); `lengths` (written for every valid row by decoder3's
lead workgroup or by stop_rule_kernel before zero_tail_rows_kernel reads it, and that kernel's row loop is bounded by B * Td
whatever it reads); the feature front end's length / mel-range words and bounds / kept (host upload, fb_ranges_kernel and
fb_trim_kernel, all in front of fb_frames_kernel).  Every other index comes from an input (text, text_length, speaker).
"""
import os

import numpy as np
import pytest
import torch

from oracle import taco_numpy as on
from tests import poison
from tests.test_gpu_infer_stop import spread_rule
from tests.test_gpu_model import Runner, _full_case, golden
from tests.util import small_case

pytestmark = pytest.mark.gpu

GUARD_FLOATS = 4096          # 16 KiB of sentinel around every buffer (a 128 x 1028 tile's row overrun lands inside it)
ALL = ('qnan', 'ones', 'noise')
OUT_NAMES = ('s2s', 'out', 'al', 'loss', 'grads')


def bits(t):
    return t.detach().contiguous().view(-1).view(torch.int32).cpu().numpy()


class PoisonRunner(Runner):
    """`Runner` with workspace, s2s, out, al, loss, grads and lengths carved from ONE guarded arena.  (Runner.__init__ is not
    called: it would allocate zero-filled twins of every buffer.)  `share`: another PoisonRunner whose workspace memory this
    one uses -- two layouts over the same bytes; `ws_floats`: a workspace buffer larger than this shape needs."""

    def __init__(self, lib, B, Tt, Td, r, V, train=True, S=1, ws_floats=None, share=None):
        from tacotron_amd.params import ParamBuffer
        self.lib, self.train = lib, train
        self.speaker = None
        self.B, self.Td = B, Td
        self.shape = lib.make_shape(B, Tt, Td, r, V, S)
        self.pb = ParamBuffer(self.shape, 'cuda')
        self.table = lib.workspace_table(self.shape, train)
        self.wtab = {n: (o, s, d) for n, o, s, d in self.table}
        need = lib.workspace_bytes(self.shape, train) // 4
        sizes = [('s2s', B * Td * 80 * r), ('out', B * Td * 1025 * r), ('al', B * Td * Tt), ('loss', 3),
                 ('grads', self.pb.numel), ('lengths', B)]
        if share is None:
            sizes.insert(0, ('ws', max(need, ws_floats or 0)))
        self.arena = poison.carve(sizes, GUARD_FLOATS, 'cuda')
        self.owner = share or self
        self.ws_full = share.ws_full if share is not None else self.arena.f32('ws')
        assert self.ws_full.numel() >= need
        self.ws = self.ws_full[:need]
        self.s2s = self.arena.f32('s2s', B, Td, 80 * r)
        self.out = self.arena.f32('out', B, Td, 1025 * r)
        self.al = self.arena.f32('al', B, Td, Tt)
        self.loss = self.arena.f32('loss')
        self.grads = self.arena.f32('grads')
        self.lengths = self.arena.view('lengths', torch.int32)
        self.gaps = poison.table_gaps(self.table, need)
        self.marks = {}

    def buffers(self):
        return {'ws': self.ws_full, 's2s': self.s2s, 'out': self.out, 'al': self.al, 'loss': self.loss, 'grads': self.grads,
                'lengths': self.lengths}

    def clear_error(self):
        """what the header prescribes for a fresh workspace; the bounded spins of the decoders must see clean words"""
        self.lib.clear_error(self.shape, self.train, self.ws)
        torch.cuda.synchronize()
        self.check_err()

    def fill(self, pattern, only=None):
        """`pattern` into the workspace and every output (only = [(offset, size)]: into those workspace ranges alone, zeros
        everywhere else), then taco_clear_error."""
        self.marks = {}
        for i, (name, buf) in enumerate(self.buffers().items()):
            if only is None:
                self.marks[name] = poison.poison(buf, pattern, seed=11 + i, scale=1.0)
            else:
                poison.poison(buf, 'zeros')
        if only is not None:
            for j, (o, s) in enumerate(only):
                poison.poison(self.ws[o:o + s], pattern, seed=31 + j, scale=1.0)
        self.clear_error()

    def infer_stop(self, rule):
        self.lib.infer_stop(self.shape, self.pb.flat, self.text, self.tl, rule, self.s2s, self.out, self.al, self.lengths, self.ws,
                            self.speaker)
        torch.cuda.synchronize()
        self.check_err()

    def results(self, names):
        return {n: bits(self.buffers()[n]) for n in names}

    def check_coverage(self, names, label):
        """(b): the named outputs hold no poison; guard bands, table gaps and the workspace floats behind this layout intact"""
        for n in names:
            if n in self.marks:
                ok, first, count = poison.fully_written(self.buffers()[n], self.marks[n])
                assert ok, '%s: %d element(s) of %s still hold the poison, first at flat index %d' % (label, count, n, first)
        for R in {self, self.owner}:
            rep = poison.guards_intact(R.arena)
            assert rep, '%s: %r' % (label, rep)
        mark = self.marks.get('ws')
        if mark is not None:
            spans = self.gaps + ([(self.ws.numel(), self.ws_full.numel())] if self.ws_full.numel() > self.ws.numel() else [])
            for lo, hi in spans:
                m = mark if isinstance(mark, str) else mark[lo:hi]
                assert bool(poison.untouched(self.ws_full[lo:hi], m).all()), \
                    '%s: workspace floats [%d, %d), which no table row covers, were written' % (label, lo, hi)


def same_bits(got, ref, names, label):
    for n in names:
        d = int((got[n] != ref[n]).sum())
        print('  %-44s %-8s %s' % (label, n, 'bit-identical' if d == 0 else '%d of %d words differ' % (d, ref[n].size)))
    for n in names:
        assert np.array_equal(got[n], ref[n]), '%s: %s differs from the clean run' % (label, n)


def close_grads(got, ref, label):
    g, r = got['grads'].view(np.float32).astype(np.float64), ref['grads'].view(np.float32).astype(np.float64)
    finite = bool(np.isfinite(g).all())
    rel = float(np.linalg.norm(g - r) / np.linalg.norm(r)) if finite else float('nan')
    print('  %-44s %-8s rel-L2 %.2e to the clean run, finite: %s' % (label, 'grads', rel, finite))
    assert finite, '%s: non-finite gradient element(s)' % label
    assert rel < 1e-5, '%s: gradients rel-L2 %.2e from the clean run' % (label, rel)


def clean_infer_stop(lib, C, rule):
    """taco_infer_stop on a zero-filled `Runner` (which has no lengths buffer of its own); returns the lengths tensor"""
    ln = torch.zeros(C.shape.B, dtype=torch.int32, device='cuda')
    lib.infer_stop(C.shape, C.pb.flat, C.text, C.tl, rule, C.s2s, C.out, C.al, ln, C.ws, C.speaker)
    torch.cuda.synchronize()
    C.check_err()
    return ln


def foreign_of(c):
    """other parameters (another init seed: every weight differs, not at the rounding level), text, lengths, targets, masks"""
    S = c.get('S', 1)
    if c.get('device_init'):
        p = None
    else:
        p = on.init_params(c['V'], c['r'], seed=977, perturb=0.25, num_speakers=S)
    inp, masks = small_case(r=c['r'], V=c['V'], B=c['B'], Tt=c['Tt'], Td=c['Td'], seed=4242, full_len_row0=False)
    if S > 1:
        inp['speaker'] = (np.arange(c['B']) * 3 + 1).astype(np.int32) % S
    return p, inp, masks


def load(R, c, p, inp, masks, seed):
    if p is None:                       # full size: parameters drawn on the host by ParamBuffer.init_ (as the S1 tests do)
        R.pb.init_(seed=seed)
        R.text = torch.as_tensor(inp['text']).to('cuda', torch.int32).contiguous()
        R.tl = torch.as_tensor(inp['text_length']).to('cuda', torch.int32).contiguous()
        if 'mel' in inp:
            R.mel = torch.as_tensor(inp['mel']).to('cuda', torch.float32).contiguous()
            R.stft = torch.as_tensor(inp['stft']).to('cuda', torch.float32).contiguous()
        R.masks = {k: torch.as_tensor(v).to('cuda', torch.uint8).contiguous() for k, v in (masks or {}).items()}
    else:
        R.set(p, inp, masks)


def run_train_case(lib, c, monkeypatch, label):
    for k, v in c.get('env', {}).items():
        monkeypatch.setenv(k, v)
    prev = lib.decoder_mode(c['decoder_mode']) if 'decoder_mode' in c else None
    try:
        _train_case(lib, c, monkeypatch, label)
    finally:
        if prev is not None:
            lib.decoder_mode(prev)


def _train_case(lib, c, monkeypatch, label):
    dims = (c['B'], c['Tt'], c['Td'], c['r'], c['V'])
    S = c.get('S', 1)
    p, inp, masks = c.get('p'), c['inp'], c['masks']
    fp, finp, fmasks = foreign_of(c)
    outs = ('s2s', 'out', 'al', 'loss')

    def step(R):
        R.forward()
        if 'cluster' in c:
            assert lib.last_cluster(0) == c['cluster']
        R.backward()
        if 'cluster' in c:
            assert lib.last_cluster(1) == c['cluster']

    P = PoisonRunner(lib, *dims, S=S)
    for det in (False, True):
        if det:
            monkeypatch.setenv('TACO_DETERMINISTIC', '1')
        tag = '%s%s' % (label, ' det' if det else '')
        C = Runner(lib, *dims, S=S)
        load(C, c, p, inp, masks, 3)
        step(C)
        ref = {'s2s': bits(C.s2s), 'out': bits(C.out), 'al': bits(C.al), 'loss': bits(C.loss), 'grads': bits(C.grads)}
        del C
        assert np.isfinite(ref['grads'].view(np.float32)).all() and np.isfinite(ref['loss'].view(np.float32)).all()

        def compare(what):
            got = P.results(OUT_NAMES)
            same_bits(got, ref, OUT_NAMES if det else outs, '%s / %s' % (tag, what))
            if not det:
                close_grads(got, ref, '%s / %s' % (tag, what))

        # two clean runs in two separately carved allocations agree (the premise of every comparison below)
        load(P, c, p, inp, masks, 3)
        P.fill('zeros')
        step(P)
        compare('second clean arena')
        for pattern in c.get('patterns', ALL):
            P.fill(pattern)
            step(P)
            compare(pattern)
            P.check_coverage(OUT_NAMES, '%s / %s' % (tag, pattern))
        # foreign history: a complete other step on this workspace (over qnan, so that the table gaps stay checkable)
        P.fill('qnan')
        load(P, c, fp, finp, fmasks, 4)
        step(P)
        assert not np.array_equal(bits(P.s2s), ref['s2s']), 'the foreign step computed the same outputs: no history'
        load(P, c, p, inp, masks, 3)
        step(P)
        compare('foreign')
        P.check_coverage(OUT_NAMES, '%s / foreign' % tag)


def run_infer_case(lib, c, monkeypatch, label):
    for k, v in c.get('env', {}).items():
        monkeypatch.setenv(k, v)
    prev = lib.decoder_mode(c['decoder_mode']) if 'decoder_mode' in c else None
    try:
        _infer_case(lib, c, label)
    finally:
        if prev is not None:
            lib.decoder_mode(prev)


def _infer_case(lib, c, label):
    dims = (c['B'], c['Tt'], c['Td'], c['r'], c['V'])
    S = c.get('S', 1)
    keys = ('text', 'text_length', 'speaker')
    p, inp = c.get('p'), {k: v for k, v in c['inp'].items() if k in keys}
    fp, finp, _ = foreign_of(c)
    finp = {k: v for k, v in finp.items() if k in keys}
    B, Td = c['B'], c['Td']
    outs = ('s2s', 'out', 'al')
    C = Runner(lib, *dims, train=False, S=S)
    load(C, c, p, inp, None, 3)
    C.infer()
    ref = {'s2s': bits(C.s2s), 'out': bits(C.out), 'al': bits(C.al)}
    # a rule taken from this decode so that the lengths spread; at Td < 4 every row runs to Td
    rule = spread_rule(lib, C.al.cpu().numpy(), np.asarray(inp['text_length'])) if Td >= 4 else lib.TacoStopRule(0, 1, 1)
    ln = clean_infer_stop(lib, C, rule)
    ref_stop = {'s2s': bits(C.s2s), 'out': bits(C.out), 'al': bits(C.al), 'lengths': bits(ln)}
    lens = ln.cpu().numpy()
    print('  %s: %r lengths %s' % (label, rule, sorted(set(lens.tolist()))))
    del C
    P = PoisonRunner(lib, *dims, train=False, S=S)

    def both(what, fill):
        names = outs + ('lengths',)
        load(P, c, p, inp, None, 3)
        if fill is not None:
            P.fill(fill)
        P.infer()
        same_bits(P.results(outs), ref, outs, '%s infer / %s' % (label, what))
        if fill not in (None, 'zeros'):
            P.check_coverage(outs, '%s infer / %s' % (label, what))
            P.fill(fill)
        P.infer_stop(rule)
        same_bits(P.results(names), ref_stop, names, '%s infer_stop / %s' % (label, what))
        for name, x in (('s2s', P.s2s), ('out', P.out), ('al', P.al)):
            for b in range(B):
                assert not bool(x[b, int(lens[b]):].view(torch.int32).any()), '%s: %s row %d not 0 from len_b' % (what, name, b)
        if fill not in (None, 'zeros'):
            P.check_coverage(names, '%s infer_stop / %s' % (label, what))

    both('second clean arena', 'zeros')
    for pattern in c.get('patterns', ALL):
        both(pattern, pattern)
    # foreign history: infer + infer_stop with other parameters, text and lengths on this workspace, then the case
    P.fill('qnan')
    load(P, c, fp, finp, None, 4)
    P.infer()
    P.infer_stop(lib.TacoStopRule(0, 1, max(1, Td // 2)))
    both('foreign', None)
    P.check_coverage((), '%s / foreign' % label)


# ---- cases: each one a shape (and route) that another test of the suite holds to the fp64 oracle ---------------------------

def _gold(r, spk=False):
    g, p, inp, masks = golden(r, spk)
    c = dict(B=int(g['B']), Tt=int(g['Tt']), Td=int(g['Td']), r=r, V=int(g['V']), p=p, inp=inp, masks=masks)
    if spk:
        c['S'] = int(g['num_speakers'])
    return c


def _ragged():        # test_backward_without_masks_and_ragged_lengths
    r, V, B, Tt, Td = 2, 17, 3, 13, 7
    inp, _ = small_case(r=r, V=V, B=B, Tt=Tt, Td=Td, seed=21, full_len_row0=False)
    inp['text_length'][:] = [1, 13, 6]
    inp['text'][0, 1:] = 0
    inp['text'][2, 6:] = 0
    return dict(B=B, Tt=Tt, Td=Td, r=r, V=V, p=on.init_params(V, r, seed=9, perturb=0.3), inp=inp, masks=None)


def _shortest(Td):    # test_shortest_decodes
    r, V, B, Tt = 2, 19, 2, 9
    inp, masks = small_case(r=r, V=V, B=B, Tt=Tt, Td=Td, seed=33)
    return dict(B=B, Tt=Tt, Td=Td, r=r, V=V, p=on.init_params(V, r, seed=4, perturb=0.3), inp=inp, masks=masks)


def _r3():            # test_gpu_reduction.py::test_small_all_factors[3-23-7] (decoder.hip: decoder3 has no r = 3 form)
    r, V, B, Tt, Td = 3, 21, 2, 23, 7
    inp, masks = small_case(r=r, V=V, B=B, Tt=Tt, Td=Td, seed=60 + r)
    return dict(B=B, Tt=Tt, Td=Td, r=r, V=V, p=on.init_params(V, r, seed=50 + r, perturb=0.3), inp=inp, masks=masks, cluster=8)


def _geometry(B, mode, r):   # test_stages_decoder_geometries / test_r5_fallback_decoders
    V, Tt, Td = 33, 41, 9
    inp, masks = small_case(r=r, V=V, B=B, Tt=Tt, Td=Td, seed=40 + B)
    c = dict(B=B, Tt=Tt, Td=Td, r=r, V=V, p=on.init_params(V, r, seed=8, perturb=0.2), inp=inp, masks=masks,
             cluster=32 if mode in ('default', 'agent') else 8)
    if mode == 'agent':
        c['env'] = {'TACO_DEC_V3_AGENT': '1'}
    if mode == 'v3_off':
        c['env'] = {'TACO_DEC_V3': '0'}
    if mode == 'decoder_mode(2)':
        c['decoder_mode'] = 2
    return c


def _medium(env):     # test_medium_shape_forward_backward under test_medium_shape_with_gemm2_forced / _with_optional_paths
    r, V, B, Tt, Td = 2, 40, 4, 37, 12
    inp, masks = small_case(r=r, V=V, B=B, Tt=Tt, Td=Td, seed=8)
    return dict(B=B, Tt=Tt, Td=Td, r=r, V=V, p=on.init_params(V, r, seed=4, perturb=0.2), inp=inp, masks=masks, env=env)


def _pooled(B, Tt, Td):      # test_pooled_bank_epilogue_tile_edges
    r, V = 2, 40
    inp, masks = _full_case(B, Tt, Td, r, V)
    return dict(B=B, Tt=Tt, Td=Td, r=r, V=V, p=on.init_params(V, r, seed=11, perturb=0.3), inp=inp, masks=masks,
                env={'TACO_GEMM2_MIN_TILES': '1'})


def _infer_random(B, Tt, Td, r, V, seed):   # test_gpu_infer_stop.py CASES b1 / b48
    inp, _ = small_case(r=r, V=V, B=B, Tt=Tt, Td=Td, seed=seed)
    return dict(B=B, Tt=Tt, Td=Td, r=r, V=V, p=on.init_params(V, r, seed=seed, perturb=0.2), inp=inp, masks=None)


def _s1():            # test_full_size_properties / test_stages_s1 / test_gpu_infer_stop.py `full`
    B, Tt, Td, r, V = 32, 200, 180, 2, 60
    inp, masks = _full_case(B, Tt, Td, r, V)
    return dict(B=B, Tt=Tt, Td=Td, r=r, V=V, inp=inp, masks=masks, device_init=True, patterns=('qnan',), cluster=32)


TRAIN_CASES = {
    'golden-r2': lambda: _gold(2), 'golden-r5': lambda: _gold(5), 'golden-spk': lambda: _gold(2, True),
    'ragged-1-13-6-no-masks': _ragged, 'Td1': lambda: _shortest(1), 'Td2': lambda: _shortest(2), 'r3-decoder.hip': _r3,
    'B11': lambda: _geometry(11, 'default', 2), 'B40-r5': lambda: _geometry(40, 'default', 5),
    'B70-r5': lambda: _geometry(70, 'default', 5), 'B12-agent': lambda: _geometry(12, 'agent', 2),
    'B5-v3_off': lambda: _geometry(5, 'v3_off', 2), 'B11-r5-decoder_mode2': lambda: _geometry(11, 'decoder_mode(2)', 5),
    'medium-gemm2-32x2': lambda: _medium({'TACO_GEMM2_MIN_TILES': '1', 'TACO_GEMM2_VARIANT': '32x2'}),
    'medium-gemm2-16x3': lambda: _medium({'TACO_GEMM2_MIN_TILES': '1', 'TACO_GEMM2_VARIANT': '16x3'}),
    'medium-bsplit0': lambda: _medium({'TACO_GEMM2_BSPLIT': '0'}),
    'pooled-3-127-64': lambda: _pooled(3, 127, 64), 'pooled-2-128-9': lambda: _pooled(2, 128, 9),
    'S1': _s1,
}
INFER_CASES = {
    'golden-r2': lambda: _gold(2), 'golden-r5': lambda: _gold(5), 'golden-spk': lambda: _gold(2, True),
    'Td1': lambda: _shortest(1), 'Td2': lambda: _shortest(2), 'r3-decoder.hip': _r3,
    'B11': lambda: _geometry(11, 'default', 2), 'B70-r5': lambda: _geometry(70, 'default', 5),
    'B12-agent': lambda: _geometry(12, 'agent', 2), 'B5-v3_off': lambda: _geometry(5, 'v3_off', 2),
    'B11-r5-decoder_mode2': lambda: _geometry(11, 'decoder_mode(2)', 5),
    'b1': lambda: _infer_random(1, 30, 40, 2, 33, 12), 'b48': lambda: _infer_random(48, 41, 24, 2, 33, 13),
    'S1': _s1,
}


@pytest.mark.parametrize('case', list(TRAIN_CASES))
def test_train_step_on_poisoned_buffers(built_lib, case, monkeypatch):
    """taco_forward + taco_backward: (a), (b) and the foreign history of (c), default and deterministic gradient mode"""
    if case == 'S1':
        torch.set_num_threads(min(os.cpu_count() or 1, 16))
    c = TRAIN_CASES[case]()
    run_train_case(built_lib, c, monkeypatch, case)


@pytest.mark.parametrize('case', list(INFER_CASES))
def test_inference_on_poisoned_buffers(built_lib, case, monkeypatch):
    """taco_infer and taco_infer_stop (with its lengths, and exact zeros from len_b on in all three outputs)"""
    c = INFER_CASES[case]()
    c.pop('cluster', None)
    run_infer_case(built_lib, c, monkeypatch, case)


@pytest.mark.parametrize('order', ['large-then-small', 'small-then-large'])
@pytest.mark.parametrize('train', [True, False], ids=['train', 'infer'])
def test_one_workspace_two_layouts(built_lib, train, order, monkeypatch):
    """(c) across shapes: one workspace allocation, sized for the larger layout, serves B = 11, Tt = 41, r = 2 (decoder3) and
    B = 2, Tt = 23, r = 3 (decoder.hip) in turn -- the two layouts put different tensors over the same bytes, and the decoders'
    exchange areas at different offsets.  The second call must compute what it computes on a clean workspace; what lies behind
    the smaller layout stays as the larger call left it."""
    monkeypatch.setenv('TACO_DETERMINISTIC', '1')
    big, small = _geometry(11, 'default', 2), _r3()
    first, second = (big, small) if order == 'large-then-small' else (small, big)
    keys = ('text', 'text_length')
    stop = built_lib.TacoStopRule(0, 1, 4)

    def dims(c):
        return (c['B'], c['Tt'], c['Td'], c['r'], c['V'])

    def run(R, c):
        if train:
            R.set(c['p'], c['inp'], c['masks'])
            R.forward()
            R.backward()
        else:
            R.set(c['p'], {k: c['inp'][k] for k in keys})
            R.infer()
            if isinstance(R, PoisonRunner):
                R.infer_stop(stop)

    names = OUT_NAMES if train else ('s2s', 'out', 'al')
    C = Runner(built_lib, *dims(second), train=train)
    run(C, second)
    if not train:
        clean_infer_stop(built_lib, C, stop)
    ref = {n: bits(getattr(C, n)) for n in names}
    del C
    need = max(built_lib.workspace_bytes(built_lib.make_shape(*dims(c), 1), train) // 4 for c in (big, small))
    A = PoisonRunner(built_lib, *dims(first), train=train, ws_floats=need)
    Bq = PoisonRunner(built_lib, *dims(second), train=train, share=A)
    Bq.fill('qnan')
    A.fill('qnan')
    run(A, first)
    A.check_coverage(names, 'first layout')
    behind = bits(A.ws_full[Bq.ws.numel():]) if Bq.ws.numel() < A.ws_full.numel() else None
    Bq.clear_error()     # (dec.err sits at another offset in this layout: cleared as for any workspace new to a shape)
    run(Bq, second)
    same_bits(Bq.results(names), ref, names, '%s, %s' % ('train' if train else 'infer', order))
    Bq.marks.pop('ws', None)
    Bq.check_coverage(names, 'second layout')
    if behind is not None:
        assert np.array_equal(bits(A.ws_full[Bq.ws.numel():]), behind), 'the smaller layout wrote behind its workspace'


GROUPS = ['enc.', 'dec.', 'dec.xchg', 'post.', 'bwd.', 'gemm.', 'tapsplit+loss']


@pytest.mark.parametrize('group', GROUPS)
def test_localisation_by_workspace_family(built_lib, group, monkeypatch):
    """(d) at the smallest shape (the r = 2 golden fixture): poison in one family of workspace-table rows only (`dec.` is every
    decoder tensor but dec.err; dec.xchg also runs by itself), everything else zero as in the clean run."""
    monkeypatch.setenv('TACO_DETERMINISTIC', '1')
    c = _gold(2)
    dims = (c['B'], c['Tt'], c['Td'], c['r'], c['V'])
    for train in (True, False):
        C = Runner(built_lib, *dims, train=train)
        P = PoisonRunner(built_lib, *dims, train=train)
        if group == 'tapsplit+loss':
            only = poison.rows_with_prefix(P.table, 'tapsplit') + poison.rows_with_prefix(P.table, 'loss')
        else:
            only = poison.rows_with_prefix(P.table, group)
        if not only:
            assert group == 'bwd.' and not train      # (the inference workspace has no backward tensors)
            continue
        names = OUT_NAMES if train else ('s2s', 'out', 'al')
        inp = c['inp'] if train else {k: c['inp'][k] for k in ('text', 'text_length')}
        C.set(c['p'], inp, c['masks'] if train else None)
        P.set(c['p'], inp, c['masks'] if train else None)

        def run(R):
            if train:
                R.forward()
                R.backward()
            else:
                R.infer()

        run(C)
        ref = {n: bits(getattr(C, n)) for n in names}
        for pattern in ALL:
            P.fill(pattern, only=only)
            run(P)
            same_bits(P.results(names), ref, names, '%s in %s (%s)' % (pattern, group, 'train' if train else 'infer'))
            assert poison.guards_intact(P.arena)
