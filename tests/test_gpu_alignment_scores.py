"""taco_alignment_scores on the GPU (include/taco_hip.h): per-utterance attention scores against the NumPy restatement
(tests/align_ref.py).  Every op-level call goes through lib.alignment_scores with all five buffers carved from one guarded arena
(tests/poison.py): the outputs start as poison and must be written completely, the guard bands and the inputs must come back as they
were.  counts are compared exactly, means with the float64 restatement to (Tt + Td) 2^-23 absolute; where the restatement's mean is NaN
the device's must be, and only there."""
import os

import numpy as np
import pytest
import torch

from tests import align_ref as ar
from tests.poison import Guarded
from tests.util import small_case

pytestmark = pytest.mark.gpu


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def run(lib, al, tl, steps=None, max_jump=ar.MAX_JUMP, shift=0):
    """one guarded call -> (counts, means) as host arrays.  shift: floats by which alignments starts behind a 256-byte boundary"""
    al = np.ascontiguousarray(al, dtype=np.float32)
    B, Td, Tt = al.shape
    specs = {'al': ((al.size + shift,), torch.float32, 'zeros'), 'tl': ((B,), torch.int32, 'zeros'),
             'counts': ((B, 6), torch.int32, 'ones'), 'means': ((B, 2), torch.float32, 'ones')}
    if steps is not None:
        specs['steps'] = ((B,), torch.int32, 'zeros')
    G = Guarded(specs)
    a = G['al'][shift:].view(B, Td, Tt)
    assert a.data_ptr() % 16 == (4 * shift) % 16
    a.copy_(torch.from_numpy(al))
    G['tl'].copy_(torch.as_tensor(np.asarray(tl, dtype=np.int32)))
    if steps is not None:
        G['steps'].copy_(torch.as_tensor(np.asarray(steps, dtype=np.int32)))
    counts, means = lib.alignment_scores(a, G['tl'], G['steps'] if steps is not None else None, max_jump, G['counts'], G['means'])
    torch.cuda.synchronize()
    assert counts is G['counts'] and means is G['means']
    G.check('counts', 'means')
    assert np.array_equal(bits(a.cpu().numpy()), bits(al)), 'alignments were written'
    assert np.array_equal(G['tl'].cpu().numpy(), np.asarray(tl, dtype=np.int32))
    if steps is not None:
        assert np.array_equal(G['steps'].cpu().numpy(), np.asarray(steps, dtype=np.int32))
    return counts.cpu().numpy(), means.cpu().numpy()


def compare(got, want, Td, Tt, label=''):
    (c, m), (rc, rm) = got, want
    assert c.dtype == np.int32 and m.dtype == np.float32
    assert np.array_equal(c, rc), '%s counts\n%s\nrestatement\n%s' % (label, c, rc)
    assert np.array_equal(np.isnan(m), np.isnan(rm)), '%s NaN means\n%s\nrestatement\n%s' % (label, m, rm)
    ok = ~np.isnan(rm)
    err = float(np.abs(m.astype(np.float64) - rm)[ok].max()) if ok.any() else 0.0
    print('  %-34s max |mean - fp64| %.2e (bound %.2e)' % (label, err, ar.means_bound(Td, Tt)))
    assert err <= ar.means_bound(Td, Tt), label


def check(lib, al, tl, steps=None, max_jump=ar.MAX_JUMP, shift=0, label=''):
    got = run(lib, al, tl, steps, max_jump, shift)
    compare(got, ar.scores(al, tl, steps, max_jump), al.shape[1], al.shape[2], label)
    return got


def peaks(path, Tt, base=0.02, peak=0.8):
    """(len(path), Tt): `base` everywhere, `peak` at path[t]; an entry of path that is a tuple puts the peak at each of its indices"""
    a = np.full((len(path), Tt), base, dtype=np.float32)
    for t, s in enumerate(path):
        a[t, list(s) if isinstance(s, tuple) else s] = peak
    return a


# ---- the core case -------------------------------------------------------------------------------------------------------------------
def test_core_case(built_lib):
    B, Td, Tt, J = 4, 12, 7, 2
    tl, steps = [7, 4, 1, 9], [12, 8, 0, 5]
    al = np.stack([
        # maximum at s = 0; a tie of 1 and 3 (1 wins); +2 = max_jump (no skip); back; +3 (skip); maximum at s = Tt - 1
        peaks([0, 0, 1, (1, 3), 3, 2, 5, 6, 6, 6, 6, 6], Tt),
        # L = 4: 4, 5 and 6 lie on padding; back 5 -> 3; skip 3 -> 6; the steps from 8 on are not scored
        peaks([0, 1, 2, 3, 4, 5, 3, 6, 0, 6, 0, 6], Tt),
        # no step is scored
        peaks([3, 0, 6, 1, 5, 2, 4, 0, 6, 3, 1, 5], Tt),
        # L = 9 clamps to 7: nothing is padding
        peaks([6, 6, 0, 3, 3, 0, 6, 0, 6, 0, 6, 0], Tt),
    ])
    assert al.shape == (B, Td, Tt)
    counts, means = check(built_lib, al, tl, steps, J, label='core')
    #                           n  end pad back skip covered
    assert counts.tolist() == [[12, 6, 0, 1, 1, 6],
                               [8, 6, 3, 1, 1, 4],
                               [0, 0, 0, 0, 0, 0],
                               [5, 6, 0, 1, 1, 3]]
    assert means[2].tolist() == [0.0, 0.0]
    assert abs(means[0, 0] - 0.8) < 1e-6 and means[0, 1] == 0.0 and means[3, 1] == 0.0
    assert abs(means[1, 1] - (3 * (0.8 + 2 * 0.02) + 5 * 3 * 0.02) / 8) < 1e-6


# ---- tile edges ------------------------------------------------------------------------------------------------------------------------
def edge_rows(Tt, vec, rng):
    """Td = 4 steps over Tt characters: the maximum in the last element; a tie of the first and the last element; a tie of two
    neighbours; a tie of two elements that one lane meets in two iterations of its loop (64 items apart: items are elements on the
    4-byte path, groups of four on the 16-byte path), the later one listed first"""
    a = (rng.random((4, Tt)) * 0.5).astype(np.float32)
    a[0, Tt - 1] = 0.9
    a[1, [0, Tt - 1]] = 0.9
    a[2, [Tt // 2, min(Tt // 2 + 1, Tt - 1)]] = 0.9
    stride = 256 if vec else 64
    lo = 21 if Tt > 21 + stride else 0
    hi = lo + stride + (1 if vec else 0) if lo + stride + 1 < Tt else Tt - 1
    a[3, [hi, lo]] = 0.9
    return a, [Tt - 1, 0, Tt // 2, lo]


@pytest.mark.parametrize('Tt', [1, 63, 64, 65, 200, 257, 300])
def test_tile_edges_of_the_text_axis(built_lib, Tt):
    rng = np.random.default_rng(Tt)
    for shift in (0, 1):                                  # (shift 1: one float off a 16-byte boundary -- the 4-byte path for every Tt)
        vec = Tt % 4 == 0 and shift == 0
        rows = [edge_rows(Tt, vec, rng) for _ in range(2)]
        al = np.stack([r[0] for r in rows])
        tl = [Tt, max(1, Tt // 2)]
        counts, _ = check(built_lib, al, tl, None, 2, shift, label='Tt=%d shift=%d' % (Tt, shift))
        assert counts[0, 1] == Tt - 1 and counts[0, 0] == 4
        want = rows[0][1]
        # the argmax path of row 0 is known: read it back through `end` and `covered` on prefixes of the steps
        for n in range(1, 5):
            c, _ = run(built_lib, al, tl, [n, n], Tt, shift)
            assert c[0].tolist()[:2] == [n, max(want[:n])] and c[0, 5] == len(set(want[:n])), (Tt, shift, n, c[0], want)


@pytest.mark.parametrize('Td', [1, 2, 181])
@pytest.mark.parametrize('B', [1, 33])
def test_step_and_batch_counts(built_lib, Td, B):
    rng = np.random.default_rng(100 * Td + B)
    Tt = 12
    al = rng.random((B, Td, Tt)).astype(np.float32)
    al /= al.sum(-1, keepdims=True)
    tl = rng.integers(1, Tt + 1, size=B)
    check(built_lib, al, tl, None, 3, label='Td=%d B=%d' % (Td, B))
    if Td == 181:   # a record longer than one pass of the workgroup's 16 waves, steps on both sides of every row's end
        steps = rng.integers(0, Td + 1, size=B)
        steps[0] = 180
        check(built_lib, al, tl, steps, 0, label='Td=%d B=%d steps' % (Td, B))


def test_steps_and_max_jump_ranges(built_lib):
    rng = np.random.default_rng(8)
    B, Td, Tt = 5, 9, 20
    al = rng.random((B, Td, Tt)).astype(np.float32)
    tl = [20, 1, 7, 0, 33]                                # (0 and 33 clamp to 1 and Tt)
    base = check(built_lib, al, tl, None, 3, label='steps NULL')
    assert (base[0][:, 0] == Td).all()
    got = check(built_lib, al, tl, [-3, Td + 5, 0, Td, 4], 3, label='steps clamp')
    assert got[0][:, 0].tolist() == [0, Td, 0, Td, 4]
    assert np.array_equal(got[0][1], base[0][1]) and np.array_equal(bits(got[1][1]), bits(base[1][1]))
    j0 = check(built_lib, al, tl, None, 0, label='max_jump 0')
    jt = check(built_lib, al, tl, None, Tt, label='max_jump Tt')
    assert (jt[0][:, 4] == 0).all() and (j0[0][:, 4] > 0).all()
    assert np.array_equal(j0[0][:, [0, 1, 2, 3, 5]], jt[0][:, [0, 1, 2, 3, 5]])
    big = check(built_lib, al, tl, None, (1 << 31) - 1, label='max_jump 2^31 - 1')
    assert np.array_equal(big[0], jt[0])


def test_one_float_off_a_16_byte_boundary(built_lib):
    """Tt = 200 rows are 16-byte aligned only when the base is: the same data at shift 0 and 1 gives the same counts"""
    rng = np.random.default_rng(21)
    al = rng.random((3, 17, 200)).astype(np.float32)
    tl = [200, 90, 140]
    a = check(built_lib, al, tl, None, 3, 0, label='aligned')
    b = check(built_lib, al, tl, None, 3, 1, label='one float off')
    c = check(built_lib, al, tl, None, 3, 3, label='three floats off')
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[0], c[0])


# ---- NaN ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('Tt', [7, 200])
def test_nan(built_lib, Tt):
    rng = np.random.default_rng(31 + Tt)
    B, Td = 4, 6
    al = rng.random((B, Td, Tt)).astype(np.float32)
    al /= al.sum(-1, keepdims=True)
    tl = [Tt, Tt - 2, Tt - 2, Tt - 2]
    al[0, 2, int(al[0, 2].argmax())] = np.nan      # row 0: one NaN, where the maximum was: the counts move, both means stay finite
    al[1, 3, :] = np.nan                           # row 1: a step that is all NaN
    al[2, 1, Tt - 1] = np.nan                      # row 2: a NaN at s >= L only: focus stays finite, pad_mass does not
    want = ar.scores(al, tl, None, 3)              # row 3: clean
    assert np.isnan(want[1]).tolist() == [[False, False], [True, True], [False, True], [False, False]]
    got = run(built_lib, al, tl, None, 3)
    compare(got, want, Td, Tt, 'NaN Tt=%d' % Tt)
    got = run(built_lib, al, tl, None, 3, shift=1)
    compare(got, want, Td, Tt, 'NaN Tt=%d, 4-byte path' % Tt)


# ---- the training shape --------------------------------------------------------------------------------------------------------------------
def s1_alignments(seed=0):
    """B = 32, Td = 180, Tt = 200: the fp32 softmax of seeded logits with a peak that walks the row's text, with some noise"""
    rng = np.random.default_rng(seed)
    B, Td, Tt = 32, 180, 200
    tl = rng.integers(60, Tt + 1, size=B).astype(np.int32)
    logits = rng.standard_normal((B, Td, Tt)).astype(np.float32)
    t = np.arange(Td)
    for b in range(B):
        path = np.clip(t * int(tl[b]) // 150 + rng.integers(-2, 3, size=Td), 0, Tt - 1)
        logits[b, t, path] += np.float32(6.0)
    e = np.exp(logits - logits.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True, dtype=np.float32)).astype(np.float32), tl


@pytest.fixture(scope='module')
def s1():
    al, tl = s1_alignments()
    return al, tl, ar.scores(al, tl, None, ar.MAX_JUMP)


def test_s1_shape(built_lib, s1):
    al, tl, want = s1
    got = run(built_lib, al, tl)
    compare(got, want, 180, 200, 'S1')
    assert got[0][:, 2].max() > 0 and got[0][:, 3].max() > 0 and got[0][:, 4].max() > 0 and (got[0][:, 5] > 40).all()


def test_two_calls_give_the_same_bits(built_lib, s1):
    al, tl, _ = s1
    a = run(built_lib, al, tl)
    b = run(built_lib, al, tl)
    assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))


def test_graph_capture(built_lib, s1):
    """one captured call replays to the eager results, bit for bit"""
    al, tl, want = s1
    a = torch.from_numpy(al).cuda()
    t = torch.from_numpy(tl).cuda()
    steps = torch.full((32,), 100, dtype=torch.int32, device='cuda')
    counts = torch.empty(32, 6, dtype=torch.int32, device='cuda')
    means = torch.empty(32, 2, device='cuda')
    built_lib.alignment_scores(a, t, steps, 3, counts, means)
    torch.cuda.synchronize()
    ref = (counts.clone(), means.clone())
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        built_lib.alignment_scores(a, t, steps, 3, counts, means)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            built_lib.alignment_scores(a, t, steps, 3, counts, means)
    torch.cuda.synchronize()
    counts.fill_(-1)
    means.fill_(float('nan'))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(counts, ref[0]) and torch.equal(means, ref[1])
    compare((counts.cpu().numpy(), means.cpu().numpy()), ar.scores(al, tl, [100] * 32, 3), 180, 200, 'replay')
    steps.fill_(180)   # a replay follows what `steps` holds at replay time
    g.replay()
    torch.cuda.synchronize()
    compare((counts.cpu().numpy(), means.cpu().numpy()), want, 180, 200, 'replay, other steps')


def test_bad_arguments_enqueue_nothing(built_lib):
    a = torch.rand(2, 3, 8, device='cuda')
    tl = torch.full((2,), 8, dtype=torch.int32, device='cuda')
    counts = torch.full((2, 6), -1, dtype=torch.int32, device='cuda')
    means = torch.full((2, 2), float('nan'), device='cuda')
    fn, P = built_lib._lib.taco_alignment_scores, built_lib.ptr
    for args in ((None, P(tl), None, 3, P(counts), P(means), 2, 3, 8), (P(a), None, None, 3, P(counts), P(means), 2, 3, 8),
                 (P(a), P(tl), None, 3, None, P(means), 2, 3, 8), (P(a), P(tl), None, 3, P(counts), None, 2, 3, 8),
                 (P(a), P(tl), None, -1, P(counts), P(means), 2, 3, 8), (P(a), P(tl), None, 3, P(counts), P(means), 0, 3, 8),
                 (P(a), P(tl), None, 3, P(counts), P(means), 2, 0, 8), (P(a), P(tl), None, 3, P(counts), P(means), 2, 3, 0),
                 (P(a), P(tl), None, 3, P(counts), P(means), 2, built_lib.ALIGN_MAX_TD + 1, 8),
                 (P(a), P(tl), None, 3, P(counts), P(means), 2, 3, built_lib.ALIGN_MAX_TT + 1)):
        assert fn(*args, built_lib.stream_ptr()) == -1
        assert built_lib.last_error().startswith('alignment_scores:')
    torch.cuda.synchronize()
    assert (counts == -1).all() and torch.isnan(means).all()


# ---- model level ---------------------------------------------------------------------------------------------------------------------------
def _config_and_batch(B=3, Tt=9, Td=8):
    from tacotron_amd.config import Config
    c = Config()
    c.r, c.vocab_size, c.max_decode_iter = 2, 20, Td
    inp, _ = small_case(r=2, V=20, B=B, Tt=Tt, Td=Td, seed=3)
    return c, {k: torch.as_tensor(v) for k, v in inp.items()}, inp['text_length']


def test_model_after_inference_with_and_without_stop(built_lib):
    from tacotron_amd.model import Tacotron
    c, batch, tl = _config_and_batch()
    m = Tacotron(c, {'text': batch['text'], 'text_length': batch['text_length']}, train=False, seed=5)
    m.run(stop=built_lib.TacoStopRule(end_offset=100, hold=1, min_steps=3))   # target 0: every row stops after step 2 -> len 4
    counts, means = m.alignment_scores()
    torch.cuda.synchronize()
    ln = m.lengths.cpu().numpy()
    assert ln.tolist() == [4, 4, 4]
    al = m.alignments.cpu().numpy()
    compare((counts.cpu().numpy(), means.cpu().numpy()), ar.scores(al, tl, ln, built_lib.MAX_JUMP), 8, 9, 'model, stop')
    assert counts[:, 0].tolist() == [4, 4, 4]
    m.run()
    again = m.alignment_scores(max_jump=1)
    torch.cuda.synchronize()
    assert again[0] is counts and again[1] is means and m.lengths is None            # the same two tensors, allocated once
    compare((counts.cpu().numpy(), means.cpu().numpy()), ar.scores(m.alignments.cpu().numpy(), tl, None, 1), 8, 9, 'model, no stop')
    assert counts[:, 0].tolist() == [8, 8, 8]
    m.check()


def test_model_after_a_training_step(built_lib):
    from tacotron_amd.model import Tacotron
    c, batch, tl = _config_and_batch()
    m = Tacotron(c, batch, train=True, seed=0)
    m.step(1e-3)
    counts, means = m.alignment_scores()
    torch.cuda.synchronize()
    compare((counts.cpu().numpy(), means.cpu().numpy()), ar.scores(m.alignments.cpu().numpy(), tl, None, built_lib.MAX_JUMP), 8, 9,
            'model, train step')
    assert counts[:, 0].tolist() == [8, 8, 8]
    m.check()


# ---- the driver ------------------------------------------------------------------------------------------------------------------------------
def test_cli_align_scores(built_lib, tmp_path, capsys):
    """tacotron_amd.test.test(stop=..., align_scores=True): prompt_NNN_ascore.npy is the restatement of the saved alignment and
    length, the picture has len_b zoom rows; without the option the files are today's"""
    from tacotron_amd import test as drv
    from tacotron_amd.alignment import flags
    from tacotron_amd.config import Config
    prompts = ['hello world.\n', 'short\n']

    def cfg():
        c = Config()
        c.data_path = str(tmp_path / 'no_data') + '/'
        c.max_decode_iter = 16
        return c

    rule = built_lib.TacoStopRule(end_offset=200, hold=1, min_steps=5)   # target 0: len_b = 8 for every prompt
    plain, scored = tmp_path / 'plain', tmp_path / 'scored'
    assert drv.test(cfg(), prompts, out_dir=str(plain), vocode=False, stop=rule) == 2
    capsys.readouterr()
    assert drv.test(cfg(), prompts, out_dir=str(scored), vocode=False, stop=rule, align_scores=True) == 2
    out = capsys.readouterr().out
    today = sorted('prompt_%03d_%s.npy' % (i, k) for i in range(2) for k in ('spec', 'align', 'len'))
    assert sorted(os.listdir(plain)) == today
    assert sorted(os.listdir(scored)) == sorted(today + ['prompt_%03d_%s' % (i, k) for i in range(2) for k in ('ascore.npy', 'align.png')])
    for i, text in enumerate(prompts):
        for k in ('spec', 'align', 'len'):
            name = 'prompt_%03d_%s.npy' % (i, k)
            assert open(plain / name, 'rb').read() == open(scored / name, 'rb').read()
        al = np.load(scored / ('prompt_%03d_align.npy' % i))
        ln = int(np.load(scored / ('prompt_%03d_len.npy' % i)))
        score = np.load(scored / ('prompt_%03d_ascore.npy' % i))
        L = len(text)                                                   # (the newline is the end-of-text character)
        assert ln == 8 and al.shape == (8, 140) and score.dtype == np.float64 and score.shape == (8,)
        rc, rm = ar.scores(al[None], [L], [ln], built_lib.MAX_JUMP)
        assert score[:6].tolist() == rc[0].tolist()
        assert np.abs(score[6:] - rm[0]).max() <= ar.means_bound(8, 140)
        px = ar.read_png(str(scored / ('prompt_%03d_align.png' % i)))
        assert px.shape == (ln * 4, 140 * 4, 3) and np.array_equal(px, ar.pixels(al, ln, 4))
        found = flags(score[:6], score[6:], L, end_offset=rule.end_offset)
        line = 'WARNING prompt %d: %s' % (i, ', '.join(found))
        assert (line in out) == bool(found) and out.count('WARNING prompt %d:' % i) == (1 if found else 0)
