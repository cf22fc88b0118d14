"""taco_alignment_path on the GPU (include/taco_hip.h): the best monotone path through an attention matrix against the NumPy
restatement (tests/align_path_ref.py).  Every op-level call goes through lib.alignment_path with all buffers, the workspace included,
carved from one guarded arena (tests/poison.py): the outputs and the workspace start as poison, the outputs must be written
completely, the guard bands and the inputs must come back as they were.  The comparison is exact -- path, dur and counts equal, mass
equal in its bits: every cell is one rounded fp32 addition, so there is no tolerance to choose."""
import numpy as np
import pytest
import torch

from tests import align_path_ref as pr
from tests.poison import Guarded

pytestmark = pytest.mark.gpu


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def run(lib, al, tl, steps=None, max_jump=4, shift=0):
    """one guarded call -> (path, dur, counts, mass) as host arrays.  shift: floats by which alignments starts behind a 256-byte
    boundary"""
    al = np.ascontiguousarray(al, dtype=np.float32)
    B, Td, Tt = al.shape
    specs = {'al': ((al.size + shift,), torch.float32, 'zeros'), 'tl': ((B,), torch.int32, 'zeros'),
             'path': ((B, Td), torch.int32, 'qnan'), 'dur': ((B, Tt), torch.int32, 'qnan'), 'counts': ((B, 3), torch.int32, 'qnan'),
             'mass': ((B,), torch.float32, 'ones')}
    if steps is not None:
        specs['steps'] = ((B,), torch.int32, 'zeros')
    ws_bytes = lib.alignment_path_workspace_bytes(B, Td, Tt)
    if ws_bytes:
        specs['ws'] = ((ws_bytes,), torch.uint8, 'ones')
    G = Guarded(specs)
    a = G['al'][shift:].view(B, Td, Tt)
    assert a.data_ptr() % 16 == (4 * shift) % 16
    a.copy_(torch.from_numpy(al))
    G['tl'].copy_(torch.as_tensor(np.asarray(tl, dtype=np.int32)))
    if steps is not None:
        G['steps'].copy_(torch.as_tensor(np.asarray(steps, dtype=np.int32)))
    out = lib.alignment_path(a, G['tl'], G['steps'] if steps is not None else None, max_jump, G['path'], G['dur'], G['counts'], G['mass'],
                             G['ws'] if ws_bytes else None)
    torch.cuda.synchronize()
    assert all(o is G[k] for o, k in zip(out, ('path', 'dur', 'counts', 'mass')))
    G.check('path', 'dur', 'counts', 'mass')
    assert np.array_equal(bits(a.cpu().numpy()), bits(al)), 'alignments were written'
    assert np.array_equal(G['tl'].cpu().numpy(), np.asarray(tl, dtype=np.int32))
    if steps is not None:
        assert np.array_equal(G['steps'].cpu().numpy(), np.asarray(steps, dtype=np.int32))
    return tuple(o.cpu().numpy() for o in out)


def same(got, want, label=''):
    for name, g, w in zip(('path', 'dur', 'counts'), got, want):
        assert g.dtype == np.int32 and np.array_equal(g, w), '%s %s\n%s\nrestatement\n%s' % (label, name, g, w)
    assert got[3].dtype == np.float32 and np.array_equal(bits(got[3]), bits(want[3])), '%s mass %s restatement %s' % (label, got[3], want[3])


def check(lib, al, tl, steps=None, max_jump=4, shifts=(0,), label=''):
    want = pr.best_paths(al, tl, steps, max_jump)
    for shift in shifts:
        got = run(lib, al, tl, steps, max_jump, shift)
        same(got, want, '%s shift=%d' % (label, shift))
    return want


def softmax_rows(rng, B, Td, Tt, tl):
    """the fp32 softmax of seeded logits with a peak that wanders along each row's text"""
    logits = rng.standard_normal((B, Td, Tt)).astype(np.float32)
    t = np.arange(Td)
    for b in range(B):
        L = min(max(int(tl[b]), 1), Tt)
        walk = np.clip(t * L // max(Td - 1, 1) + rng.integers(-2, 3, size=Td), 0, Tt - 1)
        logits[b, t, walk] += np.float32(6.0)
    e = np.exp(logits - logits.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True, dtype=np.float32)).astype(np.float32)


def dyadic_rows(rng, B, Td, Tt, levels=3):
    """multiples of 1/8 from a few levels only: every sum is exact, and ties in the predecessor choice and the final argmax are real"""
    return (rng.integers(0, levels, size=(B, Td, Tt)) / 8.0).astype(np.float32)


# ---- the shapes at which each part can go wrong ------------------------------------------------------------------------------------
# Tt: lane boundaries (3, 4, 5), wave-row and wave boundaries (63 .. 65, 255, 256), the change of form (256 -> 257, 260: the general
# form with and without the 16-byte row), the limit.  (Td, J) pairs walk Td in {1, 2, 5, 13} and J in {1, 2, 4, 15}, and every
# instantiation of the single-wave form: candidates in 1, 2, 3 or 4 lanes below (J <= 4, 8, 12, 15), J a multiple of 4 or not.
PAIRS = [(1, 1), (2, 2), (5, 4), (13, 15), (13, 1), (5, 15), (5, 6), (13, 8), (5, 11), (13, 12)]


@pytest.mark.parametrize('Tt', [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 260])
def test_text_axis(built_lib, Tt):
    rng = np.random.default_rng(1000 + Tt)
    for Td, J in PAIRS:
        tl = [Tt, max(1, Tt // 2), 1]
        label = 'Tt=%d Td=%d J=%d' % (Tt, Td, J)
        check(built_lib, softmax_rows(rng, 3, Td, Tt, tl), tl, None, J, (0, 1), label + ' softmax')   # (shift 1: the 4-byte loads)
        check(built_lib, dyadic_rows(rng, 3, Td, Tt), tl, None, J, (0,), label + ' dyadic')


def test_text_axis_at_the_limit(built_lib):
    """Tt = 4096 with enough steps for the path to reach the last characters (J (Td - 1) >= Tt - 1): sixteen waves, four cells a lane"""
    Tt, Td, J = built_lib.PATH_MAX_TT, 300, 15
    rng = np.random.default_rng(4096)
    tl = [Tt, 2500]
    al = softmax_rows(rng, 2, Td, Tt, tl)
    want = pr.best_paths(al, tl, [Td, 200], J, one=pr.best_path_fast)
    assert want[2][0, 1] > 3500 and want[2][1, 1] > 1500
    for shift in (0, 1):
        same(run(built_lib, al, tl, [Td, 200], J, shift), want, 'Tt=%d shift=%d' % (Tt, shift))
    assert built_lib.alignment_path_workspace_bytes(2, Td, Tt) == 2 * Td * Tt


def test_training_shape_rows(built_lib):
    """Td = 180 over Tt = 200: the product's shape, the single-wave form with its direction table in LDS"""
    rng = np.random.default_rng(180)
    tl = [200, 117]
    assert built_lib.alignment_path_workspace_bytes(32, 180, 200) == 0
    al = softmax_rows(rng, 2, 180, 200, tl)
    want = check(built_lib, al, tl, [180, 150], 4, (0, 1), 'S1 rows')
    assert want[2][0, 1] > 150 and want[2][1, 1] > 80 and (want[1].sum(-1) == [180, 150]).all()


def test_long_decode_takes_the_general_form(built_lib):
    """Tt <= 256 with a direction table beyond the LDS budget: the general form, chosen by Td"""
    Td, Tt = 520, 256
    assert built_lib.alignment_path_workspace_bytes(1, 500, Tt) == 0 and built_lib.alignment_path_workspace_bytes(2, Td, Tt) == 2 * Td * Tt
    rng = np.random.default_rng(520)
    tl = [30, 12]
    al = softmax_rows(rng, 2, Td, Tt, tl)
    want = check(built_lib, al, tl, [Td, 300], 2, (0,), 'Td=520')
    assert (want[2][:, 1] > 3).all() and (want[1].sum(-1) == [Td, 300]).all()


# ---- steps, text_length ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('Tt', [20, 300])
def test_steps_and_text_length_ranges(built_lib, Tt):
    rng = np.random.default_rng(8 + Tt)
    B, Td = 4, 9
    tl = [Tt, 0, 7, Tt + 33]                              # (0 and Tt + 33 clamp to 1 and Tt)
    al = softmax_rows(rng, B, Td, Tt, tl)
    base = check(built_lib, al, tl, None, 3, label='steps NULL')
    assert (base[2][:, 0] == Td).all() and (base[0] >= 0).all() and (base[1][1, 1:] == 0).all() and base[1][1, 0] == Td
    got = check(built_lib, al, tl, [0, Td + 5, -3, 4], 3, label='steps clamp')
    assert got[2][:, 0].tolist() == [0, Td, 0, 4]
    for b in (0, 2):                                      # the empty row
        assert (got[0][b] == -1).all() and (got[1][b] == 0).all() and got[2][b].tolist() == [0, 0, 0] and bits(got[3][b]) == 0
    assert (got[0][3, 4:] == -1).all() and (got[0][3, :4] >= 0).all() and got[1][3].sum() == 4


def test_fewer_steps_than_characters(built_lib):
    """n < L with J = 1: a diagonal that the path follows as far as its steps reach, e = n - 1"""
    Td, Tt = 6, 12
    al = np.full((1, Td, Tt), 0.01, np.float32)
    al[0, np.arange(Td), np.arange(Td)] = 0.9
    want = check(built_lib, al, [Tt], None, 1, label='n < L')
    assert want[0][0].tolist() == list(range(Td)) and want[2][0].tolist() == [Td, Td - 1, 0]
    want = check(built_lib, al, [Tt], [4], 1, label='n < L, steps')
    assert want[2][0].tolist() == [4, 3, 0] and want[1][0].tolist() == [1] * 4 + [0] * 8


# ---- ties --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('Tt', [6, 300])
def test_ties(built_lib, Tt):
    Td = 5
    flat = np.full((1, Td, Tt), 0.25, np.float32)         # all equal: d = 0 wins every tie, the path stays on character 0
    want = check(built_lib, flat, [Tt], None, 2, label='all equal')
    assert want[0][0].tolist() == [0] * Td and want[1][0, 0] == Td and want[2][0].tolist() == [Td, 0, 0]
    a = np.zeros((1, Td, Tt), np.float32)                 # two ends of equal mass: the lower one is the end
    a[0, :, 0] = 0.5
    a[0, 1:, 2] = 0.625                                   # 0.5 + 4 * 0.625 = 3.0 via character 2 from step 1 on
    a[0, 1:, 1] = 0.625                                   # and the same via character 1
    want = check(built_lib, a, [Tt], None, 2, label='two ends')
    assert want[2][0, 1] == 1 and float(want[3][0]) == 3.0 and want[0][0].tolist() == [0, 1, 1, 1, 1]
    a = np.zeros((1, 3, Tt), np.float32)                  # a skipped character: 0 -> 2 pays, 1 does not
    a[0, 0, 0] = a[0, 1, 2] = a[0, 2, 2] = 0.5
    want = check(built_lib, a, [Tt], None, 2, label='skip')
    assert want[0][0].tolist() == [0, 2, 2] and want[2][0].tolist() == [3, 2, 1] and want[1][0, :3].tolist() == [1, 0, 2]
    rng = np.random.default_rng(77 + Tt)                  # and ties at random
    for J in (1, 2, 4, 15):
        check(built_lib, dyadic_rows(rng, 4, 13, Tt, levels=2), [Tt, Tt // 2, 3, 1], None, J, label='dyadic J=%d' % J)


# ---- values that are no weights ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('Tt', [7, 200, 300])
def test_nan_negative_zero_and_infinity(built_lib, Tt):
    rng = np.random.default_rng(31 + Tt)
    B, Td = 4, 6
    tl = [Tt, Tt - 2, Tt - 2, Tt]
    al = softmax_rows(rng, B, Td, Tt, tl)
    al[0, 2, int(al[0, 2].argmax())] = np.nan             # a NaN where the path wanted to go
    al[0, 4, :] = np.nan                                  # a step that is all NaN
    al[1, 1, :3] = [-1.0, -0.0, -np.inf]                  # negative values and -0 weigh +0
    al[1, 0, 0] = -0.0
    al[2, 3, 2] = np.inf                                  # +inf stays +inf along the path
    want = check(built_lib, al, tl, None, 3, (0, 1), 'no weights')
    assert np.isfinite(want[3][[0, 1, 3]]).all() and np.isposinf(want[3][2])
    zero = np.full((1, Td, Tt), -0.0, np.float32)
    want = check(built_lib, zero, [Tt], None, 3, label='all -0')
    assert bits(want[3])[0] == 0                          # (+0, not -0)


# ---- independence ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('Tt', [24, 264])
def test_rows_are_independent(built_lib, Tt):
    rng = np.random.default_rng(5 + Tt)
    B, Td = 4, 13
    tl, steps = [Tt - 4, 9, Tt, 17], [9, 13, 5, 11]
    al = softmax_rows(rng, B, Td, Tt, tl)
    base = run(built_lib, al, tl, steps, 4)
    same(base, pr.best_paths(al, tl, steps, 4), 'base')
    dirty = al.copy()
    for b in range(B):
        L, n = pr.row_args(Td, Tt, tl[b], steps[b])
        dirty[b, n:, :] = np.nan                          # steps >= n
        dirty[b, :, L:] = np.nan                          # characters >= L
    same(run(built_lib, dirty, tl, steps, 4), base, 'NaN behind n and L')
    other = al.copy()
    other[[0, 2, 3]] = np.nan                             # every other row
    got = run(built_lib, other, tl, steps, 4)
    same(tuple(g[1:2] for g in got), tuple(g[1:2] for g in base), 'NaN in the other rows')
    for b in range(B):                                    # a row of a B = 4 call is its own B = 1 call
        one = run(built_lib, al[b:b + 1], tl[b:b + 1], steps[b:b + 1], 4)
        same(one, tuple(g[b:b + 1] for g in base), 'row %d alone' % b)


@pytest.mark.parametrize('Tt', [200, 300])
def test_two_calls_give_the_same_bits(built_lib, Tt):
    rng = np.random.default_rng(2 + Tt)
    tl = [Tt, 150, 33]
    al = softmax_rows(rng, 3, 40, Tt, tl)
    a = run(built_lib, al, tl, None, 4)
    b = run(built_lib, al, tl, None, 4)
    same(a, b, 'again')


def test_graph_capture(built_lib):
    """one captured call replays to the eager results, bit for bit, and follows what `steps` holds at replay time"""
    rng = np.random.default_rng(9)
    B, Td, Tt = 3, 40, 200
    tl = np.array([200, 150, 33], np.int32)
    al = softmax_rows(rng, B, Td, Tt, tl)
    a, t = torch.from_numpy(al).cuda(), torch.from_numpy(tl).cuda()
    steps = torch.full((B,), 25, dtype=torch.int32, device='cuda')
    out = built_lib.alignment_path(a, t, steps, 4)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            built_lib.alignment_path(a, t, steps, 4, *out)
    torch.cuda.synchronize()
    for o in out:
        o.view(torch.int32).fill_(-7)
    g.replay()
    torch.cuda.synchronize()
    same(tuple(o.cpu().numpy() for o in out), pr.best_paths(al, tl, [25] * B, 4), 'replay')
    steps.fill_(Td)
    g.replay()
    torch.cuda.synchronize()
    same(tuple(o.cpu().numpy() for o in out), pr.best_paths(al, tl, None, 4), 'replay, other steps')


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_enqueue_nothing(built_lib):
    lib = built_lib
    B, Td, Tt = 2, 3, 300                                 # (the general form: this shape needs a workspace)
    a = torch.rand(B, Td, Tt, device='cuda')
    tl = torch.full((B,), Tt, dtype=torch.int32, device='cuda')
    path = torch.full((B, Td), -9, dtype=torch.int32, device='cuda')
    dur = torch.full((B, Tt), -9, dtype=torch.int32, device='cuda')
    counts = torch.full((B, 3), -9, dtype=torch.int32, device='cuda')
    mass = torch.full((B,), float('nan'), device='cuda')
    ws = torch.full((lib.alignment_path_workspace_bytes(B, Td, Tt),), 255, dtype=torch.uint8, device='cuda')
    assert ws.numel() == B * Td * Tt
    fn, P = lib._lib.taco_alignment_path, lib.ptr
    good = [P(a), P(tl), None, 4, P(path), P(dur), P(counts), P(mass), P(ws), B, Td, Tt]

    def bad(**kw):
        names = ('alignments', 'text_length', 'steps', 'max_jump', 'path', 'dur', 'counts', 'mass', 'workspace', 'B', 'Td', 'Tt')
        return [kw.get(n, v) for n, v in zip(names, good)]

    cases = [({k: None}, k) for k in ('alignments', 'text_length', 'path', 'dur', 'counts', 'mass', 'workspace')]
    cases += [({'B': 0}, 'B'), ({'Td': 0}, 'Td'), ({'Tt': 0}, 'Tt'), ({'B': -1}, 'B'), ({'Td': lib.PATH_MAX_TD + 1}, 'Td'),
              ({'Tt': lib.PATH_MAX_TT + 1}, 'Tt'), ({'max_jump': 0}, 'max_jump'), ({'max_jump': lib.PATH_MAX_JUMP + 1}, 'max_jump'),
              ({'max_jump': -1}, 'max_jump')]
    for kw, word in cases:
        assert fn(*bad(**kw), lib.stream_ptr()) == -1, kw
        msg = lib.last_error()
        assert msg.startswith('alignment_path:') and word in msg, (kw, msg)
    size = lib._lib.taco_alignment_path_workspace_bytes
    for shape in ((0, 3, 8), (2, 0, 8), (2, 3, 0), (-1, 3, 8), (2, lib.PATH_MAX_TD + 1, 8), (2, 3, lib.PATH_MAX_TT + 1)):
        assert size(*shape) == -1, shape
    assert size(2, lib.PATH_MAX_TD, lib.PATH_MAX_TT) == 2 * lib.PATH_MAX_TD * lib.PATH_MAX_TT
    torch.cuda.synchronize()
    assert (path == -9).all() and (dur == -9).all() and (counts == -9).all() and torch.isnan(mass).all() and (ws == 255).all()
    assert fn(*good, lib.stream_ptr()) == 0               # and the same arguments, all in place, are taken
    torch.cuda.synchronize()
    same((path.cpu().numpy(), dur.cpu().numpy(), counts.cpu().numpy(), mass.cpu().numpy()),
         pr.best_paths(a.cpu().numpy(), tl.cpu().numpy(), None, 4), 'good')


# ---- model level -------------------------------------------------------------------------------------------------------------------
def test_model_after_inference_with_and_without_stop(built_lib):
    from tacotron_amd.config import Config
    from tacotron_amd.model import Tacotron
    from tests.util import small_case
    c = Config()
    c.r, c.vocab_size, c.max_decode_iter = 2, 20, 8
    inp, _ = small_case(r=2, V=20, B=3, Tt=9, Td=8, seed=3)
    tl = inp['text_length']
    m = Tacotron(c, {'text': torch.as_tensor(inp['text']), 'text_length': torch.as_tensor(tl)}, train=False, seed=5)
    m.run(stop=built_lib.TacoStopRule(end_offset=100, hold=1, min_steps=3))   # target 0: every row stops after step 2 -> len 4
    out = m.alignment_path()
    torch.cuda.synchronize()
    ln = m.lengths.cpu().numpy()
    assert ln.tolist() == [4, 4, 4]
    same(tuple(o.cpu().numpy() for o in out), pr.best_paths(m.alignments.cpu().numpy(), tl, ln, built_lib.PATH_JUMP), 'model, stop')
    m.run()
    again = m.alignment_path(max_jump=1)
    torch.cuda.synchronize()
    assert all(x is y for x, y in zip(again, out)) and m.lengths is None            # the same four tensors, allocated once
    same(tuple(o.cpu().numpy() for o in again), pr.best_paths(m.alignments.cpu().numpy(), tl, None, 1), 'model, no stop')
    assert again[2][:, 0].tolist() == [8, 8, 8]
    m.check()
