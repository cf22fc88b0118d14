"""GPU: weight averaging (taco_param_ema, ema.hip) against the NumPy float32 restatement tests/ema_ref.py.

Op level: the bits of the average at every size that takes another path (below, at and above one 16-byte group, one wave, one
workgroup, one batch of a thread; more than one workgroup; a tail of 1..3 floats), at w = 0, 1, float32(0.001) and float32(0.9);
every pointer alignment of both operands between guard bands; the guard on the two error words; the statistics within the bound of a
sum of n exact non-negative terms in any order, n 2^-52 relative, identical on a second call and with a poisoned workspace; a chain
of 20 updates under the warm-up.  Model level, under TACO_DETERMINISTIC=1 (the default mode's fp32 atomics would make two runs of the
SAME model differ): a model with averaging on takes exactly the steps of one without, its average follows the restatement over the
parameter snapshots, and the checkpoint carries it.

Inputs: parameters randn * 0.1, an average that differs from them by randn * 1e-3, some entries exactly zero, some p == e, and no
subnormal value anywhere in the update (the build's denormal mode is not this feature's to set): `case` asserts it."""
import numpy as np
import pytest
import torch

from tests import ema_ref as er
from tests.poison import Guarded

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 5, 255, 256, 257, 1023, 4099, (1 << 20) + 3]
WEIGHTS = [np.float32(0.001), np.float32(0.9), np.float32(0.0), np.float32(1.0)]
TINY = np.float32(1.1754944e-38)   # the smallest normal float32


def bits(x):
    a = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def case(n, seed):
    """(e, p) float32 arrays of n values; no update of them at any weight of this file meets a subnormal"""
    rng = np.random.default_rng(seed)
    p = (rng.standard_normal(n) * 0.1).astype(np.float32)
    e = (p + rng.standard_normal(n).astype(np.float32) * np.float32(1e-3)).astype(np.float32)
    e[3::7] = p[3::7]      # p == e
    p[1::5] = 0.0          # exact zeros on either side, and on both (index 31, 66, ...)
    e[2::11] = 0.0
    d = (p - e).astype(np.float32)
    for w in WEIGHTS + [np.float32(0.1)]:
        t = (np.float32(w) * d).astype(np.float32)
        for v in (d, t, e, p, (e + t).astype(np.float32)):
            assert not ((v != 0) & (np.abs(v) < TINY)).any(), 'a subnormal value in the test inputs'
    return e, p


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_cases = {}


def shared(n, seed=None):
    """the inputs of size n, built once; never modified"""
    key = (n, n if seed is None else seed)
    if key not in _cases:
        _cases[key] = case(n, key[1])
    return _cases[key]


# ---- 1: bit identity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('w', WEIGHTS, ids=lambda w: 'w%g' % w)
@pytest.mark.parametrize('n', SIZES)
def test_bits_of_the_average(built_lib, n, w):
    e, p = shared(n)
    want = er.ema_update(e, p, w)
    ema, params = dev(e), dev(p)
    built_lib.param_ema(ema, params, w)
    got = bits(ema)
    bad = np.flatnonzero(got != bits(want))
    assert not len(bad), (n, float(w), bad[:5], e[bad[:5]], p[bad[:5]], ema.cpu().numpy()[bad[:5]], want[bad[:5]])
    assert np.array_equal(bits(params), bits(p))          # params are read only
    if w == 0:
        assert np.array_equal(got, bits(e))


# ---- 2: pointer alignment, between guard bands ---------------------------------------------------------------------------------
@pytest.mark.parametrize('b', range(4))
@pytest.mark.parametrize('a', range(4))
def test_every_alignment_of_both_pointers(built_lib, a, b):
    n, w = 4099, np.float32(0.001)
    e, p = shared(n)
    want = bits(er.ema_update(e, p, w))
    need = built_lib.param_ema_workspace_bytes(n)
    G = Guarded({'ema': ((a + n,), torch.float32, 'qnan'), 'params': ((b + n,), torch.float32, 'qnan'),
                 'stats': ((3,), torch.float64, 'qnan'), 'work': ((need,), torch.uint8, 'qnan')})
    ema, params = G['ema'][a:], G['params'][b:]
    assert ema.data_ptr() % 16 == 4 * a and params.data_ptr() % 16 == 4 * b and ema.numel() == n == params.numel()
    ema.copy_(dev(e))
    params.copy_(dev(p))
    built_lib.param_ema(ema, params, w, None, G['stats'], G['work'])
    torch.cuda.synchronize()
    assert np.array_equal(bits(ema), want)                # the bits of the aligned call (test 1), whatever the path
    assert np.array_equal(bits(params), bits(p))
    G.check('stats')                                      # the bands in front of and behind ema, params, stats and the workspace
    head = torch.zeros(a + n, dtype=torch.bool, device='cuda')
    head[:a] = True
    assert G.margin_intact('ema', head)                   # the floats between the 16-byte boundary and ema
    d2, p2 = er.ema_stats(e, p)
    st = G['stats'].cpu().numpy()
    assert st[2] == 1.0 and abs(st[0] - d2) <= n * 2.0 ** -52 * d2 and abs(st[1] - p2) <= n * 2.0 ** -52 * p2


# ---- 3: the guard --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [5, 4099])
@pytest.mark.parametrize('words', [None, (0, 0), (1, 0), (0, 1), (2, 7)])
def test_the_guard(built_lib, words, n):
    w = np.float32(0.9)
    e, p = shared(n)
    err = None if words is None else torch.tensor(words, dtype=torch.int32, device='cuda')   # the test's own two words
    for off in (0, 1):                                     # the 16-byte path and the float path
        ema, params = dev(np.concatenate([np.zeros(off, np.float32), e]))[off:], dev(p)
        stats = torch.full((3,), 7.0, dtype=torch.float64, device='cuda')
        built_lib.param_ema(ema, params, w, err, stats)
        if words is None or words == (0, 0):
            assert np.array_equal(bits(ema), bits(er.ema_update(e, p, w))) and stats[2].item() == 1.0
        else:
            assert np.array_equal(bits(ema), bits(e))
            assert stats.tolist() == [-1.0, -1.0, 0.0]
        ema2 = dev(e)
        built_lib.param_ema(ema2, params, w, err)          # without stats: the same decision
        assert np.array_equal(bits(ema2), bits(ema))
    if err is not None:
        assert err.tolist() == list(words)                 # the words are read only


# ---- 4: the statistics ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('off', [0, 3])
@pytest.mark.parametrize('n', [1, 5, 257, 4099, (1 << 20) + 3])
def test_stats(built_lib, n, off):
    w = np.float32(0.001)
    e, p = shared(n)
    d2, p2 = er.ema_stats(e, p)
    need = built_lib.param_ema_workspace_bytes(n)
    runs = []
    for fill in ('qnan', 'ones', 'qnan'):
        G = Guarded({'stats': ((3,), torch.float64, fill), 'work': ((need,), torch.uint8, fill)})
        ema, params = dev(np.concatenate([np.zeros(off, np.float32), e]))[off:], dev(p)
        built_lib.param_ema(ema, params, w, None, G['stats'], G['work'])
        torch.cuda.synchronize()
        G.check('stats')
        runs.append((bits(G['stats']).copy(), bits(ema).copy()))
    st = runs[0][0].view(np.float64)
    print('  n %d off %d: d2 %.17g (ref %.17g, rel %.2e)  p2 %.17g (ref %.17g, rel %.2e)  bound %.2e'
          % (n, off, st[0], d2, abs(st[0] - d2) / d2 if d2 else 0.0, st[1], p2, abs(st[1] - p2) / p2 if p2 else 0.0, n * 2.0 ** -52))
    assert st[2] == 1.0
    assert abs(st[0] - d2) <= n * 2.0 ** -52 * d2 and abs(st[1] - p2) <= n * 2.0 ** -52 * p2
    for other in runs[1:]:                                 # the same bits again, whatever the workspace and stats held
        assert np.array_equal(other[0], runs[0][0]) and np.array_equal(other[1], runs[0][1])
    plain = dev(np.concatenate([np.zeros(off, np.float32), e]))[off:]
    built_lib.param_ema(plain, dev(p), w)                  # stats=None: the same average
    assert np.array_equal(bits(plain), runs[0][1]) and np.array_equal(runs[0][1], bits(er.ema_update(e, p, w)))


def test_c_abi_refusals_enqueue_nothing(built_lib):
    import ctypes as C
    raw = built_lib._lib
    e, p = shared(257)
    ema, params = dev(e), dev(p)
    stats = torch.zeros(3, dtype=torch.float64, device='cuda')
    work = torch.empty(built_lib.param_ema_workspace_bytes(257), dtype=torch.uint8, device='cuda')
    P = lambda t, o=0: C.c_void_p(t.data_ptr() + o)
    s = built_lib.stream_ptr()
    bad = [((None, P(params), 257, 0.5, None, None, None, s), 'NULL'),
           ((P(ema), None, 257, 0.5, None, None, None, s), 'NULL'),
           ((P(ema), P(params), 0, 0.5, None, None, None, s), 'n=0'),
           ((P(ema), P(params), -3, 0.5, None, None, None, s), 'n=-3'),
           ((P(ema), P(params), 257, -0.1, None, None, None, s), 'w='),
           ((P(ema), P(params), 257, 1.5, None, None, None, s), 'w='),
           ((P(ema), P(params), 257, float('nan'), None, None, None, s), 'w='),
           ((P(ema), P(params), 257, float('inf'), None, None, None, s), 'w='),
           ((P(ema), P(ema, 4 * 100), 157, 0.5, None, None, None, s), 'overlap'),
           ((P(ema), P(ema), 257, 0.5, None, None, None, s), 'overlap'),
           ((P(ema), P(params), 257, 0.5, None, P(stats), None, s), 'workspace')]
    for args, said in bad:
        assert raw.taco_param_ema(*args) == -1 and said in built_lib.last_error(), (said, built_lib.last_error())
    torch.cuda.synchronize()
    assert np.array_equal(bits(ema), bits(e)) and stats.tolist() == [0.0, 0.0, 0.0]
    assert raw.taco_param_ema(P(ema), P(params), 257, 0.5, None, P(stats), P(work), s) == 0


# ---- 5: a chain under the warm-up ----------------------------------------------------------------------------------------------
def test_a_chain_of_twenty_updates(built_lib):
    n, decay = 4099, 0.999
    e, _ = shared(n)
    ema, want = dev(e), e.copy()
    for k in range(20):
        _, p = shared(n, 1000 + k)                         # fresh parameters each time
        w = built_lib.ema_weight(decay, k)
        assert w == er.ema_weight(decay, k)
        built_lib.param_ema(ema, dev(p), w)
        want = er.ema_update(want, p, w)
        assert not ((want != 0) & (np.abs(want) < TINY)).any()
        assert np.array_equal(bits(ema), bits(want)), k


# ---- 6: the model --------------------------------------------------------------------------------------------------------------
def test_model_with_and_without_averaging(built_lib, monkeypatch):
    from tacotron_amd.config import Config
    from tacotron_amd.data import synthetic_batch
    from tacotron_amd.model import Tacotron
    monkeypatch.setenv('TACO_DETERMINISTIC', '1')          # fixed summation orders: two runs of one model give the same bits
    lib = built_lib
    batch = synthetic_batch(4, 24, 10, 2, 30, seed=5, min_len=10)
    plain_c, avg_c = Config(), Config()
    for c in (plain_c, avg_c):
        c.r, c.vocab_size = 2, 30
    avg_c.ema_decay = 0.999
    plain = Tacotron(plain_c, batch, train=True, seed=1)
    avg = Tacotron(avg_c, batch, train=True, seed=1)
    for name in ('ema', 'ema_updates', 'ema_decay', 'ema_stats'):
        assert hasattr(avg, name) and not hasattr(plain, name), name
    assert avg.ema_updates == 0 and avg.ema.data_ptr() != avg.params.flat.data_ptr()
    assert np.array_equal(bits(avg.ema), bits(avg.params.flat)) and np.array_equal(bits(avg.params.flat), bits(plain.params.flat))
    masks = plain.draw_masks()                             # drawn once, the same tensors for both models and all steps
    want = avg.params.flat.cpu().numpy().copy()
    for k in range(3):
        plain.step(lr=1e-3, masks=masks)
        avg.step(lr=1e-3, masks=masks, ema_stats=(k == 2))
        for name in ('adam_m', 'adam_v'):
            assert np.array_equal(bits(getattr(avg, name)), bits(getattr(plain, name))), (k, name)
        assert np.array_equal(bits(avg.params.flat), bits(plain.params.flat)), k
        assert np.array_equal(bits(avg._loss), bits(plain._loss)), k
        snap = avg.params.flat.cpu().numpy()
        before = want
        want = er.ema_update(want, snap, er.ema_weight(0.999, k))
        assert np.array_equal(bits(avg.ema), bits(want)), k
    plain.check()
    avg.check()
    assert avg.ema_updates == 3 and avg.global_step == 3 == plain.global_step
    d2, p2 = er.ema_stats(before, snap)                    # the last step asked for the statistics
    st = avg.ema_stats.tolist()
    n = snap.size
    assert st[2] == 1.0 and abs(st[0] - d2) <= n * 2.0 ** -52 * d2 and abs(st[1] - p2) <= n * 2.0 ** -52 * p2
    # the checkpoint
    sd, sd_plain = avg.state_dict(), plain.state_dict()
    assert set(sd) - set(sd_plain) == {'ema', 'ema_updates', 'ema_decay'} and set(sd_plain) <= set(sd)
    assert sd['ema_updates'] == 3 and sd['ema_decay'] == 0.999 and np.array_equal(bits(sd['ema']), bits(want))
    assert np.array_equal(bits(sd['params']), bits(sd_plain['params']))
    infer_c = Config()
    infer_c.r, infer_c.vocab_size, infer_c.max_decode_iter = 2, 30, 10
    text = {'text': batch['text'], 'text_length': batch['text_length']}
    mi = Tacotron(infer_c, text, train=False)
    mi.load_state_dict(sd, use_ema=True)
    assert np.array_equal(bits(mi.params.flat), bits(want)) and not hasattr(mi, 'ema')
    mi.load_state_dict(sd)
    assert np.array_equal(bits(mi.params.flat), bits(snap))
    with pytest.raises(lib.TacoError, match='adam_m.*params'):   # (the message names the file's keys)
        mi.load_state_dict(sd_plain, use_ema=True)
    # a training model with averaging on continues the checkpoint's average; from a plain checkpoint it starts again
    again = Tacotron(avg_c, batch, train=True, seed=2)
    again.load_state_dict(sd)
    assert again.ema_updates == 3 and np.array_equal(bits(again.ema), bits(want)) and np.array_equal(bits(again.params.flat), bits(snap))
    again.load_state_dict(sd_plain)
    assert again.ema_updates == 0 and np.array_equal(bits(again.ema), bits(snap))
