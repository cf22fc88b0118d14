"""taco_frames_active / taco_frame_dtw on the GPU (include/taco_hip.h) against the NumPy restatement (tests/dtw_ref.py), and what is
built on them: Tacotron.mel_distortion and tacotron_amd.evaluate.  Every op-level call goes through lib.frame_dtw / lib.frames_active
with all of its buffers carved from one guarded arena (tests/poison.py): the outputs (and the workspace) start as poison, the guard
bands and the inputs must come back as they were.  The device's cost BITS and steps are compared with the float32 restatement
exactly -- no tolerance; the float64 recurrence bounds the result itself to twice dtw_ref.dtw_bound."""
import os
import pickle

import numpy as np
import pytest
import torch

from tests import dtw_ref as dr
from tests.poison import Guarded

pytestmark = pytest.mark.gpu

THREADS = 256   # kDtwThreads of dtw.hip: cells of one anti-diagonal a workgroup takes per pass


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def run(lib, a, b, na=None, nb=None, basis=None, shift=(0, 0)):
    """one guarded call -> (cost, steps) as host arrays.  shift: floats by which a / b start behind a 256-byte boundary"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    B, Fa, C = a.shape
    Fb = b.shape[1]
    K = C if basis is None else basis.shape[0]
    specs = {'a': ((a.size + shift[0],), torch.float32, 'zeros'), 'b': ((b.size + shift[1],), torch.float32, 'zeros'),
             'cost': ((B,), torch.float32, 'ones'), 'steps': ((B,), torch.int32, 'ones')}
    ints = {'na': na, 'nb': nb}
    for k, v in ints.items():
        if v is not None:
            specs[k] = ((B,), torch.int32, 'zeros')
    if basis is not None:
        specs['basis'] = (basis.shape, torch.float32, 'zeros')
    nbytes = lib.frame_dtw_workspace_bytes(B, Fa, Fb, K)
    if nbytes:
        specs['work'] = ((nbytes,), torch.uint8, 'qnan')
    G = Guarded(specs)
    ta = G['a'][shift[0]:].view(B, Fa, C)
    tb = G['b'][shift[1]:].view(B, Fb, C)
    assert ta.data_ptr() % 256 == 4 * shift[0] and tb.data_ptr() % 256 == 4 * shift[1]
    ta.copy_(torch.from_numpy(a))
    tb.copy_(torch.from_numpy(b))
    for k, v in ints.items():
        if v is not None:
            G[k].copy_(torch.as_tensor(np.asarray(v, dtype=np.int32)))
    if basis is not None:
        G['basis'].copy_(torch.from_numpy(basis))
    cost, steps = lib.frame_dtw(ta, tb, G['na'] if na is not None else None, G['nb'] if nb is not None else None,
                                G['basis'] if basis is not None else None, G['cost'], G['steps'], G['work'] if nbytes else None)
    torch.cuda.synchronize()
    assert cost is G['cost'] and steps is G['steps']
    G.check('cost', 'steps')
    assert np.array_equal(bits(ta.cpu().numpy()), bits(a)) and np.array_equal(bits(tb.cpu().numpy()), bits(b)), 'frames were written'
    for k, v in ints.items():
        if v is not None:
            assert np.array_equal(G[k].cpu().numpy(), np.asarray(v, dtype=np.int32))
    if basis is not None:
        assert np.array_equal(bits(G['basis'].cpu().numpy()), bits(basis))
    return cost.cpu().numpy(), steps.cpu().numpy()


def same(got, want, label=''):
    (c, n), (rc, rn) = got, want
    assert c.dtype == np.float32 and n.dtype == np.int32
    assert np.array_equal(n, rn), '%s steps\n%s\nrestatement\n%s' % (label, n, rn)
    assert np.array_equal(bits(c), bits(rc)), '%s cost\n%s\nrestatement\n%s' % (label, c, rc)


def within_fp64(cost, case, label):
    c64, _ = case['ref64']
    B = len(cost)
    na = np.clip(np.asarray(case['na'] if case['na'] is not None else [case['a'].shape[1]] * B), 0, case['a'].shape[1])
    nb = np.clip(np.asarray(case['nb'] if case['nb'] is not None else [case['b'].shape[1]] * B), 0, case['b'].shape[1])
    K = case['a'].shape[2] if case['basis'] is None else case['basis'].shape[0]
    for r in range(B):
        bound = 2 * dr.dtw_bound(max(int(na[r]) + int(nb[r]) - 1, 0), K) * c64[r]
        err = abs(float(cost[r]) - c64[r])
        print('  %-10s row %d  cost %.6f  |cost - fp64| %.3e  (allowed %.3e)' % (label, r, cost[r], err, bound))
        assert err <= bound, (label, r)


def case(a, b, na, nb, basis):
    return {'a': a, 'b': b, 'na': na, 'nb': nb, 'basis': basis, 'ref32': dr.dtw32(a, b, na, nb, basis), 'ref64': dr.dtw64(a, b, na, nb, basis)}


# ---- the references, computed once -------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def core():
    rng = np.random.default_rng(0)
    a = rng.standard_normal((6, 12, 5)).astype(np.float32)
    b = rng.standard_normal((6, 9, 5)).astype(np.float32)
    return case(a, b, [1, 1, 7, 12, 0, 4], [1, 7, 1, 9, 5, 0], None)


def mel_like(rng, B, F, C=80):
    """smooth log-mel-like frames: a random walk over the frames around -5"""
    return (np.cumsum(rng.standard_normal((B, F, C)) * 0.3, axis=1) - 5.0).astype(np.float32)


@pytest.fixture(scope='module')
def product(built_lib):
    rng = np.random.default_rng(5)
    return case(mel_like(rng, 4, 360), mel_like(rng, 4, 360), [360, 301, 77, 258], [333, 360, 150, 257], built_lib.dct_basis())


@pytest.fixture(scope='module')
def envelope(built_lib):
    rng = np.random.default_rng(6)
    F, C, K = built_lib.DTW_MAX_FRAMES, 24, 32
    basis = (rng.standard_normal((K, C)) / np.sqrt(C)).astype(np.float32)
    return case(mel_like(rng, 1, F, C), mel_like(rng, 1, F, C), None, None, basis)


# ---- 1, 2, 3: core case, ties, poison ----------------------------------------------------------------------------------------------------
def test_core_case(built_lib, core):
    got = run(built_lib, core['a'], core['b'], core['na'], core['nb'])
    same(got, core['ref32'], 'core')
    assert got[1].tolist()[:3] == [1, 7, 7] and got[1].tolist()[4:] == [0, 0] and got[0].tolist()[4:] == [0.0, 0.0]
    assert 12 <= got[1][3] <= 20
    within_fp64(got[0], core, 'core')


def test_lengths_null_and_clamped(built_lib, core):
    a, b = core['a'], core['b']
    full = run(built_lib, a, b)
    same(full, dr.dtw32(a, b), 'NULL lengths')
    clamped = run(built_lib, a, b, [99, 12, 13, 1 << 30, 12, 12], [9, 9, 100, 9, 9, 10])
    same(clamped, full, 'lengths above Fa / Fb')
    neg = run(built_lib, a, b, [-1, 3, 3, 3, 3, -(1 << 31)], [3, -7, 3, 3, 3, 3])
    same(neg, dr.dtw32(a, b, [-1, 3, 3, 3, 3, -(1 << 31)], [3, -7, 3, 3, 3, 3]), 'negative lengths')
    assert neg[1].tolist()[:2] == [0, 0] and neg[1][5] == 0


def test_ties(built_lib):
    rng = np.random.default_rng(2)
    a = rng.integers(0, 2, (5, 40, 3)).astype(np.float32)
    b = rng.integers(0, 2, (5, 33, 3)).astype(np.float32)
    a[0], b[0] = 0.0, 0.0                                   # every cell ties
    b[1, :33] = a[1, :33]
    got = run(built_lib, a, b, [40, 33, 40, 2, 3], [33, 33, 30, 3, 2])
    same(got, dr.dtw32(a, b, [40, 33, 40, 2, 3], [33, 33, 30, 3, 2]), 'ties')
    assert got[0][0] == 0.0 and got[1][0] == 40             # all zeros: the diagonal first, then down the last column
    assert got[0][1] == 0.0 and got[1][1] == 33             # a sequence against itself
    zeros = np.zeros((2, 3, 1), dtype=np.float32)
    got = run(built_lib, zeros, zeros, [2, 3], [3, 2])      # the two orders tests/test_frame_dtw_host.py works by hand
    assert got[1].tolist() == [3, 3]
    x = rng.standard_normal((1, 21, 4)).astype(np.float32)
    got = run(built_lib, x, np.repeat(x, 2, axis=1))
    assert got[0].tolist() == [0.0] and got[1].tolist() == [42]


def test_poison_past_the_lengths_and_in_other_rows(built_lib):
    rng = np.random.default_rng(3)
    B, Fa, Fb, C = 4, 70, 50, 6
    a = rng.standard_normal((B, Fa, C)).astype(np.float32)
    b = rng.standard_normal((B, Fb, C)).astype(np.float32)
    na, nb = [70, 31, 5, 66], [50, 44, 50, 1]
    basis = rng.standard_normal((4, C)).astype(np.float32)
    clean = run(built_lib, a, b, na, nb, basis)
    same(clean, dr.dtw32(a, b, na, nb, basis), 'clean')
    pa, pb = a.copy(), b.copy()
    for r in range(B):
        pa[r, na[r]:] = np.nan
        pb[r, nb[r]:] = np.nan
    pa[2], pb[2] = np.nan, np.inf                            # a whole row: its own result is unspecified, the others' are not
    got = run(built_lib, pa, pb, na, nb, basis)
    keep = [0, 1, 3]
    same((got[0][keep], got[1][keep]), (clean[0][keep], clean[1][keep]), 'poisoned')


# ---- 4: long diagonals ---------------------------------------------------------------------------------------------------------------------
def test_long_diagonals_and_thin_tables(built_lib):
    rng = np.random.default_rng(4)
    F = 700
    a = rng.standard_normal((7, F, 3)).astype(np.float32)
    b = rng.standard_normal((7, F, 3)).astype(np.float32)
    na = [THREADS + 1, 65, 3, 700, THREADS, 64, 2 * THREADS + 1]
    nb = [THREADS + 1, 65, 700, 3, THREADS + 44, 64, 2 * THREADS + 1]
    got = run(built_lib, a, b, na, nb)
    same(got, dr.dtw32(a, b, na, nb), 'long diagonals')


# ---- 5, 6, 7: product shape, envelope, fp64 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shift', [1, 2, 3])
def test_product_shape(built_lib, product, shift):
    p = product
    assert built_lib.frame_dtw_workspace_bytes(4, 360, 360, 13) == 0      # the coefficients live in LDS
    got = run(built_lib, p['a'], p['b'], p['na'], p['nb'], p['basis'], shift=(shift, shift))
    same(got, p['ref32'], 'product shape, %d floats off' % shift)
    if shift == 1:
        within_fp64(got[0], p, 'product')


def test_envelope_with_the_workspace(built_lib, envelope):
    e = envelope
    F = built_lib.DTW_MAX_FRAMES
    assert built_lib.frame_dtw_workspace_bytes(1, F, F, 32) > 0              # K = 32 at this length does not fit LDS
    got = run(built_lib, e['a'], e['b'], None, None, e['basis'])
    same(got, e['ref32'], 'envelope')
    assert F <= got[1][0] <= 2 * F - 1
    within_fp64(got[0], e, 'envelope')


def test_two_calls_give_the_same_bits(built_lib, product):
    p = product
    x = run(built_lib, p['a'], p['b'], p['na'], p['nb'], p['basis'])
    y = run(built_lib, p['a'], p['b'], p['na'], p['nb'], p['basis'])
    assert np.array_equal(bits(x[0]), bits(y[0])) and np.array_equal(x[1], y[1])


# ---- 8: frames_active -------------------------------------------------------------------------------------------------------------------------
def active(lib, x, floor):
    x = np.ascontiguousarray(x, dtype=np.float32)
    G = Guarded({'x': (x.shape, torch.float32, 'zeros'), 'n': ((x.shape[0],), torch.int32, 'ones')})
    G['x'].copy_(torch.from_numpy(x))
    n = lib.frames_active(G['x'], floor, G['n'])
    torch.cuda.synchronize()
    assert n is G['n']
    G.check('n')
    assert np.array_equal(bits(G['x'].cpu().numpy()), bits(x))
    return n.cpu().numpy()


def test_frames_active(built_lib):
    floor = float(np.float16(np.log(1e-8)))
    F, C = 37, 80                                            # (2960 elements a row: more than one pass of the workgroup, no multiple of it)
    x = np.full((7, F, C), floor, dtype=np.float32)          # row 0: none above the floor -- a value equal to it does not count
    x[1, F - 1, C - 1] = floor + 1.0                         # only the last frame, in its last element
    x[2, 0, 0] = 0.0                                         # only frame 0
    x[3, 5:] = np.nan                                        # NaN frames do not count
    x[3, 4, 40] = -3.0
    x[4] = np.nan                                            # nothing but NaN
    x[5, :20] = -4.0                                         # a recording of 20 frames
    x[5, 20:] = np.nextafter(np.float32(floor), np.float32(-np.inf))
    x[6, 11, 3] = np.nextafter(np.float32(floor), np.float32(0))   # one ulp above the floor
    got = active(built_lib, x, floor)
    assert got.dtype == np.int32 and got.tolist() == [0, F, 1, 5, 0, 20, 12]
    assert np.array_equal(got, dr.frames_active(x, floor))
    rng = np.random.default_rng(8)
    y = rng.standard_normal((33, 9, 5)).astype(np.float32)
    assert np.array_equal(active(built_lib, y, 1.5), dr.frames_active(y, 1.5))
    assert np.array_equal(active(built_lib, y[:1, :1, :1], -9.0), [1])


# ---- 9: bad arguments -----------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_enqueue_nothing(built_lib):
    lib, P = built_lib, built_lib.ptr
    a = torch.rand(2, 6, 4, device='cuda')
    b = torch.rand(2, 5, 4, device='cuda')
    basis = torch.rand(3, 4, device='cuda')
    cost = torch.full((2,), float('nan'), device='cuda')
    steps = torch.full((2,), -1, dtype=torch.int32, device='cuda')
    n = torch.full((2,), -1, dtype=torch.int32, device='cuda')
    fn = lib._lib.taco_frame_dtw
    good = dict(a=P(a), na=None, b=P(b), nb=None, basis=P(basis), cost=P(cost), steps=P(steps), work=None, B=2, Fa=6, Fb=5, C=4, K=3)
    assert fn(*good.values(), lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert not torch.isnan(cost).any() and (steps > 0).all()
    cost.fill_(float('nan'))
    steps.fill_(-1)
    M = lib.DTW_MAX_FRAMES
    bad = [dict(a=None), dict(b=None), dict(cost=None), dict(steps=None), dict(B=0), dict(B=-2), dict(Fa=0), dict(Fb=0), dict(Fb=-1),
           dict(C=0), dict(K=0), dict(K=-3), dict(basis=None), dict(basis=None, K=5), dict(K=lib.DTW_MAX_K + 1),
           dict(basis=None, C=lib.DTW_MAX_K + 1, K=lib.DTW_MAX_K + 1), dict(C=lib.DTW_MAX_C + 1), dict(Fa=M + 1), dict(Fb=M + 1),
           dict(Fa=M, Fb=M, K=lib.DTW_MAX_K)]               # (the last: a shape that needs a workspace, and none is given)
    for change in bad:
        args = dict(good, **change)
        assert fn(*args.values(), lib.stream_ptr()) == -1, change
        assert lib.last_error().startswith('frame_dtw:'), (change, lib.last_error())
    x = torch.rand(2, 3, 4, device='cuda')
    for args in ((None, 0.0, P(n), 2, 3, 4), (P(x), 0.0, None, 2, 3, 4), (P(x), 0.0, P(n), 0, 3, 4), (P(x), 0.0, P(n), 2, 0, 4),
                 (P(x), 0.0, P(n), 2, 3, -1)):
        assert lib._lib.taco_frames_active(*args, lib.stream_ptr()) == -1
        assert lib.last_error().startswith('frames_active:')
    torch.cuda.synchronize()
    assert torch.isnan(cost).all() and (steps == -1).all() and (n == -1).all()


# ---- 10: graph capture ----------------------------------------------------------------------------------------------------------------------
def test_graph_capture(built_lib, product):
    """one captured frames_active + frame_dtw pair replays to the eager bits, and follows what the buffers hold at replay time"""
    lib, p = built_lib, product
    a, b = torch.from_numpy(p['a']).cuda(), torch.from_numpy(p['b']).cuda()
    basis = torch.from_numpy(p['basis']).cuda()
    na = torch.as_tensor(p['na'], dtype=torch.int32).cuda()
    nb = torch.empty(4, dtype=torch.int32, device='cuda')
    cost, steps = torch.empty(4, device='cuda'), torch.empty(4, dtype=torch.int32, device='cuda')
    floor = -1e30                                             # every frame counts: nb = 360

    def call():
        lib.frames_active(b, floor, nb)
        lib.frame_dtw(a, b, na, nb, basis, cost, steps)

    call()
    torch.cuda.synchronize()
    ref = (cost.clone(), steps.clone())
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            call()
    torch.cuda.synchronize()
    cost.fill_(float('nan'))
    steps.fill_(-1)
    nb.fill_(-1)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(cost, ref[0]) and torch.equal(steps, ref[1]) and nb.tolist() == [360] * 4
    same((cost.cpu().numpy(), steps.cpu().numpy()), dr.dtw32(p['a'], p['b'], p['na'], None, p['basis']), 'replay')
    na.copy_(torch.as_tensor([360, 301, 77, 258], dtype=torch.int32) // 2)   # a replay follows what `na` holds at replay time
    g.replay()
    torch.cuda.synchronize()
    same((cost.cpu().numpy(), steps.cpu().numpy()), dr.dtw32(p['a'], p['b'], [180, 150, 38, 129], None, p['basis']), 'replay, other na')


# ---- 11: the model and the driver ----------------------------------------------------------------------------------------------------------
def test_model_mel_distortion(built_lib):
    from tacotron_amd.config import Config
    from tacotron_amd.model import Tacotron
    from tests.util import small_case
    lib = built_lib
    c = Config()
    c.r, c.vocab_size, c.max_decode_iter = 2, 20, 8
    inp, _ = small_case(r=2, V=20, B=3, Tt=9, Td=8, seed=3)
    m = Tacotron(c, {k: torch.as_tensor(inp[k]) for k in ('text', 'text_length')}, train=False, seed=5)
    rng = np.random.default_rng(11)
    m.mel_mean, m.mel_std = rng.standard_normal(160).astype(np.float32), (rng.random(160) + 0.5).astype(np.float32)
    m.run(stop=lib.TacoStopRule(end_offset=100, hold=1, min_steps=3))      # target 0: every row stops after step 2 -> len 4
    frames, na = m.predicted_mel()
    mine = frames.clone()
    cost, steps, na2 = m.mel_distortion(mine, na.clone())                   # a batch against itself
    torch.cuda.synchronize()
    assert na2 is na and na.tolist() == [8, 8, 8] and frames.shape == (3, 16, 80)
    assert cost.tolist() == [0.0, 0.0, 0.0] and steps.tolist() == [8, 8, 8]
    want = lib.denorm_unframe(m.seq2seq_output, torch.as_tensor(m.mel_mean).cuda(), torch.as_tensor(m.mel_std).cuda(), 2)
    assert torch.equal(frames, want)
    rec = mel_like(rng, 3, 11)
    nb = [11, 6, 0]
    m.run()
    out = m.mel_distortion(torch.from_numpy(rec).cuda(), torch.as_tensor(nb, dtype=torch.int32).cuda(), cepstra=5)
    torch.cuda.synchronize()
    assert out[0] is cost and out[1] is steps and out[2] is na and na.tolist() == [16, 16, 16]   # the same tensors, allocated once
    same((cost.cpu().numpy(), steps.cpu().numpy()), dr.dtw32(frames.cpu().numpy(), rec, None, nb, lib.dct_basis(80, 1, 5)), 'model')
    m.check()


def write_corpus(path, n=7, r=2, V=20, Tt=9, Td=8, seed=9):
    """an npy corpus as tacotron_amd.preprocess leaves it: fp16 features in the r-frame layout, every recording padded to Td steps with
    frames of log(1e-8); utterance i holds 4 + i frames (of Td r = 16)"""
    from tacotron_amd.audio import reshape_frames
    rng = np.random.default_rng(seed)
    pad = np.float32(np.log(1e-8))
    os.makedirs(path, exist_ok=True)
    F = Td * r
    frames = []
    mels, stfts = np.empty((n, Td, 80 * r), dtype=np.float16), np.empty((n, Td, 1025 * r), dtype=np.float16)
    for i in range(n):
        mel = np.full((80, F), pad, dtype=np.float32)
        stft = np.full((1025, F), pad, dtype=np.float32)
        mel[:, :4 + i] = mel_like(rng, 1, 4 + i)[0].T
        stft[:, :4 + i] = rng.standard_normal((1025, 4 + i)) - 3.0
        mels[i], stfts[i] = reshape_frames(mel, r), reshape_frames(stft, r)
        frames.append(4 + i)
    text = rng.integers(1, V, size=(n, Tt)).astype(np.int32)
    tl = rng.integers(Tt // 2, Tt + 1, size=n).astype(np.int32)
    text[np.arange(Tt)[None, :] >= tl[:, None]] = 0
    for name, arr in (('texts', text), ('text_lens', tl), ('mels', mels), ('stfts', stfts)):
        np.save(os.path.join(path, name + '.npy'), arr)
    with open(os.path.join(path, 'meta.pkl'), 'wb') as f:
        pickle.dump({'r': r, 'vocab': {i: chr(97 + i) for i in range(V)}}, f)
    return frames, mels


def test_evaluate(built_lib, tmp_path, capsys):
    """tacotron_amd.evaluate.main on a small corpus on disk: 5 held-out utterances in batches of 3 (the second one padded).
    eval_0.npy is the restatement fed with the frames the warp was given; the recorded frames are the stored ones and their counts
    the corpus's; the padded copies are left out."""
    from tacotron_amd import evaluate as ev
    from tacotron_amd.audio import reshape_frames
    from tacotron_amd.config import Config
    lib = built_lib
    frames, mels = write_corpus(str(tmp_path / 'data'))

    def cfg():
        c = Config()
        c.data_path = str(tmp_path / 'data') + '/'
        c.batch_size, c.max_decode_iter = 3, 12
        return c

    out_dir = tmp_path / 'eval'
    rows, mean_loss = ev.main(['--holdout', '5', '--cepstra', '13', '--out-dir', str(out_dir)], config=cfg())
    out = capsys.readouterr().out
    assert sorted(os.listdir(out_dir)) == ['eval_0.npy']
    saved = np.load(out_dir / 'eval_0.npy')
    assert saved.dtype == np.float64 and saved.shape == (5, 6) and np.array_equal(saved, rows)
    assert saved[:, 0].tolist() == [2, 3, 4, 5, 6] and saved[:, 2].tolist() == [frames[i] for i in range(2, 7)]
    assert out.count('\nbatch ') + out.startswith('batch ') == 2 and 'held out: 5 utterances' in out and np.isfinite(mean_loss)
    trace = []
    again, _ = ev.evaluate(cfg(), 5, cepstra=13, out_dir=str(out_dir), trace=trace)
    assert np.array_equal(again, saved)                                     # the same run gives the same bits
    assert len(trace) == 2 and trace[0]['predicted'].shape == (3, 24, 80) and trace[0]['recorded'].shape == (3, 16, 80)
    basis = lib.dct_basis(80, 1, 13)
    at = 0
    for (index, valid), t in zip(ev.holdout_batches(7, 5, 3), trace):
        for row, i in enumerate(index):
            stored = reshape_frames(mels[i].astype(np.float32), 2, forward=False)
            assert np.array_equal(t['recorded'][row], stored) and t['nb'][row] == frames[i]
        cost, steps = dr.dtw32(t['predicted'], t['recorded'], t['na'], t['nb'], basis)
        for row in range(valid):
            want = [index[row], t['na'][row], t['nb'][row], steps[row], float(cost[row]), lib.MCD_DB * float(cost[row]) / steps[row]]
            assert saved[at].tolist() == want, (at, saved[at], want)
            at += 1
    assert at == 5
    assert index.tolist() == [5, 6, 6] and trace[1]['nb'].tolist() == [frames[5], frames[6], frames[6]]   # (the padding repeats the last utterance)
