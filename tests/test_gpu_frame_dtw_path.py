"""taco_frame_dtw_path / taco_path_f0_scores on the GPU (include/taco_hip.h) against the NumPy restatements (tests/path_ref.py) on
the inputs of tests/path_cases.py, and what is built on them: Tacotron.mel_distortion(want_path=True) and evaluate --f0-aligned.
Every op-level call goes through lib.frame_dtw_path / lib.path_f0_scores with all of its buffers carved from one guarded arena
(tests/poison.py): the outputs and the workspace start as poison, every output element must have been written, the guard bands and
the inputs must come back as they were.  Cost BITS, steps and both path arrays are compared with the restatement exactly, and so is
lib.frame_dtw on the same inputs; the counts of path_f0_scores exactly, its means within path_ref.PATH_SCORES_ATOL of float64."""
import numpy as np
import pytest
import torch

from tests import path_cases as pc
from tests import path_ref as pr
from tests.poison import Guarded

pytestmark = pytest.mark.gpu


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def run(lib, a, b, na=None, nb=None, basis=None, shift=(0, 0), keep=None):
    """one guarded call -> (cost, steps, path_a, path_b) as host arrays, after the same inputs went through lib.frame_dtw for the
    same cost bits and steps.  The path outputs are poisoned with a pattern that is no -1 (the tails are -1), the workspace with 0xff
    bytes (no direction).  keep: a dict that receives the arena and the device tensors"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    B, Fa, C = a.shape
    Fb = b.shape[1]
    K = C if basis is None else basis.shape[0]
    P = Fa + Fb - 1
    specs = {'a': ((a.size + shift[0],), torch.float32, 'zeros'), 'b': ((b.size + shift[1],), torch.float32, 'zeros'),
             'cost': ((B,), torch.float32, 'ones'), 'steps': ((B,), torch.int32, 'ones'),
             'path_a': ((B, P), torch.int32, 'qnan'), 'path_b': ((B, P), torch.int32, 'qnan'),
             'cost0': ((B,), torch.float32, 'ones'), 'steps0': ((B,), torch.int32, 'ones')}
    ints = {'na': na, 'nb': nb}
    for k, v in ints.items():
        if v is not None:
            specs[k] = ((B,), torch.int32, 'zeros')
    if basis is not None:
        specs['basis'] = (basis.shape, torch.float32, 'zeros')
    nbytes = lib.frame_dtw_path_workspace_bytes(B, Fa, Fb, K)
    assert nbytes >= B * P * Fa
    specs['work'] = ((nbytes,), torch.uint8, 'ones')
    n0 = lib.frame_dtw_workspace_bytes(B, Fa, Fb, K)
    if n0:
        specs['work0'] = ((n0,), torch.uint8, 'qnan')
    G = Guarded(specs)
    ta = G['a'][shift[0]:].view(B, Fa, C)
    tb = G['b'][shift[1]:].view(B, Fb, C)
    ta.copy_(torch.from_numpy(a))
    tb.copy_(torch.from_numpy(b))
    for k, v in ints.items():
        if v is not None:
            G[k].copy_(torch.as_tensor(np.asarray(v, dtype=np.int32)))
    if basis is not None:
        G['basis'].copy_(torch.from_numpy(basis))
    tna, tnb = (G['na'] if na is not None else None), (G['nb'] if nb is not None else None)
    tbasis = G['basis'] if basis is not None else None
    out = lib.frame_dtw_path(ta, tb, tna, tnb, tbasis, G['cost'], G['steps'], G['path_a'], G['path_b'], G['work'])
    lib.frame_dtw(ta, tb, tna, tnb, tbasis, G['cost0'], G['steps0'], G['work0'] if n0 else None)
    torch.cuda.synchronize()
    assert out[0] is G['cost'] and out[1] is G['steps'] and out[2] is G['path_a'] and out[3] is G['path_b']
    G.check('cost', 'steps', 'path_a', 'path_b', 'cost0', 'steps0')
    assert np.array_equal(bits(ta.cpu().numpy()), bits(a)) and np.array_equal(bits(tb.cpu().numpy()), bits(b)), 'frames were written'
    for k, v in ints.items():
        if v is not None:
            assert np.array_equal(G[k].cpu().numpy(), np.asarray(v, dtype=np.int32))
    if basis is not None:
        assert np.array_equal(bits(G['basis'].cpu().numpy()), bits(basis))
    got = tuple(G[k].cpu().numpy() for k in ('cost', 'steps', 'path_a', 'path_b'))
    assert np.array_equal(bits(got[0]), bits(G['cost0'].cpu().numpy())) and np.array_equal(got[1], G['steps0'].cpu().numpy()), \
        'cost / steps differ from lib.frame_dtw on the same inputs'
    if keep is not None:
        keep.update(G=G)
    return got


def same(got, want, label='', rows=None):
    rows = slice(None) if rows is None else rows
    assert got[0].dtype == np.float32 and all(x.dtype == np.int32 for x in got[1:])
    assert np.array_equal(got[1][rows], want[1][rows]), '%s steps\n%s\nrestatement\n%s' % (label, got[1], want[1])
    assert np.array_equal(bits(got[0])[rows], bits(want[0])[rows]), '%s cost\n%s\nrestatement\n%s' % (label, got[0], want[0])
    for k, name in ((2, 'path_a'), (3, 'path_b')):
        bad = np.argwhere(got[k][rows] != want[k][rows])
        assert len(bad) == 0, '%s %s differs in %d entries, first at %s: %d, restatement %d' % (
            label, name, len(bad), bad[0], got[k][rows][tuple(bad[0])], want[k][rows][tuple(bad[0])])


# ---- the cases of the table -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(pc.dtw_cases()))
def test_paths(built_lib, name):
    c = pc.dtw_cases()[name]
    got = run(built_lib, c['a'], c['b'], c['na'], c['nb'], c['basis'], c['shift'])
    same(got, pc.dtw_ref(name), name)
    if name == 'small tables':
        assert got[1].tolist()[:3] == [1, 7, 7] and got[1].tolist()[4:] == [0, 0]
        assert (got[2][4:] == -1).all() and (got[3][4:] == -1).all()                       # the empty rows: -1 throughout
        assert got[2][1, :7].tolist() == [0] * 7 and got[3][1, :7].tolist() == list(range(7))   # a single row of the table
        assert got[2][2, :7].tolist() == list(range(7)) and got[3][2, :7].tolist() == [0] * 7   # a single column
    if name == 'envelope':
        F = built_lib.DTW_MAX_FRAMES
        assert built_lib.frame_dtw_workspace_bytes(1, F, F, 32) > 0 and got[2].shape == (1, 2 * F - 1)
    if name == 'doubled':
        assert got[2][0, :42].tolist() == [t // 2 for t in range(42)]


def test_nan_behind_the_lengths_and_in_another_row(built_lib):
    c = pc.dtw_cases()['isolation']
    clean = pc.dtw_ref('isolation')
    pa, pb = c['a'].copy(), c['b'].copy()
    for r in range(4):
        pa[r, c['na'][r]:] = np.nan
        pb[r, c['nb'][r]:] = np.nan
    pa[2], pb[2] = np.nan, np.inf                            # a whole row: its own result is unspecified, the others' are not
    got = run(built_lib, pa, pb, c['na'], c['nb'], c['basis'])
    same(got, clean, 'poisoned', rows=[0, 1, 3])


def test_two_calls_give_the_same_bits(built_lib):
    c = pc.dtw_cases()['product shape']
    x = run(built_lib, c['a'], c['b'], c['na'], c['nb'], c['basis'])
    y = run(built_lib, c['a'], c['b'], c['na'], c['nb'], c['basis'])
    assert np.array_equal(bits(x[0]), bits(y[0])) and all(np.array_equal(p, q) for p, q in zip(x[1:], y[1:]))
    same(x, pc.dtw_ref('product shape'), 'no shift')


def test_bad_arguments_enqueue_nothing(built_lib):
    lib, P = built_lib, built_lib.ptr
    a = torch.rand(2, 6, 4, device='cuda')
    b = torch.rand(2, 5, 4, device='cuda')
    basis = torch.rand(3, 4, device='cuda')
    cost = torch.full((2,), float('nan'), device='cuda')
    steps = torch.full((2,), -7, dtype=torch.int32, device='cuda')
    path_a = torch.full((2, 10), -7, dtype=torch.int32, device='cuda')
    path_b = torch.full((2, 10), -7, dtype=torch.int32, device='cuda')
    M = lib.DTW_MAX_FRAMES
    work = torch.full((lib.frame_dtw_path_workspace_bytes(1, M, M, lib.DTW_MAX_K),), 0xee, dtype=torch.uint8, device='cuda')
    fn = lib._lib.taco_frame_dtw_path
    good = dict(a=P(a), na=None, b=P(b), nb=None, basis=P(basis), cost=P(cost), steps=P(steps), path_a=P(path_a), path_b=P(path_b),
                work=P(work), B=2, Fa=6, Fb=5, C=4, K=3)
    assert fn(*good.values(), lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert not torch.isnan(cost).any() and (steps > 0).all() and (path_a[:, 0] == 0).all() and (path_a != -7).all()
    cost.fill_(float('nan'))
    for t in (steps, path_a, path_b):
        t.fill_(-7)
    work.fill_(0xee)
    bad = [dict(a=None), dict(b=None), dict(cost=None), dict(steps=None), dict(B=0), dict(B=-2), dict(Fa=0), dict(Fb=0), dict(Fb=-1),
           dict(C=0), dict(K=0), dict(K=-3), dict(basis=None), dict(basis=None, K=5), dict(K=lib.DTW_MAX_K + 1),
           dict(basis=None, C=lib.DTW_MAX_K + 1, K=lib.DTW_MAX_K + 1), dict(C=lib.DTW_MAX_C + 1), dict(Fa=M + 1), dict(Fb=M + 1),
           dict(Fa=M, Fb=M, K=lib.DTW_MAX_K, work=None),    # every refusal of taco_frame_dtw, then the path form's own
           dict(path_a=None), dict(path_b=None), dict(work=None)]
    for change in bad:
        args = dict(good, **change)
        assert fn(*args.values(), lib.stream_ptr()) == -1, change
        assert lib.last_error().startswith('frame_dtw_path:'), (change, lib.last_error())
    torch.cuda.synchronize()
    assert torch.isnan(cost).all() and all((t == -7).all() for t in (steps, path_a, path_b)) and (work == 0xee).all()


# ---- path_f0_scores ---------------------------------------------------------------------------------------------------------------------
def scores(lib, s, paths=None):
    """one guarded call on a case of path_cases.score_cases -> (counts, means); paths: device tensors (path_a, path_b, steps) to use
    instead of the case's"""
    pa, pb = s['period_a'], s['period_b']
    B, P = pa.shape[0], pa.shape[1] + pb.shape[1] - 1
    specs = {'period_a': (pa.shape, torch.float32, 'zeros'), 'period_b': (pb.shape, torch.float32, 'zeros'),
             'path_a': ((B, P), torch.int32, 'zeros'), 'path_b': ((B, P), torch.int32, 'zeros'), 'steps': ((B,), torch.int32, 'zeros'),
             'counts': ((B, 5), torch.int32, 'ones'), 'means': ((B, 2), torch.float32, 'qnan')}
    G = Guarded(specs)
    for k in ('period_a', 'period_b', 'path_a', 'path_b', 'steps'):
        G[k].copy_(torch.from_numpy(np.ascontiguousarray(s[k])))
    if paths is not None:
        for k, t in zip(('path_a', 'path_b', 'steps'), paths):
            G[k].copy_(t)
    counts, means = lib.path_f0_scores(G['period_a'], G['period_b'], G['path_a'], G['path_b'], G['steps'], pc.GROSS, G['counts'], G['means'])
    torch.cuda.synchronize()
    assert counts is G['counts'] and means is G['means']
    G.check('counts', 'means')
    for k in ('period_a', 'period_b'):
        assert np.array_equal(bits(G[k].cpu().numpy()), bits(s[k]))
    return counts.cpu().numpy(), means.cpu().numpy()


def close(got, want, label):
    (c, m), (rc, rm) = got, want
    assert c.dtype == np.int32 and m.dtype == np.float32
    assert np.array_equal(c, rc), '%s counts\n%s\nrestatement\n%s' % (label, c, rc)
    err = np.abs(m.astype(np.float64) - rm)
    print('  %-14s |means - fp64| max %.3e (allowed %.3e)' % (label, err.max(), pr.PATH_SCORES_ATOL))
    assert (err <= pr.PATH_SCORES_ATOL).all(), (label, m, rm)


@pytest.mark.parametrize('name', list(pc.score_cases()))
def test_path_f0_scores(built_lib, name):
    s = pc.score_cases()[name]
    want = pr.path_scores(s['period_a'], s['period_b'], s['path_a'], s['path_b'], s['steps'], pc.GROSS)
    got = scores(built_lib, s)
    close(got, want, name)
    empty = want[0][:, 1] == 0
    assert (bits(got[1][empty]) == 0).all()                  # +0 where no cell is voiced in both
    again = scores(built_lib, s)
    assert np.array_equal(got[0], again[0]) and np.array_equal(bits(got[1]), bits(again[1]))


def test_path_f0_scores_on_the_devices_own_paths(built_lib):
    lib = built_lib
    c = pc.dtw_cases()['product shape']
    s = pc.score_cases()['product paths']
    dev = lambda x, dt=None: torch.as_tensor(np.asarray(x), dtype=dt).cuda()   # noqa: E731
    _, steps, path_a, path_b = lib.frame_dtw_path(dev(c['a']), dev(c['b']), dev(c['na'], torch.int32), dev(c['nb'], torch.int32),
                                                  dev(c['basis']))
    want = pr.path_scores(s['period_a'], s['period_b'], s['path_a'], s['path_b'], s['steps'], pc.GROSS)
    close(scores(lib, s, (path_a, path_b, steps)), want, 'device paths')


def test_path_f0_scores_bad_arguments_enqueue_nothing(built_lib):
    lib, P = built_lib, built_lib.ptr
    pa, pb = torch.rand(2, 5, device='cuda') + 50, torch.rand(2, 4, device='cuda') + 50
    ia = torch.zeros(2, 8, dtype=torch.int32, device='cuda')
    n = torch.ones(2, dtype=torch.int32, device='cuda')
    counts = torch.full((2, 5), -7, dtype=torch.int32, device='cuda')
    means = torch.full((2, 2), float('nan'), device='cuda')
    fn = lib._lib.taco_path_f0_scores
    good = dict(pa=P(pa), pb=P(pb), ia=P(ia), ib=P(ia), n=P(n), gross=1.2, counts=P(counts), means=P(means), B=2, Fa=5, Fb=4)
    assert fn(*good.values(), lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert counts.tolist() == [[1, 1, 0, 0, 0]] * 2 and not torch.isnan(means).any()
    counts.fill_(-7)
    means.fill_(float('nan'))
    M = lib.DTW_MAX_FRAMES
    for change in (dict(pa=None), dict(pb=None), dict(ia=None), dict(ib=None), dict(n=None), dict(counts=None), dict(means=None),
                   dict(B=0), dict(B=-1), dict(Fa=0), dict(Fb=-3), dict(Fa=M + 1), dict(Fb=M + 1), dict(gross=1.0), dict(gross=0.0),
                   dict(gross=-2.0), dict(gross=float('nan'))):
        assert fn(*dict(good, **change).values(), lib.stream_ptr()) == -1, change
        assert lib.last_error().startswith('path_f0_scores:'), (change, lib.last_error())
    torch.cuda.synchronize()
    assert (counts == -7).all() and torch.isnan(means).all()


# ---- graph capture -------------------------------------------------------------------------------------------------------------------------
def test_graph_capture(built_lib):
    """one captured frames_active + frame_dtw_path + path_f0_scores replays to the restatement, and follows what `na` holds at replay
    time"""
    lib = built_lib
    c, s = pc.dtw_cases()['product shape'], pc.score_cases()['product paths']
    a, b, basis = (torch.from_numpy(c[k]).cuda() for k in ('a', 'b', 'basis'))
    pa, pb = torch.from_numpy(s['period_a']).cuda(), torch.from_numpy(s['period_b']).cuda()
    na = torch.as_tensor(c['na'], dtype=torch.int32).cuda()
    nb = torch.empty(4, dtype=torch.int32, device='cuda')
    cost, steps = torch.empty(4, device='cuda'), torch.empty(4, dtype=torch.int32, device='cuda')
    path_a, path_b = (torch.empty(4, 719, dtype=torch.int32, device='cuda') for _ in range(2))
    work = torch.empty(lib.frame_dtw_path_workspace_bytes(4, 360, 360, 13), dtype=torch.uint8, device='cuda')
    counts, means = torch.empty(4, 5, dtype=torch.int32, device='cuda'), torch.empty(4, 2, device='cuda')
    floor = -1e30                                             # every frame counts: nb = 360

    def call():
        lib.frames_active(b, floor, nb)
        lib.frame_dtw_path(a, b, na, nb, basis, cost, steps, path_a, path_b, work)
        lib.path_f0_scores(pa, pb, path_a, path_b, steps, pc.GROSS, counts, means)

    g = torch.cuda.CUDAGraph()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        call()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=st):
            call()
    torch.cuda.synchronize()
    for lengths in (c['na'], [180, 150, 38, 129]):
        na.copy_(torch.as_tensor(lengths, dtype=torch.int32))
        cost.fill_(float('nan'))
        for t in (steps, path_a, path_b, counts, nb):
            t.fill_(-7)
        means.fill_(float('nan'))
        work.fill_(0xff)
        g.replay()
        torch.cuda.synchronize()
        want = pr.dtw32_path(c['a'], c['b'], lengths, None, c['basis'])
        same((cost.cpu().numpy(), steps.cpu().numpy(), path_a.cpu().numpy(), path_b.cpu().numpy()), want, 'replay %s' % (lengths,))
        close((counts.cpu().numpy(), means.cpu().numpy()),
              pr.path_scores(s['period_a'], s['period_b'], want[2], want[3], want[1], pc.GROSS), 'replay')
        assert nb.tolist() == [360] * 4


# ---- the model and the driver ------------------------------------------------------------------------------------------------------------
def test_model_mel_distortion_with_the_path(built_lib):
    from tacotron_amd.config import Config
    from tacotron_amd.model import Tacotron
    from tests.util import small_case
    lib = built_lib
    c = Config()
    c.r, c.vocab_size, c.max_decode_iter = 2, 20, 8
    inp, _ = small_case(r=2, V=20, B=3, Tt=9, Td=8, seed=3)
    m = Tacotron(c, {k: torch.as_tensor(inp[k]) for k in ('text', 'text_length')}, train=False, seed=5)
    m.run(stop=lib.TacoStopRule(end_offset=100, hold=1, min_steps=3))      # every row stops after step 2 -> 8 frames
    frames, na = m.predicted_mel()
    plain = m.mel_distortion(frames.clone(), na.clone())
    assert len(plain) == 3                                                  # the default: what it returned before
    cost, steps, na2, path_a, path_b = m.mel_distortion(frames.clone(), na.clone(), want_path=True)   # a batch against itself
    torch.cuda.synchronize()
    assert cost is plain[0] and steps is plain[1] and na2 is na and na.tolist() == [8, 8, 8]
    assert cost.tolist() == [0.0, 0.0, 0.0] and steps.tolist() == [8, 8, 8] and path_a.shape == (3, 31) and path_a.dtype == torch.int32
    want = [list(range(8)) + [-1] * 23] * 3
    assert path_a.tolist() == want and path_b.tolist() == want
    again = m.mel_distortion(frames.clone(), na.clone(), want_path=True)
    assert again[3] is path_a and again[4] is path_b                        # allocated once
    m.check()


def test_evaluate_f0_aligned(built_lib, tmp_path, capsys):
    """evaluate --f0-aligned on a small corpus on disk: the 12 columns of a --f0 run bit for bit, five more behind them that the
    restatement gives from the traced frames and the tracked periods; a plain --f0 run prints and saves what it did"""
    from tacotron_amd import evaluate as ev
    from tacotron_amd.config import Config
    from tests.test_gpu_frame_dtw import write_corpus
    lib = built_lib
    write_corpus(str(tmp_path / 'data'))

    def cfg():
        c = Config()
        c.data_path = str(tmp_path / 'data') + '/'
        c.batch_size, c.max_decode_iter = 3, 12
        return c

    f0_rows, _ = ev.main(['--holdout', '5', '--cepstra', '13', '--f0', '--out-dir', str(tmp_path / 'f0')], config=cfg())
    f0_out = capsys.readouterr().out
    assert f0_rows.shape == (5, 12) and 'not aligned' in f0_out and '(aligned)' not in f0_out and 'aligned)' in f0_out
    assert np.array_equal(np.load(tmp_path / 'f0' / 'eval_0.npy'), f0_rows, equal_nan=True)
    rows, _ = ev.main(['--holdout', '5', '--cepstra', '13', '--f0-aligned', '--out-dir', str(tmp_path / 'al')], config=cfg())
    out = capsys.readouterr().out
    saved = np.load(tmp_path / 'al' / 'eval_0.npy')
    assert rows.shape == (5, 17) and saved.dtype == np.float64 and np.array_equal(saved, rows, equal_nan=True)
    assert np.array_equal(rows[:, :12].view(np.uint64), f0_rows.view(np.uint64))            # the first 12 columns, bit for bit
    added = [line for line in out.splitlines() if line.endswith('aligned)') and 'not aligned' not in line]
    assert len(added) == 3 and added[0].startswith('batch 0 F0 RMSE') and added[2].startswith('held out: F0 RMSE')
    assert [line for line in out.splitlines() if line not in added] == f0_out.splitlines()  # nothing else changed
    trace = []
    again, _ = ev.evaluate(cfg(), 5, cepstra=13, out_dir=str(tmp_path / 'al'), trace=trace, f0_aligned=True)
    capsys.readouterr()
    assert np.array_equal(again, rows, equal_nan=True)
    basis = lib.dct_basis(80, 1, 13)
    at = 0
    for (index, valid), t in zip(ev.holdout_batches(7, 5, 3), trace):
        assert t['period'].shape == (3, 24) and t['rec_period'].shape == (3, 16)
        _, steps, path_a, path_b = pr.dtw32_path(t['predicted'], t['recorded'], t['na'], t['nb'], basis)
        counts, means = pr.path_scores(t['period'], t['rec_period'], path_a, path_b, steps, ev.GROSS)
        want = ev.aligned_columns(counts, means)
        for row in range(valid):
            got = rows[at, 12:]
            assert rows[at, 3] == steps[row] == counts[row, 0]
            assert np.array_equal(got[[0, 3, 4]], want[row, [0, 3, 4]], equal_nan=True), (at, got, want[row])
            assert np.array_equal(np.isnan(got), np.isnan(want[row]))
            if counts[row, 1]:
                assert np.abs(got[1:3] - want[row, 1:3]).max() <= 1200.0 * pr.PATH_SCORES_ATOL, (at, got, want[row])
            at += 1
    assert at == 5
