"""taco_f0_viterbi on the GPU (include/taco_hip.h): the pitch track smoothed across frames against the NumPy restatement
(tests/f0_viterbi_ref.py).  Every op-level call goes through lib.f0_viterbi with inputs, outputs and workspace carved from one guarded
arena (tests/poison.py): the outputs and the workspace start as poison, the outputs must be written completely, the guard bands and
the inputs must come back as they were.  Every comparison is exact -- period, strength and score equal in their bits, counts equal:
the input is acf itself and every rule is one rounded fp32 operation, so there is no tolerance to choose.  No test feeds non-finite
values inside a row's first F_b columns."""
import numpy as np
import pytest
import torch

from tests import f0_cases
from tests import f0_ref as fr
from tests import f0_viterbi_ref as vr
from tests.poison import Guarded

pytestmark = pytest.mark.gpu
f32 = np.float32


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def run(lib, acf, frames=None, per_unit=1, bias=None, lg=None, lag_min=8, K=4, threshold=0.3, jump=0.35, switch=0.14, shift=0):
    """one guarded call -> (period, strength, counts, score) as host arrays.  shift: floats by which acf starts behind a 256-byte
    boundary"""
    acf = np.ascontiguousarray(acf, dtype=np.float32)
    B, L, F = acf.shape
    ws_bytes = lib.f0_viterbi_workspace_bytes(B, L, F, K)
    specs = {'acf': ((acf.size + shift,), torch.float32, 'zeros'), 'lg': ((L,), torch.float32, 'zeros'),
             'period': ((B, F), torch.float32, 'qnan'), 'strength': ((B, F), torch.float32, 'qnan'), 'counts': ((B, 4), torch.int32, 'qnan'),
             'score': ((B,), torch.float32, 'ones'), 'ws': ((ws_bytes,), torch.uint8, 'ones')}
    if frames is not None:
        specs['frames'] = ((B,), torch.int32, 'zeros')
    if bias is not None:
        specs['bias'] = ((L,), torch.float32, 'zeros')
    G = Guarded(specs)
    a = G['acf'][shift:].view(B, L, F)
    assert a.data_ptr() % 256 == 4 * shift
    a.copy_(torch.from_numpy(acf))
    G['lg'].copy_(torch.from_numpy(np.asarray(lg, dtype=np.float32)))
    if frames is not None:
        G['frames'].copy_(torch.as_tensor(np.asarray(frames, dtype=np.int32)))
    if bias is not None:
        G['bias'].copy_(torch.from_numpy(np.asarray(bias, dtype=np.float32)))
    out = lib.f0_viterbi(a, G['frames'] if frames is not None else None, per_unit, lag_min, lag_min + L - 3,
                         G['bias'] if bias is not None else None, G['lg'], K, threshold, jump, switch,
                         (G['period'], G['strength'], G['counts'], G['score']), G['ws'])
    torch.cuda.synchronize()
    assert all(o is G[k] for o, k in zip(out, ('period', 'strength', 'counts', 'score')))
    G.check('period', 'strength', 'counts', 'score')
    assert np.array_equal(bits(a.cpu().numpy()), bits(acf)), 'acf was written'
    assert np.array_equal(bits(G['lg'].cpu().numpy()), bits(lg))
    if frames is not None:
        assert np.array_equal(G['frames'].cpu().numpy(), np.asarray(frames, dtype=np.int32))
    if bias is not None:
        assert np.array_equal(bits(G['bias'].cpu().numpy()), bits(bias))
    return tuple(o.cpu().numpy() for o in out)


def same(got, want, label=''):
    for name, g, w in zip(('period', 'strength', 'counts', 'score'), got, want):
        if name == 'counts':
            assert g.dtype == np.int32 and np.array_equal(g, w), '%s counts\n%s\nrestatement\n%s' % (label, g, w)
        else:
            assert g.dtype == np.float32 and np.array_equal(bits(g), bits(w)), '%s %s\n%s\nrestatement\n%s' % (label, name, g, w)


def check(lib, acf, frames=None, per_unit=1, bias=None, lg=None, lag_min=8, K=4, threshold=0.3, jump=0.35, switch=0.14, shifts=(0,),
          label=''):
    want = vr.paths(acf, frames, per_unit, bias, lg, lag_min, K, threshold, jump, switch)
    for shift in shifts:
        same(run(lib, acf, frames, per_unit, bias, lg, lag_min, K, threshold, jump, switch, shift), want, '%s shift=%d' % (label, shift))
    return want


def log_lags(L, lag_min=8):
    return np.log2(np.arange(lag_min - 1, lag_min - 1 + L, dtype=np.float64)).astype(f32)


def noise(rng, B, L, F):
    """seeded normal noise, scaled so that the threshold 0.3 falls among the candidates' heights"""
    return (0.4 * rng.standard_normal((B, L, F))).astype(f32)


def dyadic(rng, B, L, F):
    """acf, lg and bias from a few multiples of 1/8 and 1/4: with dyadic costs every sum is exact, and the ties in the order of the
    candidates, in the predecessor choice and at the end are real"""
    return ((rng.integers(0, 3, size=(B, L, F)) / 8.0).astype(f32), (rng.integers(0, 8, size=L) / 4.0).astype(f32),
            (rng.integers(0, 2, size=L) / 8.0).astype(f32))


DYADIC_COSTS = dict(threshold=0.125, jump=0.125, switch=0.125)

# ---- the shapes at which each part can go wrong --------------------------------------------------------------------------------------
# L: the smallest (one row that can be a candidate), 4 and 5, then fewer rows than a part has threads for (34: 2 rows per part), 66,
# the production 229 + 2, and the cap (32 rows per part: the whole candidate mask).  F walks 1, 2 and the edges of the 32-frame tile
# and of the four frames the path wave keeps in flight; K walks 1 .. 5 and the cap of 15.
PAIRS = [(1, 1), (2, 2), (31, 3), (32, 4), (33, 5), (65, 15), (33, 1), (2, 15), (5, 4), (6, 2)]


@pytest.mark.parametrize('L', [3, 4, 5, 34, 66, 231, 512])
def test_lags_frames_and_candidates(built_lib, L):
    rng = np.random.default_rng(500 + L)
    lg = log_lags(L)
    for n, (F, K) in enumerate(PAIRS):
        label = 'L=%d F=%d K=%d' % (L, F, K)
        bias = (0.01 * (lg - lg[-2])).astype(f32) if n % 2 else None
        check(built_lib, noise(rng, 3, L, F), None, 1, bias, lg, 8, K, shifts=(0, 1), label=label + ' noise')
        y, dlg, dbias = dyadic(rng, 3, L, F)
        check(built_lib, y, None, 1, None if n % 2 else dbias, dlg, 8, K, label=label + ' dyadic', **DYADIC_COSTS)


@pytest.mark.parametrize('per_unit', [1, 2])
def test_frame_counts(built_lib, per_unit):
    """frames negative, 0, inside and beyond F, and NaN behind every row's F_b"""
    rng = np.random.default_rng(60 + per_unit)
    L, F = 40, 65
    lg = log_lags(L)
    for frames in ([-3, 0, 40], [17, 2 ** 30, 33 // per_unit], [0, 1, F]):
        y = noise(rng, 3, L, F)
        for b in range(3):
            y[b, :, vr.row_frames(frames[b], per_unit, F):] = np.nan
        want = check(built_lib, y, frames, per_unit, None, lg, 8, 4, shifts=(0, 1), label='frames=%s x %d' % (frames, per_unit))
        assert want[2][:, 0].tolist() == [vr.row_frames(n, per_unit, F) for n in frames]
        for b in range(3):
            if want[2][b, 0] == 0:
                assert want[2][b].tolist() == [0, 0, 0, 0] and bits(want[3])[b] == 0 and not bits(want[0][b]).any()


def test_back_pointer_capacity(built_lib):
    """F = 8192, the cap: 64 KiB of back pointers and the byte per frame of the path"""
    rng = np.random.default_rng(8192)
    y = noise(rng, 1, 8, 8192)
    want = check(built_lib, y, None, 1, None, log_lags(8), 8, 15, label='F=8192')
    assert want[2][0, 0] == 8192 and 0 < want[2][0, 1] < 8192 and want[2][0, 3] > 0


def test_production_shape_rows(built_lib):
    """229 lags over 360 frames with the Python layer's own tables and costs on a track with a rival octave: the device agrees with the
    restatement, and the path does what it is for"""
    bias, lg, jump, switch = built_lib.f0_viterbi_tables()
    rng = np.random.default_rng(229)
    lags = np.arange(39, 268, dtype=np.float64)
    F = 360
    y = 0.05 * rng.standard_normal((2, 229, F))
    for f in range(60, 300):
        for lag, h in ((80.0, 0.8), (160.0, 0.9 if f % 3 == 0 else 0.7)):
            y[0, :, f] += h * np.exp(-0.5 * ((lags - lag) / 3.0) ** 2)
    y = y.astype(f32)
    want = check(built_lib, y, [F, 200], 1, bias, lg, 40, 4, 0.3, jump, switch, shifts=(0, 1), label='production')
    pick = fr.pick(y[0] - bias[:, None], 40, 1.0, 0.3)[0]                                    # (the per-frame choice among the same scores)
    rival = lambda p: int((p[60:300] > 120).sum())   # noqa: E731
    assert rival(pick) > 40 and 4 * rival(want[0][0]) < rival(pick) and want[2][0, 1] == 240 and want[2][0, 2] > 0


# ---- rule 8 on the device's own output -----------------------------------------------------------------------------------------------
def test_zero_costs_give_the_bits_of_frames_f0(built_lib):
    lib = built_lib
    for case in (f0_cases.small(33, 4, 20, 33), f0_cases.small(17, 2, 15, 31), f0_cases.small(33, 2, 31, 65)):
        x = torch.from_numpy(case.x).cuda()
        frames = torch.as_tensor(np.asarray(case.frames, dtype=np.int32)).cuda()
        per, st, acf = lib.frames_f0(x, frames, case.per_unit, case.weight, case.gain, case.lag_min, case.lag_max, 1.0, case.threshold,
                                     want_acf=True)
        for K in (1, 4, 15):
            got = lib.f0_viterbi(acf, frames, case.per_unit, case.lag_min, case.lag_max, None, None, K, case.threshold, 0.0, 0.0)
            torch.cuda.synchronize()
            assert torch.equal(got[0].view(torch.int32), per.view(torch.int32)), (case.name, K)
            assert torch.equal(got[1].view(torch.int32), st.view(torch.int32)), (case.name, K)
            counts = got[2].cpu().numpy()
            assert (counts[:, 2] == 0).all() and counts[:, 0].tolist() == [vr.row_frames(n, case.per_unit, case.x.shape[2]) for n in case.frames]
            assert np.array_equal(counts[:, 1], (per > 0).sum(dim=1).cpu().numpy())


# ---- independence --------------------------------------------------------------------------------------------------------------------
def test_rows_are_independent(built_lib):
    rng = np.random.default_rng(5)
    B, L, F = 4, 66, 45
    lg = log_lags(L)
    frames = [33, 45, 7, 20]
    y = noise(rng, B, L, F)
    base = run(built_lib, y, frames, 1, None, lg, 8, 5)
    same(base, vr.paths(y, frames, 1, None, lg, 8, 5, 0.3, 0.35, 0.14), 'base')
    dirty = y.copy()
    for b in range(B):
        dirty[b, :, frames[b]:] = np.nan
    same(run(built_lib, dirty, frames, 1, None, lg, 8, 5), base, 'NaN behind F_b')
    other = y.copy()
    other[[0, 2, 3]] = np.nan
    got = run(built_lib, other, [0, 45, 0, 0], 1, None, lg, 8, 5)                           # (their F_b = 0: no NaN inside a row's frames)
    same(tuple(g[1:2] for g in got), tuple(g[1:2] for g in base), 'NaN in the other rows')
    for b in range(B):                                                                      # a row of a B = 4 call is its own B = 1 call
        n = frames[b]
        one = run(built_lib, y[b:b + 1, :, :n].copy(), None, 1, None, lg, 8, 5)
        assert np.array_equal(bits(one[0][0]), bits(base[0][b, :n])) and np.array_equal(bits(one[1][0]), bits(base[1][b, :n]))
        assert np.array_equal(one[2][0], base[2][b]) and bits(one[3])[0] == bits(base[3])[b]


def test_two_calls_give_the_same_bits(built_lib):
    rng = np.random.default_rng(2)
    y = noise(rng, 3, 231, 70)
    a = run(built_lib, y, None, 1, None, log_lags(231), 8, 15)
    b = run(built_lib, y, None, 1, None, log_lags(231), 8, 15)
    same(a, b, 'again')


def test_graph_capture(built_lib):
    """one captured graph of frames_f0 + f0_viterbi + f0_stats replays to the restatement and follows a changed `frames`"""
    lib = built_lib
    case = f0_cases.small(33, 4, 20, 33)
    F = case.x.shape[2]
    x = torch.from_numpy(np.nan_to_num(case.x, nan=0.25)).cuda()                            # (frames will grow over what was cut)
    frames = torch.full((3,), 9, dtype=torch.int32, device='cuda')
    gain = None if case.gain is None else torch.from_numpy(case.gain).cuda()
    weight = None if case.weight is None else torch.from_numpy(case.weight).cuda()
    lg = torch.from_numpy(log_lags(case.lag_max - case.lag_min + 3, case.lag_min)).cuda()
    args = (case.lag_min, case.lag_max, None, lg, 3, 0.3, 0.35, 0.14)
    raw = lib.frames_f0(x, frames, 1, weight, gain, case.lag_min, case.lag_max, 1.0, 0.3, want_acf=True)
    out = lib.f0_viterbi(raw[2], frames, 1, *args)
    ws = torch.empty(lib.f0_viterbi_workspace_bytes(3, raw[2].shape[1], F, 3), dtype=torch.uint8, device='cuda')
    stats = lib.f0_stats(out[0], None, frames, 1)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            lib.frames_f0(x, frames, 1, weight, gain, case.lag_min, case.lag_max, 1.0, 0.3, want_acf=True, out=raw)
            lib.f0_viterbi(raw[2], frames, 1, *args, out=out, workspace=ws)
            lib.f0_stats(out[0], None, frames, 1, out=stats)
    torch.cuda.synchronize()
    for n in ([9, 9, 9], [F, 0, 20]):
        frames.copy_(torch.as_tensor(n, dtype=torch.int32))
        for o in out + (stats,):
            o.view(torch.int32).fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        want = vr.paths(raw[2].cpu().numpy(), n, 1, None, lg.cpu().numpy(), case.lag_min, 3, 0.3, 0.35, 0.14)
        same(tuple(o.cpu().numpy() for o in out), want, 'replay %s' % n)
        assert f0_cases.stats_err(stats.cpu().numpy(), fr.stats(want[0], None, n, 1)) <= fr.F0_STATS_ATOL


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_enqueue_nothing(built_lib):
    lib = built_lib
    B, L, F, K = 2, 7, 5, 3
    rng = np.random.default_rng(11)
    y = noise(rng, B, L, F)
    acf = torch.from_numpy(y).cuda()
    lg = torch.from_numpy(log_lags(L, 10)).cuda()
    per = torch.full((B, F), -9.0, device='cuda')
    st = torch.full((B, F), -9.0, device='cuda')
    counts = torch.full((B, 4), -9, dtype=torch.int32, device='cuda')
    score = torch.full((B,), -9.0, device='cuda')
    ws = torch.full((lib.f0_viterbi_workspace_bytes(B, L, F, K),), 255, dtype=torch.uint8, device='cuda')
    fn, P = lib._lib.taco_f0_viterbi, lib.ptr
    names = ('acf', 'frames', 'frames_per_unit', 'bias', 'lg', 'lag_min', 'lag_max', 'K', 'threshold', 'jump_cost', 'switch_cost', 'period',
             'strength', 'counts', 'score', 'workspace', 'B', 'F')
    good = dict(zip(names, (P(acf), None, 1, None, P(lg), 10, 14, K, 0.3, 0.35, 0.14, P(per), P(st), P(counts), P(score), P(ws), B, F)))
    inside = P(acf[0, 1])
    nan, inf = float('nan'), float('inf')
    cases = [({k: None}, k) for k in ('acf', 'lg', 'period', 'strength', 'counts', 'score', 'workspace')]
    cases += [({k: inside}, k + ' overlaps') for k in ('period', 'strength', 'counts', 'score')]
    cases += [({'B': 0}, 'B='), ({'B': -1}, 'B='), ({'F': 0}, 'F='), ({'F': 8193}, 'F='), ({'lag_min': 1, 'lag_max': 5}, 'lag_min'),
              ({'lag_min': 14, 'lag_max': 13}, 'lag_min'), ({'lag_min': 2, 'lag_max': 512}, 'lags'), ({'K': 0}, 'K='), ({'K': 16}, 'K='),
              ({'threshold': nan}, 'threshold'), ({'threshold': inf}, 'threshold'), ({'jump_cost': -1.0}, 'jump_cost'),
              ({'jump_cost': nan}, 'jump_cost'), ({'jump_cost': inf}, 'jump_cost'), ({'switch_cost': -1.0}, 'switch_cost'),
              ({'switch_cost': nan}, 'switch_cost'), ({'switch_cost': inf}, 'switch_cost'), ({'frames_per_unit': 0}, 'frames_per_unit')]
    for kw, word in cases:
        a = dict(good, **kw)
        assert fn(*[a[k] for k in names], lib.stream_ptr()) == -1, kw
        msg = lib.last_error()
        assert msg.startswith('f0_viterbi:') and word in msg, (kw, msg)
    torch.cuda.synchronize()
    assert (per == -9).all() and (st == -9).all() and (counts == -9).all() and (score == -9).all() and (ws == 255).all()
    assert fn(*[good[k] for k in names], lib.stream_ptr()) == 0                             # and the same arguments, all in place, are taken
    torch.cuda.synchronize()
    same((per.cpu().numpy(), st.cpu().numpy(), counts.cpu().numpy(), score.cpu().numpy()),
         vr.paths(y, None, 1, None, lg.cpu().numpy(), 10, K, 0.3, 0.35, 0.14), 'good')
