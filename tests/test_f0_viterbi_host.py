"""CPU checks of the smoothed pitch track (taco_f0_viterbi): the NumPy restatement (tests/f0_viterbi_ref.py) on tracks worked by hand
in which each rule decides, its rule 8 against the per-frame pick (tests/f0_ref.pick at ratio = 1), the method itself on a seeded
track with a rival octave and a voicing dip, the host tables, the C ABI declaration, the export and its ctypes signature, every
TACO_EINVAL case of the library and every refusal of the Python binding."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import f0_ref
from tests import f0_viterbi_ref as vr

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'taco_hip.h')
f32 = np.float32


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def track(L, frames):
    """frames: per frame a {row: height} of isolated peaks over a zero floor -> acf (1, L, F) float32"""
    y = np.zeros((1, L, len(frames)), dtype=f32)
    for f, peaks in enumerate(frames):
        for i, h in peaks.items():
            y[0, i, f] = h
    return y


LG8 = np.array([0, 0.5, 1, 1.25, 1.5, 1.75, 2, 2.25], dtype=f32)   # rows 2 and 6 are an octave apart


# ---- the restatement on hand-worked tracks -------------------------------------------------------------------------------------------
def test_kept_candidates_and_their_order():
    # rule 2: the larger v first, the smaller row on equal v; the kept ones in ascending rows; absent slots behind them
    y = track(8, [{2: 0.5, 4: 0.75, 6: 0.5}])
    idx, v = vr.candidates(y, None, 1)
    assert idx[0, :, 0].tolist() == [4] and v[0, :, 0].tolist() == [0.75]
    idx, v = vr.candidates(y, None, 2)
    assert idx[0, :, 0].tolist() == [2, 4] and v[0, :, 0].tolist() == [0.5, 0.75]          # row 2 beats row 6 at equal height
    idx, v = vr.candidates(y, None, 4)
    assert idx[0, :, 0].tolist() == [2, 4, 6, -1] and v[0, :, 0].tolist() == [0.5, 0.75, 0.5, -np.inf]
    # the bias is subtracted before the order is taken: row 6 now leads
    bias = np.zeros(8, dtype=f32)
    bias[6] = -0.5
    idx, v = vr.candidates(y, bias, 1)
    assert idx[0, :, 0].tolist() == [6] and v[0, :, 0].tolist() == [1.0]
    # a plateau has its candidate at its first row (> in front, >= behind); a NaN is never one, and neither are the outer rows
    y = np.array([0.9, 0.5, 0.5, 0.25, np.nan, 0.25, 0.125, 0.9], dtype=f32).reshape(1, 8, 1)
    idx, v = vr.candidates(y, None, 3)
    assert idx[0, :, 0].tolist() == [-1, -1, -1]                                             # (0.5 > 0.9 fails; 0.25 >= NaN fails)
    y[0, 0, 0] = 0.25
    assert vr.candidates(y, None, 3)[0][0, :, 0].tolist() == [1, -1, -1]


def test_one_frame_and_the_end_tie():
    y = track(8, [{2: 0.5, 6: 0.5}])
    per, st, counts, score = vr.paths(y, None, 1, None, LG8, 10, 2, 0.25, 0.0, 0.0)
    assert per[0].tolist() == [11.0] and st[0].tolist() == [0.5] and counts[0].tolist() == [1, 1, 0, 0] and score[0] == 0.5
    # rule 5: a voiced slot at exactly the threshold is the lower slot and wins; just below it the frame is unvoiced
    per, st, counts, score = vr.paths(y, None, 1, None, LG8, 10, 2, 0.5, 0.0, 0.0)
    assert per[0].tolist() == [11.0] and counts[0].tolist() == [1, 1, 0, 0]
    per, st, counts, score = vr.paths(y, None, 1, None, LG8, 10, 2, 0.625, 0.0, 0.0)
    assert bits(per)[0, 0] == 0 and bits(st)[0, 0] == 0 and counts[0].tolist() == [1, 0, 0, 0] and score[0] == 0.625
    # the parabola: y = (0.25, 0.5, 0.375) around row 3 -> a = -0.125, d = (0.25 - 1) + 0.375 = -0.375, delta = 1/6
    y = np.array([0, 0, 0.25, 0.5, 0.375, 0, 0, 0], dtype=f32).reshape(1, 8, 1)
    per, st, _, _ = vr.paths(y, None, 1, None, LG8, 10, 1, 0.25, 0.0, 0.0)
    assert bits(per)[0, 0] == bits(f32(12.0) + f32(-0.0625) / f32(-0.375))[()] and st[0, 0] == 0.5


def test_predecessor_tie_takes_the_lowest_slot():
    # rule 4: both slots of frame 0 have D = 0 and no jump costs anything: every target of frame 1 records predecessor 0
    y = track(8, [{2: 0.5, 6: 0.5}, {4: 0.5}])
    per, st, counts, score = vr.paths(y, None, 1, None, LG8, 10, 2, 0.25, 0.0, 0.0)
    assert per[0].tolist() == [11.0, 13.0] and counts[0].tolist() == [2, 2, 0, 0] and score[0] == 1.0
    # with a jump cost the nearer one wins: row 6 (lg 2) is 0.5 octaves from row 4 (lg 1.5), row 2 (lg 1) too: still a tie, slot 0;
    # from row 5 (lg 1.75) row 6 is nearer
    per, _, counts, score = vr.paths(y, None, 1, None, LG8, 10, 2, 0.25, 0.25, 0.0)
    assert per[0].tolist() == [11.0, 13.0] and score[0] == 0.5 + (0.5 - 0.125)
    y = track(8, [{2: 0.5, 6: 0.5}, {5: 0.5}])
    per, _, counts, score = vr.paths(y, None, 1, None, LG8, 10, 2, 0.25, 0.25, 0.0)
    assert per[0].tolist() == [15.0, 14.0] and counts[0].tolist() == [2, 2, 1, 0] and score[0] == 0.5 + (0.5 - 0.0625)


def test_jump_cost_holds_the_octave():
    # frame 1 offers the octave below (row 6) a little higher than the true one (row 2)
    y = track(8, [{2: 0.5}, {2: 0.375, 6: 0.5}, {2: 0.5}])
    per, _, counts, score = vr.paths(y, None, 1, None, LG8, 10, 3, 0.25, 0.125, 0.0)
    assert per[0].tolist() == [11.0, 11.0, 11.0] and counts[0].tolist() == [3, 3, 1, 0] and score[0] == 1.375
    per, _, counts, score = vr.paths(y, None, 1, None, LG8, 10, 3, 0.25, 0.0, 0.0)
    assert per[0].tolist() == [11.0, 15.0, 11.0] and counts[0].tolist() == [3, 3, 0, 0] and score[0] == 1.5
    # K = 1 keeps only the higher one: nothing to hold on to
    per, _, counts, _ = vr.paths(y, None, 1, None, LG8, 10, 1, 0.25, 0.125, 0.0)
    assert per[0].tolist() == [11.0, 15.0, 11.0] and counts[0].tolist() == [3, 3, 0, 0]


def test_switch_cost_bridges_a_dip_and_an_absent_slot():
    y = track(8, [{2: 0.5}, {2: 0.25}, {2: 0.5}])
    per, st, counts, score = vr.paths(y, None, 1, None, LG8, 10, 3, 0.375, 0.0, 0.125)   # (two of the three slots are absent)
    assert per[0].tolist() == [11.0] * 3 and st[0].tolist() == [0.5, 0.25, 0.5] and counts[0].tolist() == [3, 3, 1, 0] and score[0] == 1.25
    per, st, counts, score = vr.paths(y, None, 1, None, LG8, 10, 3, 0.375, 0.0, 0.0)
    assert per[0].tolist() == [11.0, 0.0, 11.0] and counts[0].tolist() == [3, 2, 0, 2] and score[0] == 1.375
    # a frame without any candidate is unvoiced: its voiced slots are all absent.  The path pays the two switches around it ...
    y = track(8, [{2: 0.5}, {}, {2: 0.5}])
    per, st, counts, score = vr.paths(y, None, 1, None, LG8, 10, 3, 0.125, 0.0, 0.125)
    assert per[0].tolist() == [11.0, 0.0, 11.0] and counts[0].tolist() == [3, 2, 0, 2] and score[0] == 0.5 + (0.125 - 0.125) + (0.5 - 0.125)
    # ... unless they cost more than the two voiced frames bring: then the whole row is unvoiced
    per, st, counts, score = vr.paths(y, None, 1, None, LG8, 10, 3, 0.125, 0.0, 4.0)
    assert not bits(per).any() and not bits(st).any() and counts[0].tolist() == [3, 0, 2, 0] and score[0] == 0.375


def test_rows_and_their_frame_counts():
    rng = np.random.default_rng(3)
    y = rng.standard_normal((4, 9, 6)).astype(f32)
    frames = [-2, 0, 2, 9]
    lg = np.log2(np.arange(4, 13)).astype(f32)
    per, st, counts, score = vr.paths(y, frames, 2, None, lg, 5, 3, 0.3, 0.35, 0.14)
    assert counts[:, 0].tolist() == [0, 0, 4, 6]
    for b in (0, 1):                                                                        # F_b = 0: +0 everywhere, four zeros
        assert not bits(per[b]).any() and not bits(st[b]).any() and counts[b].tolist() == [0, 0, 0, 0] and bits(score)[b] == 0
    assert not bits(per[2, 4:]).any() and not bits(st[2, 4:]).any()
    dirty = y.copy()
    dirty[2, :, 4:] = np.nan
    dirty[[0, 1]] = np.nan
    again = vr.paths(dirty, frames, 2, None, lg, 5, 3, 0.3, 0.35, 0.14)
    for a, b in zip((per, st, score), (again[0], again[1], again[3])):
        assert np.array_equal(bits(a), bits(b))
    assert np.array_equal(counts, again[2])
    one = vr.paths(y[2:3, :, :4].copy(), None, 1, None, lg, 5, 3, 0.3, 0.35, 0.14)           # a row is its own call
    assert np.array_equal(bits(one[0][0]), bits(per[2, :4])) and np.array_equal(one[2][0], counts[2]) and bits(one[3])[0] == bits(score)[2]


# ---- rule 8 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [1, 4, 15])
def test_zero_costs_give_the_per_frame_pick(K):
    rng = np.random.default_rng(80 + K)
    for L, F in ((3, 5), (4, 7), (9, 33), (40, 64), (229, 12)):
        y = rng.standard_normal((3, L, F)).astype(f32)
        y[1, :, ::3] = 0.0                                                                   # all-zero columns: no candidate
        y[2] = np.round(y[2] * 4) / 4                                                        # real ties
        lg = np.log2(np.arange(7, 7 + L)).astype(f32)
        for thr in (0.3, -10.0, 0.5):
            want = f0_ref.pick(y, 8, 1.0, thr)
            per, st, counts, _ = vr.paths(y, None, 1, None, lg, 8, K, thr, 0.0, 0.0)
            assert np.array_equal(bits(per), bits(want[0])) and np.array_equal(bits(st), bits(want[1])), (L, F, K, thr)
            assert (counts[:, 2] == 0).all() and (counts[:, 0] == F).all()
            assert np.array_equal(counts[:, 1], (want[0] > 0).sum(axis=1))


# ---- the method ----------------------------------------------------------------------------------------------------------------------
def octave_track(seed, F=200, run=(40, 160), noise=0.05):
    """true period 20 over the voiced run with a rival peak at lag 40 that is the higher one in every third frame, two frames of a dip
    below the threshold 0.3 in the middle, Gaussian noise on every cell: (1, L, F) over the lags 9 .. 51 (lag_min = 10)"""
    rng = np.random.default_rng(seed)
    lags = np.arange(9, 52, dtype=np.float64)
    bump = lambda centre: np.exp(-0.5 * ((lags - centre) / 1.5) ** 2)   # noqa: E731
    y = np.zeros((len(lags), F))
    for f in range(*run):
        dip = 0.3 if f in (99, 100) else 1.0
        y[:, f] = dip * (0.8 * bump(20) + (0.9 if f % 3 == 0 else 0.7) * bump(40))
    y += noise * rng.standard_normal(y.shape)
    return y.astype(f32)[None], run


def test_path_removes_octave_errors_and_voicing_drops():
    y, (lo, hi) = octave_track(7)
    lg = np.log2(np.arange(9, 52)).astype(f32)
    rival = lambda p: ((p[lo:hi] > 30)).sum()           # noqa: E731  frames of the run on the rival lag (40 +- a few; the true one is 20)
    unvoiced = lambda p: (p[lo:hi] == 0).sum()          # noqa: E731
    outside = lambda p: (p[:lo] > 0).sum() + (p[hi:] > 0).sum()   # noqa: E731
    pick = f0_ref.pick(y, 10, 1.0, 0.3)[0][0]
    assert rival(pick) >= 1 and unvoiced(pick) >= 1     # the per-frame pick leaves at least one of each
    per, _, counts, _ = vr.paths(y, None, 1, None, lg, 10, 4, 0.3, 0.35, 0.14)
    assert rival(per[0]) == 0 and unvoiced(per[0]) == 0 and outside(per[0]) == 0
    assert counts[0, 1] == hi - lo and counts[0, 3] == 2 and counts[0, 2] >= rival(pick) + unvoiced(pick)
    assert (np.abs(per[0, lo:hi] - 20.0) < 2.5).all()


# ---- the host tables -----------------------------------------------------------------------------------------------------------------
def test_tables(built_lib):
    lib = built_lib
    bias, lg, jump, switch = lib.f0_viterbi_tables()
    assert bias.dtype == lg.dtype == np.float32 and bias.shape == lg.shape == (229,)
    lags = np.arange(39, 268, dtype=np.float64)
    assert np.array_equal(lg, np.log2(lags).astype(np.float32)) and np.array_equal(bias, (0.01 * np.log2(lags / 266.0)).astype(np.float32))
    assert bias[227] == 0.0 and (bias[:227] < 0).all() and bias[228] > 0                   # zero at the lowest pitch, lag_max
    # (host float64: 0.35 and 0.14 per 0.01 s, times 0.01 s over the 0.01875 s between frames)
    assert jump == pytest.approx(0.35 / 1.875, rel=1e-14) and switch == pytest.approx(0.14 / 1.875, rel=1e-14)
    b2, l2, j2, s2 = lib.f0_viterbi_tables(sr=8000, fmin=100, fmax=200, octave_cost=0.0, hop=80)
    assert l2.shape == (43,) and not b2.any() and j2 == 0.35 and s2 == 0.14                # (a 0.01 s hop: Praat's own numbers)
    assert (lib.F0_MAX_CAND, lib.F0_CANDIDATES, lib.F0_VITERBI_COUNTS) == (15, 4, ('frames', 'voiced', 'moved', 'switches'))
    for kw in (dict(fmin=0), dict(fmin=500), dict(fmin=20), dict(sr=800, fmin=60, fmax=500), dict(octave_cost=-1), dict(octave_cost=float('nan')),
               dict(octave_cost=float('inf')), dict(hop=0), dict(hop=-3), dict(hop=float('nan'))):
        with pytest.raises(ValueError, match='^f0_(viterbi_tables|lags): '):
            lib.f0_viterbi_tables(**kw)
    assert 'UNTUNED' in lib.f0_viterbi_tables.__doc__ and 'UNTUNED' in lib.f0_viterbi.__doc__
    sig = inspect.signature(lib.f0_viterbi_tables).parameters
    assert [(k, sig[k].default) for k in sig] == [('sr', 16000), ('fmin', 60.0), ('fmax', 400.0), ('octave_cost', 0.01), ('hop', 300)]


# ---- the ABI surface -----------------------------------------------------------------------------------------------------------------
def _args(decl):
    return [' '.join(a.split()) for a in decl.replace('\n', ' ').split(',')]


def test_header_declares_the_entry_points():
    hdr = open(HDR).read()
    fn = re.search(r'\bint taco_f0_viterbi\(([^)]*)\);', hdr)
    size = re.search(r'\bint64_t taco_f0_viterbi_workspace_bytes\(([^)]*)\);', hdr)
    assert fn and size
    assert _args(size.group(1)) == ['int B', 'int L', 'int F', 'int K']
    assert _args(fn.group(1)) == ['const float* acf', 'const int32_t* frames', 'int frames_per_unit', 'const float* bias', 'const float* lg',
                                  'int lag_min', 'int lag_max', 'int K', 'float threshold', 'float jump_cost', 'float switch_cost',
                                  'float* period', 'float* strength', 'int32_t* counts', 'float* score', 'void* workspace', 'int B', 'int F',
                                  'void* stream']
    assert int(re.search(r'#define\s+TACO_F0_MAX_CAND\s+(\d+)', hdr).group(1)) == 15
    assert int(re.search(r'#define\s+TACO_VERSION\s+(\d+)', hdr).group(1)) == 120
    pick = ' '.join(hdr[hdr.index('/* F0 tracker'):hdr.index('int taco_frames_f0(')].split())
    assert 'smoothing across frames (Viterbi)' not in pick and 'taco_f0_viterbi' in pick
    comment = ' '.join(hdr[hdr.index('/* A pitch track smoothed across frames'):size.start()].split())
    for word in ('larger v first, smaller i on equal v', 'lowest p', 'lowest c', 'moved', 'switches', 'ratio = 1', 'graph-capturable',
                 'detect it by the symbol', 'Not here'):
        assert word in comment, word


def test_library_exports_them(built_lib):
    P, I, F = C.c_void_p, C.c_int, C.c_float
    assert built_lib.EXPORTS['taco_f0_viterbi_workspace_bytes'] == (C.c_int64, [I, I, I, I])
    assert built_lib.EXPORTS['taco_f0_viterbi'] == (C.c_int, [P, P, I, P, P, I, I, I, F, F, F, P, P, P, P, P, I, I, P])
    so = C.CDLL(built_lib.LIB_PATH)
    assert hasattr(so, 'taco_f0_viterbi') and hasattr(so, 'taco_f0_viterbi_workspace_bytes')
    assert built_lib.version() == 120
    n = built_lib.f0_viterbi_workspace_bytes(32, 229, 360, 4)
    assert 0 < n <= 32 * 360 * 16 * 12                                                      # three 4-byte planes of sixteen slots at the most


def test_library_refuses_bad_arguments(built_lib):
    """every TACO_EINVAL case, at the library itself: rc -1 and a message that begins `f0_viterbi:` and names the argument.  The
    refusals come before the launch, so host memory stands in for the device buffers and nothing of it changes."""
    lib = built_lib
    B, L, F = 2, 7, 5
    acf = np.full(B * L * F, 0.25, dtype=np.float32)
    lg = np.ones(L, dtype=np.float32)
    per, st, score = (np.full(n, -7.0, dtype=np.float32) for n in (B * F, B * F, B))
    counts = np.full(B * 4, -7, dtype=np.int32)
    ws = np.full(lib.f0_viterbi_workspace_bytes(B, L, F, 3) // 4, -7, dtype=np.int32)
    p = lambda x: C.c_void_p(x.ctypes.data)   # noqa: E731
    names = ('acf', 'frames', 'frames_per_unit', 'bias', 'lg', 'lag_min', 'lag_max', 'K', 'threshold', 'jump_cost', 'switch_cost', 'period',
             'strength', 'counts', 'score', 'workspace', 'B', 'F')
    good = dict(zip(names, (p(acf), None, 1, None, p(lg), 10, 14, 3, 0.3, 0.35, 0.14, p(per), p(st), p(counts), p(score), p(ws), B, F)))
    inside = C.c_void_p(acf.ctypes.data + 8)
    nan, inf = float('nan'), float('inf')
    cases = [(dict(acf=None), 'acf'), (dict(lg=None), 'lg'), (dict(period=None), 'period'), (dict(strength=None), 'strength'),
             (dict(counts=None), 'counts'), (dict(score=None), 'score'), (dict(workspace=None), 'workspace'),
             (dict(period=inside), 'period overlaps'), (dict(strength=inside), 'strength overlaps'), (dict(counts=inside), 'counts overlaps'),
             (dict(score=inside), 'score overlaps'),
             (dict(B=0), 'B='), (dict(B=-1), 'B='), (dict(F=0), 'F='), (dict(F=-2), 'F='), (dict(F=8193), 'F='),
             (dict(lag_min=1, lag_max=5), 'lag_min'), (dict(lag_min=14, lag_max=13), 'lag_min'), (dict(lag_min=2, lag_max=512), 'lags'),
             (dict(K=0), 'K='), (dict(K=16), 'K='), (dict(K=-1), 'K='),
             (dict(threshold=nan), 'threshold'), (dict(threshold=inf), 'threshold'), (dict(threshold=-inf), 'threshold'),
             (dict(jump_cost=-0.5), 'jump_cost'), (dict(jump_cost=nan), 'jump_cost'), (dict(jump_cost=inf), 'jump_cost'),
             (dict(switch_cost=-0.5), 'switch_cost'), (dict(switch_cost=nan), 'switch_cost'), (dict(switch_cost=inf), 'switch_cost'),
             (dict(frames_per_unit=0), 'frames_per_unit'), (dict(frames_per_unit=-1), 'frames_per_unit')]
    fn = lib._lib.taco_f0_viterbi
    for kw, word in cases:
        a = dict(good, **kw)
        assert fn(*[a[k] for k in names], None) == -1, kw
        msg = lib.last_error()
        assert msg.startswith('f0_viterbi:') and word in msg, (kw, msg)
    assert (acf == 0.25).all() and (lg == 1).all() and all((x == -7).all() for x in (per, st, score, counts, ws))
    size = lib._lib.taco_f0_viterbi_workspace_bytes
    for shape in ((0, 7, 5, 3), (-1, 7, 5, 3), (2, 2, 5, 3), (2, 513, 5, 3), (2, 7, 0, 3), (2, 7, 8193, 3), (2, 7, 5, 0), (2, 7, 5, 16)):
        assert size(*shape) == -1, shape
        with pytest.raises(ValueError, match='^f0_viterbi_workspace_bytes: '):
            lib.f0_viterbi_workspace_bytes(*shape)
    assert size(1, 512, 8192, 15) > 0 and size(2, 3, 1, 1) > 0


def test_wrapper_refuses_bad_arguments_before_any_device_call(built_lib):
    """every refusal is raised on the host before either symbol is called (CPU tensors never reach them)"""
    lib = built_lib
    B, L, F = 3, 7, 5
    acf = torch.zeros(B, L, F)
    good = dict(acf=acf, lag_min=10, lag_max=14)
    i32 = dict(dtype=torch.int32)
    nan, inf = float('nan'), float('inf')
    bad = [
        dict(acf=acf.double()), dict(acf=torch.zeros(L, F)), dict(acf=torch.zeros(B, F, L).transpose(1, 2)), dict(acf=np.zeros((B, L, F), np.float32)),
        dict(acf=torch.zeros(B, L, 0)), dict(acf=torch.zeros(1, 1, 1).expand(1, L, 8193)),
        dict(frames=torch.ones(B)), dict(frames=torch.ones(B + 1, **i32)), dict(frames=[1, 1, 1]),
        dict(frames_per_unit=0), dict(frames_per_unit=1.5), dict(frames_per_unit=True),
        dict(lag_min=1, lag_max=5), dict(lag_min=14, lag_max=13), dict(lag_max=15), dict(lag_min=9), dict(lag_min=2.5), dict(lag_max=None),
        dict(acf=torch.zeros(1, 513, 2), lag_min=2, lag_max=512),
        dict(bias=torch.zeros(L + 1)), dict(bias=[0.0] * (L - 1)),
        dict(lg=torch.zeros(L - 1)), dict(lg=[1.0] * (L + 2)),
        dict(candidates=0), dict(candidates=16), dict(candidates=2.5), dict(candidates=True), dict(candidates=None),
        dict(threshold=nan), dict(threshold=inf), dict(threshold=-inf), dict(threshold=1e39),
        dict(jump_cost=-1.0), dict(jump_cost=nan), dict(jump_cost=inf), dict(jump_cost=1e39),
        dict(switch_cost=-1.0), dict(switch_cost=nan), dict(switch_cost=inf),
        dict(out=(torch.zeros(B, F),)), dict(out=(torch.zeros(B, F), torch.zeros(B, F), torch.zeros(B, 4), torch.zeros(B))),
        dict(out=(torch.zeros(B, F + 1), torch.zeros(B, F), torch.zeros(B, 4, **i32), torch.zeros(B))),
        dict(out=(torch.zeros(B, F), torch.zeros(B, F), torch.zeros(B, 3, **i32), torch.zeros(B))),
        dict(out=(torch.zeros(B, F), torch.zeros(B, F), torch.zeros(B, 4, **i32), torch.zeros(B, 1))),
        dict(out=(acf[0, :B], torch.zeros(B, F), torch.zeros(B, 4, **i32), torch.zeros(B))),   # period inside acf
        dict(out=(torch.zeros(B, F), torch.zeros(B, F), torch.zeros(B, 4, **i32), acf[1, 2, :B])),
        dict(workspace=torch.zeros(8)), dict(workspace=torch.zeros(2, 4, dtype=torch.uint8)), dict(workspace=[0]),
        dict(),                                                                             # everything right, but on the CPU
    ]
    called = []
    real = lib._lib.taco_f0_viterbi, lib._lib.taco_f0_viterbi_workspace_bytes
    try:
        lib._lib.taco_f0_viterbi = lambda *a: called.append(a) or 0
        lib._lib.taco_f0_viterbi_workspace_bytes = lambda *a: called.append(a) or 0
        for kw in bad:
            with pytest.raises(ValueError, match='^f0_viterbi: '):
                lib.f0_viterbi(**dict(good, **kw))
    finally:
        lib._lib.taco_f0_viterbi, lib._lib.taco_f0_viterbi_workspace_bytes = real
    assert not called
    sig = inspect.signature(lib.f0_viterbi).parameters
    assert [(k, sig[k].default) for k in sig] == [('acf', inspect.Parameter.empty), ('frames', None), ('frames_per_unit', 1), ('lag_min', 40),
                                                  ('lag_max', 266), ('bias', None), ('lg', None), ('candidates', 4),
                                                  ('threshold', lib.F0_THRESHOLD), ('jump_cost', None), ('switch_cost', None), ('out', None),
                                                  ('workspace', None)]


# ---- the drivers' options ------------------------------------------------------------------------------------------------------------
def test_check_options_and_the_command_lines(built_lib):
    from tacotron_amd import evaluate as ev
    from tacotron_amd import test as drv
    sig = inspect.signature(drv.check_options).parameters
    assert sig['f0_smooth'].default is None and list(sig)[-1] == 'path_jump'
    for ok in (None, False, True, 1, 4, 15):
        drv.check_options(f0=True, f0_smooth=ok)
    drv.check_options(f0_smooth=None)
    for bad in (dict(f0_smooth=True), dict(f0=True, f0_smooth=0), dict(f0=True, f0_smooth=16), dict(f0=True, f0_smooth=1.5),
                dict(f0=True, f0_smooth='x'), dict(f0=True, f0_smooth=True, vocode=False)):
        with pytest.raises(ValueError, match='f0'):
            drv.check_options(**bad)
    a = drv.parse_args([])
    assert a.f0 is None and a.f0_smooth is None
    a = drv.parse_args(['--f0-smooth', '--f0-candidates', '6', '--f0-range', '80,300'])
    assert a.f0 == (80.0, 300.0) and a.f0_smooth == 6
    assert drv.parse_args(['--f0-smooth']).f0 is True and drv.parse_args(['--f0-smooth']).f0_smooth is True
    for bad in (['--f0-candidates', '3'], ['--f0', '--f0-candidates', '3'], ['--f0-smooth', '--f0-candidates', '0']):
        with pytest.raises(SystemExit):
            drv.parse_args(bad)
    assert inspect.signature(drv.test).parameters['f0_smooth'].default is None
    assert '--f0-smooth' in drv.__doc__ and 'smoothing moved M of N frames' in drv.__doc__
    # the per-prompt line
    row = ([5, 1, 0], [5, 1, 0], [7, 0.25, 0], [30, 20, 3, 1])
    assert drv.f0_lines('prompt 3', row[:3], 55109) == ['prompt 3 pitch: asked +3.00, measured +3.00 semitones over 7 voiced frames']
    assert drv.f0_lines('prompt 3', row, 55109) == ['prompt 3 pitch: asked +3.00, measured +3.00 semitones over 7 voiced frames, '
                                                    'smoothing moved 3 of 30 frames']
    assert drv.f0_lines('prompt 3', row[:2] + (None, row[3])) == ['prompt 3 f0: smoothing moved 3 of 30 frames']
    assert drv.f0_lines('prompt 3', row[:2] + (None, None)) == [] and drv.f0_lines('prompt 3', row[:2] + (None,)) == []
    # evaluate
    assert ev.parse_args([]).f0_smooth is False and ev.parse_args(['--f0-smooth', '--f0-aligned']).f0_smooth is True
    assert ev.SMOOTH_COLUMNS == ('f0_moved', 'rec_f0_moved') and inspect.signature(ev.evaluate).parameters['f0_smooth'].default is False
    cols = ev.smooth_columns([[10, 4, 5, 2], [0, 0, 0, 0]], [[8, 8, 0, 0], [4, 0, 1, 0]])
    assert cols[0].tolist() == [0.5, 0.0] and np.isnan(cols[1, 0]) and cols[1, 1] == 0.25
    assert ev.smooth_summary(cols) == (0.5, 0.125) and all(np.isnan(x) for x in ev.smooth_summary(np.full((2, 2), np.nan)))
    assert '--f0-smooth' in ev.__doc__ and 'UNTUNED' in ev.__doc__
