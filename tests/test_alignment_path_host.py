"""CPU checks of the alignment path (taco_alignment_path): the NumPy restatement (tests/align_path_ref.py) against a brute force over
every admissible path and on cases worked by hand, the C ABI declaration, the export and its ctypes signature, every TACO_EINVAL case
of the library and every refusal of the Python binding, the host arithmetic of the timings (alignment.char_steps, step_samples,
word_times) on hand-worked cases, and the two drivers' options."""
import ctypes as C
import inspect
import itertools
import os
import re

import numpy as np
import pytest
import torch

from tests import align_path_ref as pr

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'taco_hip.h')
IVOCAB = {i + 1: ch for i, ch in enumerate("abcdefghijklmnopqrstuvwxyz '.,?!-")}
IVOCAB[0] = '<pad>'


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def _tie_rule_path(optimal):
    """of all optimal paths: the lowest end, then reading backwards the highest predecessor at every step (the smallest d)"""
    end = min(p[-1] for p in optimal)
    return max((p for p in optimal if p[-1] == end), key=lambda p: tuple(p[::-1]))


def test_restatement_against_brute_force():
    """every shape with Td <= 5, Tt <= 4, J <= 2 on dyadic matrices (multiples of 1/8 from three levels: every sum is exact and ties
    are real): the restatement's mass is the maximum over all admissible paths, its path is admissible, attains it and is the one
    the tie rules name; dur and counts are the path's; the vectorised form gives the same"""
    rng = np.random.default_rng(0)
    seen_ties = 0
    for Td, Tt, J in itertools.product(range(1, 6), range(1, 5), (1, 2)):
        for trial in range(6):
            a = (rng.integers(0, 3, size=(Td, Tt)) / 8.0).astype(np.float32)
            tl = [Tt, int(rng.integers(0, Tt + 2))][trial % 2]
            steps = [None, int(rng.integers(-1, Td + 2))][trial // 2 % 2]
            path, dur, counts, mass = pr.best_path(a, tl, steps, J)
            fast = pr.best_path_fast(a, tl, steps, J)
            assert all(np.array_equal(x, y) for x, y in zip((path, dur, counts), fast[:3])) and mass.tobytes() == fast[3].tobytes()
            L, n = pr.row_args(Td, Tt, tl, steps)
            best, optimal = pr.brute_force(a, tl, steps, J)
            if n == 0:
                assert optimal == [] and (path == -1).all() and (dur == 0).all() and counts.tolist() == [0, 0, 0] and mass.tobytes() == b'\0' * 4
                continue
            p = path[:n]
            assert mass == best and mass.dtype == np.float32
            assert p[0] == 0 and (np.diff(p) >= 0).all() and (np.diff(p) <= J).all() and p[-1] < L and (path[n:] == -1).all()
            assert pr.path_mass(pr.weights(a), p) == best
            assert np.array_equal(p, _tie_rule_path(optimal)), (a, tl, steps, J, p, optimal)
            seen_ties += len(optimal) > 1
            assert np.array_equal(dur, np.bincount(p, minlength=Tt)) and dur.sum() == n
            assert counts.tolist() == [n, p[-1], int((dur[:p[-1] + 1] == 0).sum())]
    assert seen_ties > 20           # (the tie rules were exercised, not just stated)


def test_restatement_on_hand_worked_cases():
    # a noisy diagonal of 36 steps over 20 characters: non-decreasing from 0, increments <= J, durations summing to n
    rng = np.random.default_rng(1)
    a = np.full((36, 20), 0.01, np.float32)
    t = np.arange(36)
    a[t, np.clip(t * 20 // 36 + rng.integers(-1, 2, size=36), 0, 19)] = 0.8
    path, dur, counts, mass = pr.best_path(a, 20, None, 4)
    assert path[0] == 0 and (np.diff(path) >= 0).all() and (np.diff(path) <= 4).all() and dur.sum() == 36 and counts[0] == 36
    assert counts[1] >= 17 and mass > 0.8 * 20
    # an all-equal matrix stays on character 0: d = 0 wins every tie, and the lowest end wins the last one
    path, dur, counts, mass = pr.best_path(np.full((5, 6), 0.25, np.float32), 6, None, 2)
    assert path.tolist() == [0] * 5 and dur.tolist() == [5, 0, 0, 0, 0, 0] and counts.tolist() == [5, 0, 0] and mass == 1.25
    # n < L with J = 1 on a diagonal: the path ends early, e = n - 1
    a = np.full((4, 9), 0.125, np.float32)
    a[np.arange(4), np.arange(4)] = 0.5
    path, dur, counts, mass = pr.best_path(a, 9, None, 1)
    assert path.tolist() == [0, 1, 2, 3] and counts.tolist() == [4, 3, 0] and mass == 2.0
    # the predecessor tie: (2, 2) can come from character 2 (d = 0) or 1 (d = 1) at equal mass -> d = 0
    a = np.array([[0.5, 0, 0], [0, 0.25, 0.25], [0, 0, 0.5]], np.float32)
    path, dur, counts, mass = pr.best_path(a, 3, None, 2)
    assert path.tolist() == [0, 2, 2] and mass == 1.25 and counts.tolist() == [3, 2, 1] and dur.tolist() == [1, 0, 2]
    # what is no weight: NaN, negative values and -0 weigh +0; +inf stays
    a = np.array([[-0.0, 9, 9], [np.nan, -1.0, 0.5], [0.25, np.nan, -np.inf]], np.float32)
    path, dur, counts, mass = pr.best_path(a, 3, None, 1)
    assert path.tolist() == [0, 0, 0] and mass == 0.25 and mass.tobytes() == np.float32(0.25).tobytes()
    assert pr.best_path(np.full((2, 2), -0.0, np.float32), 2, None, 1)[3].tobytes() == b'\0' * 4
    a = np.array([[0.5, 0], [0.25, np.inf], [0.25, 0.0]], np.float32)
    assert pr.best_path(a, 2, None, 1)[0].tolist() == [0, 1, 1] and np.isposinf(pr.best_path(a, 2, None, 1)[3])
    # characters >= L, steps >= n: text_length 2 of 3, steps 2 of 3
    a = np.array([[0.5, 0, 9], [0, 0.5, 9], [9, 9, 9]], np.float32)
    path, dur, counts, mass = pr.best_path(a, 2, 2, 2)
    assert path.tolist() == [0, 1, -1] and dur.tolist() == [1, 1, 0] and counts.tolist() == [2, 1, 0] and mass == 1.0


# ---- the ABI surface ---------------------------------------------------------------------------------------------------------------
def _args(decl):
    return [' '.join(a.split()) for a in decl.replace('\n', ' ').split(',')]


def test_header_declares_the_entry_points():
    hdr = open(HDR).read()
    fn = re.search(r'\bint taco_alignment_path\(([^)]*)\);', hdr)
    size = re.search(r'\bint64_t taco_alignment_path_workspace_bytes\(([^)]*)\);', hdr)
    assert fn and size
    assert _args(fn.group(1)) == ['const float* alignments', 'const int32_t* text_length', 'const int32_t* steps', 'int max_jump',
                                  'int32_t* path', 'int32_t* dur', 'int32_t* counts', 'float* mass', 'void* workspace', 'int B', 'int Td',
                                  'int Tt', 'void* stream']
    assert _args(size.group(1)) == ['int B', 'int Td', 'int Tt']
    scores = hdr.index('int taco_alignment_scores(')
    assert scores < size.start() < fn.start() < hdr.index('int taco_frames_active(')
    assert not re.search(r'^int(64_t)? taco_', hdr[scores + 10:size.start()], re.M)        # directly behind taco_alignment_scores
    limits = {k: int(re.search(r'#define\s+%s\s+(\d+)' % k, hdr).group(1))
              for k in ('TACO_ALIGN_PATH_MAX_TD', 'TACO_ALIGN_PATH_MAX_TT', 'TACO_ALIGN_PATH_MAX_JUMP')}
    assert limits == {'TACO_ALIGN_PATH_MAX_TD': 16384, 'TACO_ALIGN_PATH_MAX_TT': 4096, 'TACO_ALIGN_PATH_MAX_JUMP': 15}
    comment = ' '.join(hdr[hdr.index('/* Alignment path'):size.start()].split())
    for word in ('MASS', 'SMALLEST d', 'lowest s', 'skipped', '+inf', 'detect them by the symbol', 'graph-capturable', 'workspace'):
        assert word in comment, word


def test_library_exports_them(built_lib):
    P, I = C.c_void_p, C.c_int
    assert built_lib.EXPORTS['taco_alignment_path'] == (C.c_int, [P, P, P, I, P, P, P, P, P, I, I, I, P])
    assert built_lib.EXPORTS['taco_alignment_path_workspace_bytes'] == (C.c_int64, [I, I, I])
    so = C.CDLL(built_lib.LIB_PATH)
    assert hasattr(so, 'taco_alignment_path') and hasattr(so, 'taco_alignment_path_workspace_bytes')
    assert built_lib.PATH_COUNTS == ('n', 'end', 'skipped') and built_lib.PATH_JUMP == 4
    assert (built_lib.PATH_MAX_TD, built_lib.PATH_MAX_TT, built_lib.PATH_MAX_JUMP) == (16384, 4096, 15)
    # the product's shapes need no workspace; a wider text or a longer decode take a byte per cell
    assert built_lib.alignment_path_workspace_bytes(32, 180, 200) == 0 and built_lib.alignment_path_workspace_bytes(32, 200, 140) == 0
    assert built_lib.alignment_path_workspace_bytes(3, 7, 257) == 3 * 7 * 257
    assert built_lib.alignment_path_workspace_bytes(1, 16384, 256) == 16384 * 256


def test_library_refuses_bad_arguments(built_lib):
    """every TACO_EINVAL case, at the library itself: rc -1 and a message that names the argument.  The refusals come before the
    launch, so host memory stands in for the device buffers and nothing of it changes."""
    B, Td, Tt = 2, 3, 300
    al = np.full(B * Td * Tt, 0.25, dtype=np.float32)
    tl = np.full(B, 4, dtype=np.int32)
    out = {k: np.full(n, -7, dtype=np.int32) for k, n in (('path', B * Td), ('dur', B * Tt), ('counts', B * 3), ('ws', B * Td * Tt // 4))}
    mass = np.full(B, -7.0, dtype=np.float32)
    p = lambda x: C.c_void_p(x.ctypes.data)   # noqa: E731
    good = dict(al=p(al), tl=p(tl), steps=None, max_jump=2, path=p(out['path']), dur=p(out['dur']), counts=p(out['counts']), mass=p(mass),
                ws=p(out['ws']), B=B, Td=Td, Tt=Tt)
    fn = built_lib._lib.taco_alignment_path
    cases = [(dict(al=None), 'alignments'), (dict(tl=None), 'text_length'), (dict(path=None), 'path'), (dict(dur=None), 'dur'),
             (dict(counts=None), 'counts'), (dict(mass=None), 'mass'), (dict(ws=None), 'workspace'),
             (dict(B=0), 'B='), (dict(B=-1), 'B='), (dict(Td=0), 'Td='), (dict(Td=-4), 'Td='), (dict(Tt=0), 'Tt='), (dict(Tt=-1), 'Tt='),
             (dict(max_jump=0), 'max_jump'), (dict(max_jump=-1), 'max_jump'), (dict(max_jump=16), 'max_jump'),
             (dict(Td=built_lib.PATH_MAX_TD + 1), 'Td='), (dict(Tt=built_lib.PATH_MAX_TT + 1), 'Tt=')]
    for kw, word in cases:
        a = dict(good, **kw)
        rc = fn(a['al'], a['tl'], a['steps'], a['max_jump'], a['path'], a['dur'], a['counts'], a['mass'], a['ws'], a['B'], a['Td'], a['Tt'],
                None)
        assert rc == -1, kw
        msg = built_lib.last_error()
        assert msg.startswith('alignment_path:') and word in msg, (kw, msg)
    assert all((v == -7).all() for v in out.values()) and (mass == -7.0).all() and (al == 0.25).all() and (tl == 4).all()
    size = built_lib._lib.taco_alignment_path_workspace_bytes
    for shape in ((0, 3, 8), (2, 0, 8), (2, 3, 0), (-1, 3, 8), (2, built_lib.PATH_MAX_TD + 1, 8), (2, 3, built_lib.PATH_MAX_TT + 1)):
        assert size(*shape) == -1, shape
    for shape in ((0, 3, 8), (2, 3, built_lib.PATH_MAX_TT + 1), (2, 1.5, 8), (True, 3, 8)):
        with pytest.raises(ValueError, match='^alignment_path_workspace_bytes: '):
            built_lib.alignment_path_workspace_bytes(*shape)


def test_wrapper_refuses_bad_arguments_before_any_device_call(built_lib):
    """every refusal is raised on the host before either symbol is called (CPU tensors never reach them)"""
    B, Td, Tt = 3, 4, 6
    al = torch.zeros(B, Td, Tt)
    tl = torch.ones(B, dtype=torch.int32)
    good = dict(alignments=al, text_length=tl)
    called = []
    real = built_lib._lib.taco_alignment_path, built_lib._lib.taco_alignment_path_workspace_bytes
    i32 = dict(dtype=torch.int32)
    bad = [
        dict(alignments=al.double()), dict(alignments=al.half()), dict(alignments=torch.zeros(Td, Tt)), dict(alignments=torch.zeros(B, 0, Tt)),
        dict(alignments=torch.zeros(B, Tt, Td).transpose(1, 2)),                      # not contiguous
        dict(alignments=np.zeros((B, Td, Tt), dtype=np.float32)),                     # not a tensor
        dict(alignments=torch.zeros(1, 1, 1).expand(1, built_lib.PATH_MAX_TD + 1, 1)),
        dict(alignments=torch.zeros(1, 1, 1).expand(1, 1, built_lib.PATH_MAX_TT + 1)),
        dict(text_length=None), dict(text_length=tl.long()), dict(text_length=torch.ones(B + 1, **i32)), dict(text_length=[1, 1, 1]),
        dict(steps=torch.ones(B)), dict(steps=torch.ones(B - 1, **i32)), dict(steps=[4, 4, 4]),
        dict(max_jump=0), dict(max_jump=-1), dict(max_jump=16), dict(max_jump=1.5), dict(max_jump=True), dict(max_jump=None),
        dict(path=torch.zeros(B, Td)), dict(path=torch.zeros(B, Td + 1, **i32)), dict(path=torch.zeros(Td, B, **i32).t()),
        dict(dur=torch.zeros(B, Tt)), dict(dur=torch.zeros(B, Tt - 1, **i32)),
        dict(counts=torch.zeros(B, 3)), dict(counts=torch.zeros(B, 6, **i32)),
        dict(mass=torch.zeros(B, dtype=torch.float64)), dict(mass=torch.zeros(B, 1)), dict(mass=torch.zeros(B, **i32)),
        dict(workspace=torch.zeros(8)), dict(workspace=torch.zeros(2, 4, dtype=torch.uint8)), dict(workspace=[0]),
        dict(),                                                                       # everything right, but on the CPU
    ]
    try:
        built_lib._lib.taco_alignment_path = lambda *a: called.append(a) or 0
        built_lib._lib.taco_alignment_path_workspace_bytes = lambda *a: called.append(a) or 0
        for kw in bad:
            with pytest.raises(ValueError, match='^alignment_path: '):
                built_lib.alignment_path(**dict(good, **kw))
    finally:
        built_lib._lib.taco_alignment_path, built_lib._lib.taco_alignment_path_workspace_bytes = real
    assert not called
    sig = inspect.signature(built_lib.alignment_path).parameters
    assert [(k, sig[k].default) for k in sig] == [('alignments', inspect.Parameter.empty), ('text_length', inspect.Parameter.empty),
                                                  ('steps', None), ('max_jump', built_lib.PATH_JUMP), ('path', None), ('dur', None),
                                                  ('counts', None), ('mass', None), ('workspace', None)]


# ---- the host arithmetic of the timings --------------------------------------------------------------------------------------------
def test_char_steps():
    from tacotron_amd.alignment import char_steps
    start, end = char_steps([2, 0, 1, 4])
    assert start.tolist() == [0, 2, 2, 3] and end.tolist() == [2, 2, 3, 7]           # the skipped character: start == end
    start, end = char_steps(np.zeros(0, np.int32))
    assert start.shape == end.shape == (0,)
    with pytest.raises(ValueError, match='^char_steps: '):
        char_steps([1, -1])


def test_step_samples():
    from tacotron_amd.alignment import step_samples
    assert step_samples([0, 1, 4], 2).tolist() == [0.0, 600.0, 2400.0]               # step t: frame r t, sample 300 r t
    assert step_samples(4, 5).tolist() == 6000.0
    assert step_samples([4, 8], 2, step_q=131072).tolist() == [1200.0, 2400.0]       # rate 2: half the time
    assert step_samples([4, 8], 2, step_q=32768).tolist() == [4800.0, 9600.0]        # rate 0.5: twice
    assert step_samples([0, 4, 8, 20], 2, trim=(1000, 5000)).tolist() == [0.0, 1400.0, 3800.0, 4000.0]   # - s, clipped to [0, e - s]
    assert step_samples([4, 20], 2, step_q=131072, trim=(1000, 5000)).tolist() == [200.0, 4000.0]       # the trim is of the stretched file
    assert step_samples([4, 20], 2, total=9000).tolist() == [2400.0, 9000.0]         # unfinished: the 300 (frames - 1) samples of the file
    assert step_samples([4, 20], 2, trim=(1000, 5000), total=100).tolist() == [1400.0, 4000.0]          # (a trim says where the file ends)
    assert step_samples([0, 4], 2, trim=(1000, 5000), offset=16000).tolist() == [16000.0, 17400.0]      # the piece's offset, added last


def test_word_times():
    from tacotron_amd.alignment import word_times, words_tsv
    dur = [2, 2, 1, 4, 4, 4, 1]                                # 'hi you' and the newline text_length counts: the surplus is ignored
    #  h 0..2  i 2..4  ' ' 4..5  y 5..9  o 9..13  u 13..17   -> hi: steps 0 .. 4, you: steps 5 .. 17; a step is 2 x 300 samples
    assert word_times('hi you\n', IVOCAB, dur, 2) == [(0.0, 0.15, 'hi'), (0.1875, 0.6375, 'you')]
    assert word_times('hi you\n', IVOCAB, dur, 2, step_q=131072) == [(0.0, 0.075, 'hi'), (0.09375, 0.31875, 'you')]
    assert word_times('hi you\n', IVOCAB, dur, 2, step_q=32768) == [(0.0, 0.3, 'hi'), (0.375, 1.275, 'you')]
    # a trim that cuts into the first word and ends inside the last: 1200 samples off the front, the file holds 7800
    assert word_times('hi you\n', IVOCAB, dur, 2, trim=(1200, 9000)) == [(0.0, 0.075, 'hi'), (0.1125, 0.4875, 'you')]
    assert word_times('hi you\n', IVOCAB, dur, 2, total=9000) == [(0.0, 0.15, 'hi'), (0.1875, 0.5625, 'you')]
    assert word_times('hi you\n', IVOCAB, dur, 2, trim=(1200, 9000), offset=16000) == [(1.0, 1.075, 'hi'), (1.1125, 1.4875, 'you')]
    # characters outside the vocabulary are dropped as load_prompts drops them: 'H' and 'ö' are not encoded, punctuation stays attached
    assert word_times('  Hi, yöu!\n', IVOCAB, [1, 2, 1, 3, 3, 3, 9, 9, 9], 2) == [(0.0, 0.1125, 'i,'), (0.15, 0.4875, 'yu!')]
    # a skipped character inside a word and a word skipped as a whole
    assert word_times('hi you\n', IVOCAB, [2, 0, 1, 4, 4, 4], 2) == [(0.0, 0.075, 'hi'), (0.1125, 0.5625, 'you')]
    assert word_times('hi you\n', IVOCAB, [3, 3, 2, 0, 0, 0], 2) == [(0.0, 0.225, 'hi'), (0.3, 0.3, 'you')]
    assert word_times('hi you\n', IVOCAB, [3, 3], 2) == [(0.0, 0.225, 'hi'), (0.225, 0.225, 'you')]    # a shorter dur: 0 steps for the rest
    assert word_times(' \n', IVOCAB, [4, 4], 2) == [] and word_times('a  b\n', IVOCAB, [1, 1, 1, 1], 1)[1] == (0.05625, 0.075, 'b')
    assert words_tsv([(0.0, 0.15, 'hi'), (0.1875, 0.6375, 'you')]) == '0.000\t0.150\thi\n0.188\t0.637\tyou\n'.replace('0.637', '%.3f' % 0.6375)


def test_path_line():
    from tacotron_amd.alignment import path_line
    line, short = path_line('prompt 3', [8, 7, 1], 2.0, 9, end_offset=1)
    assert not short and line == 'prompt 3 path: mass per step 0.250 over 8 steps, end 7 of 8, 1 skipped'
    line, short = path_line('prompt 3', [8, 6, 0], 2.0, 9, end_offset=1)
    assert short and line.startswith('WARNING prompt 3 path: ') and 'end 6 of 8' in line
    assert path_line('prompt 0', [0, 0, 0], 0.0, 5, end_offset=100) == ('prompt 0 path: mass per step 0.000 over 0 steps, end 0 of 4, 0 skipped', False)


# ---- the drivers' options ----------------------------------------------------------------------------------------------------------
def test_check_options_and_the_command_line(built_lib):
    from tacotron_amd import test as drv
    sig = inspect.signature(drv.check_options).parameters
    assert list(sig)[-1] == 'path_jump' and sig['path_jump'].default is None         # the trailing keyword argument
    for ok in (None, 1, 4, 15):
        drv.check_options(path_jump=ok)
    for bad in (0, 16, -1, 1.5, True, 'x'):
        with pytest.raises(ValueError, match='path_jump'):
            drv.check_options(path_jump=bad)
    a = drv.parse_args([])
    assert a.timings is False and a.path_jump == built_lib.PATH_JUMP
    a = drv.parse_args(['--timings', '--path-jump', '2', '--stop', '--vocode-lengths', '--long', '--deemphasis', '--rate', '0.8', '--pitch', '2',
                        '--align-scores', '--trim-db', '30'])
    assert a.timings and a.path_jump == 2 and a.stop and a.long is not None and a.rate == 0.8 and a.align_scores
    for bad in (['--path-jump', '2'], ['--timings', '--path-jump', '0'], ['--timings', '--path-jump', '16']):
        with pytest.raises(SystemExit):
            drv.parse_args(bad)
    sig = inspect.signature(drv.test).parameters
    assert sig['timings'].default is False and sig['path_jump'].default == built_lib.PATH_JUMP


def test_evaluate_durations_options_and_columns(built_lib):
    from tacotron_amd import evaluate as ev
    assert ev.parse_args([]).durations is False and ev.parse_args(['--durations', '--path-jump', '3']).path_jump == 3
    assert ev.DUR_COLUMNS == ('dur_mae_ms', 'dur_bias_ms', 'path_mass', 'rec_path_mass')
    sig = inspect.signature(ev.evaluate).parameters
    assert sig['durations'].default is False and sig['path_jump'].default == built_lib.PATH_JUMP
    # two utterances of 2 and 3 characters; a step of r = 2 frames at 16 kHz is 37.5 ms
    cols = ev.duration_columns([[2, 3, 0, 0], [1, 1, 1, 0]], [[1, 5, 0, 0], [1, 1, 1, 9]], [2, 3], [[5, 1, 0], [0, 0, 0]], [2.5, 0.0],
                               [[6, 1, 0], [3, 2, 0]], [3.0, 1.5], 37.5)
    assert cols[0].tolist() == [(1 + 2) / 2 * 37.5, (1 - 2) / 2 * 37.5, 0.5, 0.5]
    assert cols[1, :2].tolist() == [0.0, 0.0] and np.isnan(cols[1, 2]) and cols[1, 3] == 0.5   # (the 9 lies behind the text; 0 steps: NaN)
    assert ev.duration_summary(cols) == (28.125, -9.375, 0.5, 0.5)
    assert all(np.isnan(x) for x in ev.duration_summary(np.full((2, 4), np.nan)))
    assert '--durations' in ev.__doc__ and 'mean nothing' in ev.__doc__
