"""CPU: prosody inside an utterance without a GPU -- the header's declarations and the binding of the three curve entry points, the
properties of the NumPy restatement (tests/curve_ref.py), the host arithmetic of tacotron_amd.lib, alignment.word_values /
word_times(src=...), and the driver's --prosody option with every refusal.  No compute calls."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import curve_ref as cr
from tests import stretch_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IVOCAB = {i: ch for i, ch in enumerate(['<pad>'] + list("abcdefghijklmnopqrstuvwxyz '.,?!-"))}


def _rows(B, Cw, F, seed=0):
    rng = np.random.default_rng(seed)
    return np.exp(rng.standard_normal((B, Cw, F)) * 2.0).astype(np.float32)


# ---- header and binding ------------------------------------------------------------------------------------------------------------
DECLS = {
    'taco_path_curve': (['const int32_t* path', 'const int32_t* values', 'int frames_per_step', 'int32_t fill', 'int32_t* curve', 'int B',
                         'int Td', 'int Tt', 'void* stream'], 'PPIiPIIIP'),
    'taco_frames_stretch_curve': (['const float* mag_t', 'const int32_t* frames', 'int frames_per_unit', 'const int32_t* dur_q',
                                   'float* out', 'int32_t* frames_out', 'int32_t* src', 'int B', 'int C', 'int F', 'int Fo',
                                   'void* stream'], 'PPIPPPPIIIIP'),
    'taco_frames_pitch_curve': (['const float* mag_t', 'const int32_t* frames', 'int frames_per_unit', 'const int32_t* step_q',
                                 'int lifter', 'float* out', 'int B', 'int C', 'int F', 'void* stream'], 'PPIPIPIIIP'),
}


def test_header_declares_and_the_library_exports_the_three_entry_points(built_lib):
    hdr = open(os.path.join(ROOT, 'include', 'taco_hip.h')).read()
    kinds = {'P': C.c_void_p, 'I': C.c_int, 'i': C.c_int32}
    so = C.CDLL(built_lib.LIB_PATH)
    for name, (args, sig) in DECLS.items():
        decl = re.search(r'int\s+%s\s*\(([^)]*)\)\s*;' % name, hdr)
        assert decl, 'include/taco_hip.h does not declare %s' % name
        assert [' '.join(a.split()) for a in decl.group(1).split(',')] == args
        assert built_lib.EXPORTS[name] == (C.c_int, [kinds[k] for k in sig])
        assert hasattr(so, name), 'the built library does not export %s' % name
    for name in ('path_curve', 'frames_stretch_curve', 'frames_pitch_curve', 'stretch_dur', 'stretch_curve_capacity'):
        assert callable(getattr(built_lib, name))
    assert 'Not here: a rate that varies' not in hdr and 'a pitch contour inside an utterance, mel' not in hdr   # the clauses this closes


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dur,step', [(16384, 262144), (32768, 131072), (65536, 65536), (131072, 32768), (262144, 16384)])
def test_power_of_two_constants_equal_the_constant_rate_stretch(dur, step):
    """a constant duration 65536 / rate and the constant step 65536 * rate: the same map, the same Fo_b, the same bits"""
    for F_b in (1, 2, 3, 7, 300, 8192):
        n, i, wq = cr.time_map(np.full(F_b, dur), F_b, sr.MAX_FRAMES)
        assert n == sr.out_frames(F_b, step, sr.MAX_FRAMES)
        ri, rfrac = sr.positions(n, step)
        assert np.array_equal(i, ri) and np.array_equal(wq, rfrac)
    x = _rows(2, 3, 37, seed=1)
    got, gn, _ = cr.stretch_curve(x, (37, 20), np.full((2, 37), dur), 1, 160)
    want, wn = sr.stretch(x, (37, 20), (step, step), 1, 160)
    assert gn.tolist() == wn.tolist() and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_the_map_rises_strictly_and_ends_inside_the_row():
    rng = np.random.default_rng(2)
    for F_b in (1, 2, 3, 7, 300, 2000):
        d = rng.integers(16384, 262145, F_b)
        n, i, wq = cr.time_map(d, F_b, sr.MAX_FRAMES)
        D, _ = cr.starts(d, F_b)
        assert n == min(sr.MAX_FRAMES, (int(D[-1]) >> 16) + 1) and n >= 1
        packed = (i << 16) | wq
        assert (np.diff(packed) > 0).all() and packed[0] == 0
        assert (wq[i == F_b - 1] == 0).all()                       # on the last source frame only with wq == 0
        assert ((wq >= 0) & (wq < 65536)).all() and int(i.max()) <= F_b - 1


def test_the_sum_of_durations_needs_the_32nd_bit():
    D, d = cr.starts(np.full(8192, 262144), 8192)
    assert int(D[-1]) + int(d[-1]) == 2 ** 31 and int(D[-1]) < 2 ** 32 and int(D[-1]) + int(d[-1]) > np.iinfo(np.int32).max
    n, i, wq = cr.time_map(np.full(8192, 262144), 8192, 8192)
    assert n == 8192 and int(i[-1]) == 2047 and int(wq[-1]) == 3 << 14


def test_clamps_null_durations_and_nan_behind_the_row():
    x = _rows(3, 2, 9, seed=3)
    a = cr.stretch_curve(x, None, np.array([[0] * 9, [-5] * 9, [2 ** 30] * 9]), 1, 40)
    b = cr.stretch_curve(x, None, np.array([[16384] * 9, [16384] * 9, [262144] * 9]), 1, 40)
    assert all(np.array_equal(p, q) for p, q in zip(a, b)) and a[1].tolist() == [3, 3, 33]
    out, n, src = cr.stretch_curve(x, (9, 4, 0), None, 1, 12)
    assert n.tolist() == [9, 4, 0] and np.array_equal(out[0, :, :9].view(np.uint32), x[0].view(np.uint32)) and not out[:, :, 9:].any()
    assert src[1].tolist() == [0, 1 << 16, 2 << 16, 3 << 16] + [-1] * 8 and (src[2] == -1).all()
    dirty = x.copy()
    dirty[1, :, 4:] = np.nan
    d = np.random.default_rng(4).integers(16384, 262145, (3, 9))
    clean, dirt = cr.stretch_curve(x, (9, 4, 0), d, 1, 40), cr.stretch_curve(dirty, (9, 4, 0), d, 1, 40)
    assert np.isfinite(dirt[0]).all() and np.array_equal(clean[0].view(np.uint32), dirt[0].view(np.uint32))


def test_path_curve_and_pitch_curve_restatements():
    path = np.array([[0, 0, 2, 3, -1], [1, 4, 9, -2, -1]])
    values = np.arange(10).reshape(2, 5) * 10
    assert cr.path_curve(path, values, 2, -7).tolist() == [[0, 0, 0, 0, 20, 20, 30, 30, -7, -7], [60, 60, 90, 90, -7, -7, -7, -7, -7, -7]]
    from tests import pitch_ref as pr
    x = _rows(1, 17, 6, seed=5)
    steps = np.array([[65536, 40000, 40000, 0, 65536, 99999]])
    got = cr.pitch_curve(x, (5,), steps, 1, 4)
    assert np.array_equal(got[0][:, [0, 4]], x[0][:, [0, 4]].astype(np.float64)) and not got[0][:, 5].any()
    # (float64 sums whose order depends on how many frames one product holds: equal to rounding, 1e-12 is 4 decimal digits above it)
    assert np.allclose(got[0][:, 1:3], pr.shift_frames(x[0][:, 1:3], 40000, 4), rtol=1e-12, atol=0)
    assert np.allclose(got[0][:, 3], pr.shift_frames(x[0][:, 3:4], 32768, 4)[:, 0], rtol=1e-12, atol=0)       # step 0 clamps to 32768
    assert np.abs(got[0][:, 1] / x[0][:, 1] - 1.0).max() > 0.01


# ---- tacotron_amd.lib ----------------------------------------------------------------------------------------------------------------
def test_stretch_dur_and_capacity(built_lib):
    lib = built_lib
    assert [lib.stretch_dur(r) for r in (4, 2, 1, 0.5, 0.25)] == [16384, 32768, 65536, 131072, 262144]
    assert lib.stretch_dur(0.8) == 81920 and lib.stretch_dur(1.25) == 52429
    for bad in (0.2499, 4.0001, 0.0, -1.0, float('nan'), float('inf'), None, 'slow'):
        with pytest.raises(ValueError):
            lib.stretch_dur(bad)
    assert lib.stretch_curve_capacity(300, 262144) == 1197 and lib.stretch_curve_capacity(16, 65536) == 16
    assert lib.stretch_curve_capacity(8192, 262144) == 8192 and lib.stretch_curve_capacity(1, 16384) == 1
    rng = np.random.default_rng(6)
    for F, top in ((37, 100000), (300, 262144), (5, 16384)):
        d = rng.integers(16384, top + 1, F)
        assert cr.time_map(d, F, sr.MAX_FRAMES)[0] <= lib.stretch_curve_capacity(F, top) == cr.time_map(np.full(F, top), F, sr.MAX_FRAMES)[0]


def test_wrappers_refuse_before_the_library(built_lib):
    import torch
    lib = built_lib
    x, i32 = torch.ones(2, 17, 8), torch.int32
    for kw in (dict(dur_q=torch.ones(2, 7, dtype=i32)), dict(dur_q=torch.ones(2, 8)), dict(dur_q=[65536] * 8),
               dict(frames=torch.ones(2, dtype=torch.int64)), dict(frames_per_unit=0), dict(Fo=0), dict(Fo=8193), dict(dur_q_max=5, dur_q=torch.ones(2, 8, dtype=i32)),
               dict(out=torch.ones(2, 17, 9), Fo=8), dict(frames_out=torch.ones(3, dtype=i32)), dict(src=torch.ones(2, 9, dtype=i32), Fo=8)):
        with pytest.raises(ValueError, match='frames_stretch_curve'):
            lib.frames_stretch_curve(x, **kw)
    with pytest.raises(ValueError, match='no CPU fallback'):
        lib.frames_stretch_curve(x, dur_q=torch.full((2, 8), 65536, dtype=i32))
    for kw in (dict(step_q=torch.ones(2, dtype=i32)), dict(step_q=torch.ones(2, 8)), dict(step_q=65536), dict(lifter=9), dict(lifter=0),
               dict(frames_per_unit=0), dict(out=torch.ones(2, 17, 9))):
        with pytest.raises(ValueError, match='frames_pitch_curve'):
            lib.frames_pitch_curve(x, **kw)
    with pytest.raises(ValueError, match='frames_pitch_curve'):
        lib.frames_pitch_curve(torch.ones(2, 18, 8))
    with pytest.raises(ValueError, match='no CPU fallback'):
        lib.frames_pitch_curve(x, step_q=torch.full((2, 8), 65536, dtype=i32), lifter=4)
    path, values = torch.zeros(2, 6, dtype=i32), torch.zeros(2, 4, dtype=i32)
    for a in ((path.long(), values), (path, values[:1]), (path, values.float()), (path, values, 0), (path, values, 1366), (path, values, 1, 2 ** 31),
              (path, values, 1, 0.5)):
        with pytest.raises(ValueError, match='path_curve'):
            lib.path_curve(*a)
    with pytest.raises(ValueError, match='path_curve'):
        lib.path_curve(path, values, curve=torch.zeros(2, 7, dtype=i32))
    with pytest.raises(ValueError, match='no CPU fallback'):
        lib.path_curve(path, values, 2)


# ---- alignment ---------------------------------------------------------------------------------------------------------------------
def test_word_values(built_lib):
    from tacotron_amd.alignment import encoded_chars, word_values
    line = '  Hi,  you #there!\n'                      # 'H' and '#' are not in the vocabulary: dropped before the words are formed
    chars = encoded_chars(line, IVOCAB)
    assert ''.join(chars) == 'i,  you there!'
    vals, n = word_values(line, IVOCAB, {0: 7, 2: 9}, 1)
    assert n == 3 and vals == [7, 7, 1, 1, 1, 1, 1, 1, 9, 9, 9, 9, 9, 9] and len(vals) == len(chars)
    assert word_values(line, IVOCAB, {}, 5) == ([5] * 14, 3)
    assert word_values('\n', IVOCAB, {}, 5) == ([], 0)
    for bad in ({3: 1}, {-1: 1}, {1.5: 1}):
        with pytest.raises(ValueError, match='word_values'):
            word_values(line, IVOCAB, bad, 0)


def test_word_times_through_a_hand_worked_map(built_lib):
    """r = 2, 'ab cd': characters last 1, 2, 1, 0, 2 steps; source frames 0 .. 11.  Every source frame of the first four lasts two output
    frames (d = 131072), the rest one: D = 0, 2, 4, 6, 8, 9, 10, .., so output frame j sits at i = j / 2 for j < 8 and i = j - 4 behind"""
    from tacotron_amd.alignment import step_samples, word_times
    d = np.array([131072] * 4 + [65536] * 8)
    n, i, wq = cr.time_map(d, 12, 64)
    assert n == 16 and i.tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 4, 5, 6, 7, 8, 9, 10, 11] and wq.tolist() == [0, 32768] * 4 + [0] * 8
    src = (i << 16) | wq
    # steps 0, 3, 4, 6 -> source frames 0, 6, 8, 12 -> output frames 0, 10, 12, 16 (12 lies behind the map: Fo_b)
    assert step_samples([0, 3, 4, 6], 2, src=src).tolist() == [0.0, 3000.0, 3600.0, 4800.0]
    assert step_samples(1, 2, src=src) == 1200.0                          # source frame 2 = output frame 4
    rows = word_times('ab cd\n', IVOCAB, [1, 2, 1, 0, 2], 2, src=src, total=300 * 15)
    assert rows == [(0.0, 3000 / 16000.0, 'ab'), (3600 / 16000.0, 4500 / 16000.0, 'cd')]      # the end is clipped to the file's samples
    plain = word_times('ab cd\n', IVOCAB, [1, 2, 1, 0, 2], 2)
    assert plain == [(0.0, 1800 / 16000.0, 'ab'), (2400 / 16000.0, 3600 / 16000.0, 'cd')]     # and without a map nothing changed
    assert word_times('ab cd\n', IVOCAB, [1, 2, 1, 0, 2], 2, src=(np.arange(12) << 16)) == plain   # the identity map
    with pytest.raises(ValueError, match='src'):
        step_samples(1, 2, step_q=65536, src=src)
    with pytest.raises(ValueError, match='src'):
        step_samples(1, 2, src=[0, 65536, -1])


# ---- the driver's option -------------------------------------------------------------------------------------------------------------
def test_prosody_option(built_lib, tmp_path):
    from tacotron_amd import test as drv
    lib = built_lib
    f = tmp_path / 'p.tsv'
    f.write_text('# prompt word rate semitones\n0\t1\t0.5\t-\n\n1\t0\t-\t3\n1\t2\t2\t-2.5\n')
    a = drv.parse_args(['--stop', '--prosody', str(f)])
    assert a.prosody == [(0, 1, 0.5, None), (1, 0, None, 3.0), (1, 2, 2.0, -2.5)] and a.path_jump == lib.PATH_JUMP
    assert drv.parse_args(['--stop', '--prosody', str(f), '--path-jump', '2', '--rate', '0.8', '--pitch', '1', '--timings', '--f0']).path_jump == 2
    assert drv.parse_args([]).prosody is None
    for argv in (['--prosody', str(f)], ['--stop', '--long', '--prosody', str(f)], ['--stop', '--prosody', str(tmp_path / 'missing.tsv')]):
        with pytest.raises(SystemExit):
            drv.parse_args(argv)
    for text in ('0\t1\t0.5\n', '0\t1\t0.5\t-\t7\n', 'x\t1\t0.5\t-\n', '0\t1.5\t0.5\t-\n', '0\t1\tfast\t-\n', '0 1 0.5 -\n'):
        f.write_text(text)
        with pytest.raises(ValueError, match='line 1'):
            drv.parse_prosody(text)
        with pytest.raises(SystemExit):
            drv.parse_args(['--stop', '--prosody', str(f)])
    drv.check_options(stop=True, prosody=[(0, 0, None, None)])
    for kw in (dict(prosody=[]), dict(prosody=[], stop=True, long=True), dict(prosody=[], stop=True, vocode=False)):
        with pytest.raises(ValueError, match='prosody'):
            drv.check_options(**kw)
    prompts = ['hello world.\n', 'a b\n']
    t = drv.prosody_table([(0, 1, 0.5, None), (1, 0, None, 12), (1, 1, 4, -12)], prompts, IVOCAB)
    assert [x.shape for x in t] == [(12, 2), (3, 2)] and all(x.dtype == np.int32 for x in t)
    assert t[0][:, 0].tolist() == [65536] * 6 + [131072] * 6 and (t[0][:, 1] == 65536).all()
    assert t[1].tolist() == [[65536, 32768], [65536, 65536], [16384, 131072]]
    t = drv.prosody_table([(0, 0, None, None), (1, 1, None, 2)], prompts, IVOCAB, [lib.stretch_dur(0.8), 65536], [65536, lib.pitch_step(-1)])
    assert (t[0][:, 0] == 81920).all() and t[1][:, 1].tolist() == [lib.pitch_step(-1)] * 2 + [lib.pitch_step(2)]
    for rows in ([(0, 0, 0.2, None)], [(0, 0, 4.5, None)], [(0, 0, float('nan'), None)], [(0, 0, None, 12.5)], [(0, 2, 1.0, None)],
                 [(1, -1, 1.0, None)], [(2, 0, 1.0, None)], [(-1, 0, 1.0, None)], [(0, 1, 1.0, None), (0, 1, None, 2.0)]):
        with pytest.raises(ValueError, match='prosody'):
            drv.prosody_table(rows, prompts, IVOCAB)
    c = type('Cfg', (), {})()   # the refusals of test() come before the configuration is touched or a device is needed
    with pytest.raises(ValueError, match='prosody'):
        drv.test(c, prompts, prosody=[(0, 0, 1.0, None)])
    with pytest.raises(ValueError, match='prosody'):
        drv.test(c, prompts, prosody=[(0, 0, 1.0, None)], stop=lib.TacoStopRule(), long=True)
    lines = drv.f0_lines('prompt 0', [(10, 7.0, 0.1), (12, 7.01, 0.1), None], prosody=True)
    assert lines == ['prompt 0 prosody: mean log-F0 moved -12.0 cents (10 -> 12 voiced frames)'] and 'asked' not in lines[0]
