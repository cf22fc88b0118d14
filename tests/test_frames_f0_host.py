"""CPU: the F0 tracker without a GPU -- what the float64 restatement (tests/f0_ref.py) measures on harmonic combs and on the pitch
shift's own output, the exact rules of the pick, the measurements that size F0_ACF_ATOL and F0_STATS_ATOL, the tables and the argument
checks of tacotron_amd.lib, the header's declarations, and the --f0 options of the driver and of evaluate.  No compute calls."""
import os
import re

import numpy as np
import pytest

from tests import f0_cases as fc
from tests import f0_ref as fr
from tests import pitch_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


# ---- the method, in float64 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('spacing', [8, 12.8, 19.3, 25.6])
def test_comb_period(built_lib, spacing):
    """harmonics every `spacing` bins at C = 1025 are a period of 2048 / spacing samples: within 0.05 samples without tables, within
    0.15 with the production tables (measured here: at most 0.018 and 0.066)"""
    mag = pr.comb(1025, 4, spacing=spacing)[0][None]
    w, g, lo, hi = built_lib.f0_tables()
    plain, s0 = fr.track(mag, lag_min=lo, lag_max=hi)
    table, s1 = fr.track(mag, weight=w, gain=g, lag_min=lo, lag_max=hi)
    want = 2048.0 / spacing
    print('  spacing %.1f: wanted %.3f, plain %s, with tables %s' % (spacing, want, plain[0], table[0]))
    assert np.abs(plain - want).max() <= 0.05 and np.abs(table - want).max() <= 0.15
    assert min(s0.min(), s1.min()) > 0.5


@pytest.mark.parametrize('semitones', [4, -5])
def test_shift_is_measured(built_lib, semitones):
    """the float64 pitch shift of the 100 Hz comb, tracked before and behind, through the paired statistic: within 0.05 semitones of what
    the step asks for, with and without the tables (measured here: 0.0002 and 0.0005 at +4, 0.0013 and 0.0011 at -5)"""
    mag = pr.comb(1025, 24)[0][None]
    step = pr.pitch_step(semitones)
    moved = pr.shift(mag, None, [step]).astype(f32)
    asked = 12.0 * np.log2(65536.0 / step)
    w, g, lo, hi = built_lib.f0_tables()
    for kw in ({}, dict(weight=w, gain=g)):
        before = fr.track(mag, lag_min=lo, lag_max=hi, **kw)[0].astype(f32)
        behind = fr.track(moved, lag_min=lo, lag_max=hi, **kw)[0].astype(f32)
        count, mean, sd = fr.stats(behind, before)[0]
        print('  asked %+.4f, measured %+.4f semitones over %d frames (deviation %.4f)%s'
              % (asked, 12.0 * mean, count, 12.0 * sd, ' with tables' if kw else ''))
        assert count == 24 and abs(12.0 * mean - asked) <= 0.05


def test_unvoiced_frames_are_zeros():
    """an all-zero frame, a frame of 1e-30 (its float32 square is 0) and a frame without an interior local maximum: period, strength
    +0, and the first two an acf column of +0; the comb next to them is voiced"""
    c = next(c for c in fc.all_cases() if c.name == 'silent')
    for dtype in (np.float64, f32):
        y = fr.acf(c.x, None, 1, None, None, c.lag_min, c.lag_max, dtype=dtype)
        assert not y[:2].any() and y[2].any() and (np.diff(y[2], axis=0) < 0).all()
    y = fr.acf(c.x, None, 1, None, None, c.lag_min, c.lag_max, dtype=f32)
    period, strength = fr.pick(y, c.lag_min, c.ratio, c.threshold)
    assert not period[:3].view(np.uint32).any() and not strength[:3].view(np.uint32).any()
    assert (period[3] > 0).all()
    p64, s64 = fr.track(c.x, None, 1, None, None, c.lag_min, c.lag_max, c.ratio, c.threshold)
    assert not p64[:3].any() and not s64[:3].any()


def column(*y):
    return np.array(y, dtype=f32)[:, None]


def test_pick_ties():
    """y[n] == y[n+1] makes n the candidate and n + 1 none; of two candidates at exactly ratio * g the smaller lag wins; a candidate
    one ulp below ratio * g does not count"""
    p, s = fr.pick(column(0.1, 0.5, 0.5, 0.2, 0.1), 10, 1.0, 0.0)          # rows are lags 9 .. 13
    assert p[0] == f32(10) + f32(0.5) and s[0] == f32(0.5)                # a = -0.1, d = -0.4 - (-0.1) ... clamped to +0.5
    g = f32(0.8)
    bar = f32(0.5) * g
    y = column(0.0, bar, 0.1, g, 0.1, bar, 0.0)                            # candidates at lags 10 (ratio * g), 12 (g), 14 (ratio * g)
    p, s = fr.pick(y, 10, 0.5, 0.0)
    assert int(np.rint(p[0])) == 10 and s[0] == bar
    y[1, 0] = np.nextafter(bar, f32(0))
    p, s = fr.pick(y, 10, 0.5, 0.0)
    assert int(np.rint(p[0])) == 12 and s[0] == g
    p, s = fr.pick(y, 10, 1.0, 0.9)                                        # the pick is below the threshold: unvoiced
    assert p[0] == 0 and s[0] == 0
    p, s = fr.pick(column(0.3, 0.2, 0.1, 0.1, 0.05), 10, 0.9, 0.0)         # falling, with an equal pair: no y[n] > y[n-1]
    assert p[0] == 0 and s[0] == 0


def test_pick_is_the_headers_arithmetic():
    """the vectorised pick against the header's rules spelled out lag by lag, one float32 operation at a time"""
    rng = np.random.default_rng(0)
    y = rng.standard_normal((2, 40, 7)).astype(f32)
    p, s = fr.pick(y, 5, 0.7, -10.0)
    for b in range(2):
        for f in range(7):
            col = y[b, :, f]
            cand = [i for i in range(1, 39) if col[i] > col[i - 1] and col[i] >= col[i + 1]]
            g = max(col[i] for i in cand)
            i = next(i for i in cand if col[i] >= f32(0.7) * g)
            d = (col[i - 1] - (col[i] + col[i])) + col[i + 1]
            delta = f32(0) if d == 0 else min(max((f32(0.5) * (col[i - 1] - col[i + 1])) / d, f32(-0.5)), f32(0.5))
            assert p[b, f] == f32(4 + i) + delta and s[b, f] == col[i]


def test_pick_d_zero():
    """a candidate whose parabola is flat after rounding: ym = 1 - 2^-24 ... built so that (ym - t) + yp == 0 with y0 > ym, y0 >= yp"""
    y0 = f32(1.0)
    ym = np.nextafter(y0, f32(0))                    # 1 - 2^-24
    yp = y0                                          # a plateau: ym < y0 == yp; t = 2; ym - 2 = -(1 + 2^-24) rounds to -1; + 1 = 0
    assert y0 > ym and y0 >= yp and (ym - (y0 + y0)) + yp == 0
    p, s = fr.pick(column(0.0, ym, y0, yp, 0.0), 20, 1.0, 0.0)   # rows are lags 19 .. 23: the candidate is lag 21
    assert p[0] == f32(21) and s[0] == y0


# ---- the tolerances --------------------------------------------------------------------------------------------------------------------
def test_case_list_covers_the_kernel():
    cases = list(fc.all_cases())
    assert {c.x.shape[1] for c in cases} >= {17, 33, 129, 1025}
    assert {c.lag_max - c.lag_min + 3 for c in cases} >= {3, 32, 33, 64, 65, 229, 512}
    for C, lo, hi in fc.SMALL:
        assert {c.x.shape[2] for c in cases if c.name.startswith('small_C%d_%d_%d_' % (C, lo, hi))} == set(fc.EDGE_F)
    mixed = cases[0]
    assert mixed.x.shape == (5, 1025, 23) and 0 in mixed.frames and mixed.weight is not None and mixed.gain is not None
    assert any(c.weight is None and c.gain is None for c in cases) and {c.per_unit for c in cases} >= {2, 3, 5, 1000}
    assert any(c.frames is not None and max(c.frames) * c.per_unit > 2 ** 31 for c in cases)
    assert all(np.isnan(c.x[b, :, fr.row_frames(n, c.per_unit, c.x.shape[2]):]).all() for c in cases[:10] for b, n in enumerate(c.frames))


def test_acf_atol_is_four_times_the_float32_error():
    """F0_ACF_ATOL comes from the restatements alone: the float32 form against the float64 one on every input of the GPU tests"""
    worst, where = 0.0, None
    for c in fc.all_cases():
        args = (c.x, c.frames, c.per_unit, c.weight, c.gain, c.lag_min, c.lag_max)
        e = fc.acf_err(fr.acf(*args, dtype=f32), fr.acf(*args))
        if e > worst:
            worst, where = e, c.name
    print('  largest float32 error %.3g on %s; F0_ACF_ATOL %.3g' % (worst, where, fr.F0_ACF_ATOL))
    assert fr.F0_ACF_ATOL == 4.0 * fr.MEASURED_FLOAT32_ACF_ERROR
    assert 0.8 * fr.MEASURED_FLOAT32_ACF_ERROR <= worst <= fr.MEASURED_FLOAT32_ACF_ERROR


def test_stats_atol_is_four_times_the_float32_error():
    worst, where = 0.0, None
    for c in fc.stats_cases():
        e = fc.stats_err(fr.stats(c.period, c.other, c.frames, c.per_unit, dtype=f32), fr.stats(c.period, c.other, c.frames, c.per_unit))
        if e > worst:
            worst, where = e, c.name
    print('  largest float32 error %.3g on %s; F0_STATS_ATOL %.3g' % (worst, where, fr.F0_STATS_ATOL))
    assert fr.F0_STATS_ATOL == 4.0 * fr.MEASURED_FLOAT32_STATS_ERROR
    assert 0.8 * fr.MEASURED_FLOAT32_STATS_ERROR <= worst <= fr.MEASURED_FLOAT32_STATS_ERROR
    counts = fr.stats(*next(c for c in fc.stats_cases() if c.name == 'paired')[1:])[:, 0]
    assert counts[0] == 0 and counts[1] == 1 and counts[2] > 256 and 0 < counts[3] < 411


def test_stats_restatement():
    p = np.array([[100.0, 0.0, 50.0, 200.0, np.nan]], dtype=f32)
    o = np.array([[200.0, 80.0, 0.0, 200.0, 1.0]], dtype=f32)
    x = np.log2([100.0, 50.0, 200.0])
    assert np.allclose(fr.stats(p, None, [4])[0], [3, x.mean(), x.std()], rtol=1e-12)
    assert np.allclose(fr.stats(p, o, [4])[0], [2, 0.5, 0.5], rtol=1e-12)             # an octave up and no change
    assert not fr.stats(p, o, [0]).any() and fr.stats(p[:, :2], o[:, :2])[0].tolist() == [1.0, 1.0, 0.0]


# ---- tacotron_amd.lib ------------------------------------------------------------------------------------------------------------------
def test_f0_tables(built_lib):
    """against the direct sums of tests/f0_ref.tables: the window's autocorrelation as products, the weight as |1 - a e^{-i w}|^-2"""
    lib = built_lib
    for kw in ({}, dict(sr=16000, fmin=80.0, fmax=300.0, deemphasis=0.0, C=513, win_length=800), dict(deemphasis=0.5, win_length=2048)):
        w, g, lo, hi = lib.f0_tables(**kw)
        w2, g2, lo2, hi2 = fr.tables(**kw)
        assert (lo, hi) == (lo2, hi2) and w.dtype == g.dtype == np.float32 and w.shape == (kw.get('C', 1025),) and g.shape == (hi - lo + 3,)
        assert np.abs(w / w2 - 1.0).max() < 1e-6 and np.abs(g / g2 - 1.0).max() < 1e-6
        if kw.get('deemphasis') == 0.0:
            assert (w == 1.0).all()
    w, g, lo, hi = lib.f0_tables()
    assert (lo, hi, len(g)) == (40, 266, 229) and (g > 1.0).all() and (np.diff(g) > 0).all() and abs(w[0] - 1.0 / 0.03 ** 2) < 0.01
    assert (lib.F0_MAX_LAGS, lib.F0_RATIO, lib.F0_THRESHOLD) == (fr.MAX_LAGS, fr.RATIO, fr.THRESHOLD)
    for bad in (dict(fmin=20.0), dict(fmin=500.0), dict(fmax=9000.0), dict(C=1000), dict(deemphasis=1.0), dict(win_length=200),
                dict(win_length=4096), dict(sr=0)):
        with pytest.raises(ValueError):
            lib.f0_tables(**bad)


def test_frames_f0_refuses_before_the_library(built_lib):
    import torch
    lib = built_lib
    x = torch.ones(2, 17, 8)
    ok = dict(lag_min=3, lag_max=10)
    for kw in (dict(lag_min=1), dict(lag_max=16), dict(lag_min=11), dict(lag_min=2.5), dict(ratio=0.0), dict(ratio=1.5),
               dict(ratio=float('nan')), dict(threshold=float('nan')), dict(frames=torch.ones(2, dtype=torch.int64)),
               dict(frames_per_unit=0), dict(weight=np.ones(16)), dict(gain=np.ones(9)), dict(weight=torch.ones(17, dtype=torch.float64)),
               dict(out=(torch.ones(2, 8),)), dict(out=(torch.ones(2, 8), torch.ones(2, 9))), dict(out=(x[:, 0], torch.ones(2, 8))),
               dict(want_acf=True, out=(torch.ones(2, 8), torch.ones(2, 8), torch.ones(2, 9, 8)))):
        with pytest.raises(ValueError):
            lib.frames_f0(x, **dict(ok, **kw))
    with pytest.raises(ValueError):
        lib.frames_f0(x)                                                 # the default lags 40 .. 266 need C >= 269
    with pytest.raises(ValueError):
        lib.frames_f0(torch.ones(1, 1025, 4), lag_min=40, lag_max=600)   # more than 512 lags
    for bad in (x.double(), torch.ones(2, 16, 8), torch.ones(2, 2049, 8), torch.ones(2, 5, 8), torch.ones(17, 8)):
        with pytest.raises(ValueError):
            lib.frames_f0(bad, **ok)
    with pytest.raises(ValueError, match='no CPU fallback'):
        lib.frames_f0(x, weight=np.ones(17), gain=np.ones(10), **ok)
    p = torch.ones(2, 8)
    for kw in (dict(other=torch.ones(2, 9)), dict(other=p.double()), dict(frames=torch.ones(3, dtype=torch.int32)), dict(frames_per_unit=0),
               dict(out=torch.ones(2, 2))):
        with pytest.raises(ValueError):
            lib.f0_stats(p, **kw)
    for bad in (p.double(), torch.ones(8), torch.ones(1, 8193)):
        with pytest.raises(ValueError):
            lib.f0_stats(bad)
    with pytest.raises(ValueError, match='no CPU fallback'):
        lib.f0_stats(p, other=p)


# ---- header and binding ----------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points(built_lib):
    import ctypes as C
    hdr = open(os.path.join(ROOT, 'include', 'taco_hip.h')).read()
    m = re.search(r'#define\s+TACO_F0_MAX_LAGS\s+(\d+)', hdr)
    assert m and int(m.group(1)) == fr.MAX_LAGS
    decl = re.search(r'int\s+taco_frames_f0\s*\(([^)]*)\)\s*;', hdr)
    assert decl, 'include/taco_hip.h does not declare taco_frames_f0'
    assert [' '.join(a.split()) for a in decl.group(1).split(',')] == [
        'const float* mag_t', 'const int32_t* frames', 'int frames_per_unit', 'const float* weight', 'const float* gain', 'int lag_min',
        'int lag_max', 'float ratio', 'float threshold', 'float* period', 'float* strength', 'float* acf', 'int B', 'int C', 'int F',
        'void* stream']
    stats = re.search(r'int\s+taco_f0_stats\s*\(([^)]*)\)\s*;', hdr)
    assert stats and [' '.join(a.split()) for a in stats.group(1).split(',')] == [
        'const float* period', 'const float* other', 'const int32_t* frames', 'int frames_per_unit', 'float* stats', 'int B', 'int F',
        'void* stream']
    assert hdr.index('int taco_frames_pitch(') < decl.start() < stats.start() < hdr.index('int taco_corpus_batch(')
    assert int(re.search(r'#define\s+TACO_VERSION\s+(\d+)', hdr).group(1)) == 120
    P, I, Fl = C.c_void_p, C.c_int, C.c_float
    assert built_lib.EXPORTS['taco_frames_f0'] == (C.c_int, [P, P, I, P, P, I, I, Fl, Fl, P, P, P, I, I, I, P])
    assert built_lib.EXPORTS['taco_f0_stats'] == (C.c_int, [P, P, P, I, P, I, I, P])
    so = C.CDLL(built_lib.LIB_PATH)
    assert hasattr(so, 'taco_frames_f0') and hasattr(so, 'taco_f0_stats')


# ---- the driver's and evaluate's options -------------------------------------------------------------------------------------------------
def test_f0_option(built_lib):
    from tacotron_amd import test as drv
    assert drv.parse_args([]).f0 is None
    assert drv.parse_args(['--f0']).f0 is True and drv.parse_args(['--f0', '--f0-range', '80,300']).f0 == (80.0, 300.0)
    a = drv.parse_args(['--f0', '--pitch', '3', '--rate', '0.9', '--stop', '--vocode-lengths', '--gl-momentum', '0.99', '--deemphasis',
                        '--long', '--align-scores'])
    assert a.f0 is True and (a.pitch, a.rate) == (3.0, 0.9)
    for bad in (['--f0-range', '80,300'], ['--f0', '--f0-range', '80'], ['--f0', '--f0-range', '10,400'], ['--f0', '--f0-range', '300,80']):
        with pytest.raises(SystemExit):
            drv.parse_args(bad)
    drv.check_options()
    drv.check_options(f0=True, pitch=2.0, rate=0.8)
    drv.check_options(f0=(70.0, 350.0))
    with pytest.raises(ValueError, match='f0'):
        drv.check_options(f0=True, vocode=False)
    with pytest.raises(ValueError, match='f0'):
        drv.check_options(f0=(5.0, 400.0))
    assert drv.f0_range(None) is None and drv.f0_range(True) == (60.0, 400.0)
    up = drv.f0_lines('prompt 7', ([30, 7.0, 0.1], [31, 6.75, 0.1], [28, 0.25, 0.01]), asked_step=built_lib.pitch_step(3))
    assert up == ['prompt 7 pitch: asked +3.00, measured +3.00 semitones over 28 voiced frames']
    slow = drv.f0_lines('prompt 7', ([30, 7.0, 0.1], [40, 7.01, 0.1], None), rate_step=built_lib.stretch_step(0.8))
    assert slow == ['prompt 7 rate 0.800: mean log-F0 moved -12.0 cents (30 -> 40 voiced frames)']
    assert drv.f0_lines('prompt 7 piece 2', ([30, 7.0, 0.1], [30, 7.0, 0.1], None)) == []


def test_f0_option_leaves_a_plain_run_alone(tmp_path):
    """write_prompt without f0 writes no _f0.npy; with it, the rows as float32"""
    from tacotron_amd import test as drv
    spec, align = np.zeros((8, 1025), dtype=f32), np.zeros((4, 10), dtype=f32)
    drv.write_prompt(str(tmp_path), 0, 2, spec, align)
    assert sorted(os.listdir(tmp_path)) == ['prompt_000_align.npy', 'prompt_000_spec.npy']
    drv.write_prompt(str(tmp_path), 1, 2, spec, align, f0=np.array([[160.0, 0.8], [0.0, 0.0]]))
    got = np.load(os.path.join(tmp_path, 'prompt_001_f0.npy'))
    assert got.dtype == np.float32 and got.tolist() == [[160.0, f32(0.8)], [0.0, 0.0]]


def test_evaluate_columns(built_lib):
    from tacotron_amd import evaluate as ev
    assert ev.COLUMNS == ('index', 'na', 'nb', 'steps', 'cost', 'mcd') and len(ev.F0_COLUMNS) == 6
    assert ev.parse_args([]).f0 is False and ev.parse_args(['--f0']).f0 is True
    rows = ev.mcd_rows([5, 6, 7], [20, 0, 10], [10, 6, 4], [25, 0, 11], [50.0, 0.0, 22.0])
    assert rows.shape == (3, 6)
    stats = [[10, 7.0, 0.1], [0, 0.0, 0.0], [0, 0.0, 0.0]]            # log2(period): 128 samples = 125 Hz
    rec = [[5, 6.0, 0.2], [3, 6.5, 0.1], [4, 7.0, 0.0]]
    full = ev.f0_rows(rows, stats, rows[:, 1], rec, rows[:, 2])
    assert full.shape == (3, 12) and np.array_equal(full[:, :6], rows, equal_nan=True)
    assert np.allclose(full[0, 6:], [np.log2(125.0), 0.1, 0.5, np.log2(250.0), 0.2, 0.5])
    assert np.isnan(full[1, 6:9]).all() and np.isnan(full[2, 6:8]).all() and full[2, 8] == 0.0
    assert np.allclose(full[1:, 9:], [[np.log2(16000.0) - 6.5, 0.1, 0.5], [np.log2(125.0), 0.0, 1.0]])
    cents, share = ev.f0_summary(full[:, 6:])
    assert abs(cents + 1200.0) < 1e-9 and abs(share - (0.0 - 1.0) / 2) < 1e-12   # one utterance has both levels; two have both shares
    assert all(np.isnan(v) for v in ev.f0_summary(np.full((2, 6), np.nan)))
