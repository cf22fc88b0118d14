"""CPU: the restatements of taco_f0_range_curve (tests/f0_range_ref.py) against their own definition -- the neighbour search against a
brute-force scan, the neutral scale, the flat contour of k = 0, the composition with a base -- the measurement that sizes
F0_RANGE_STEP_ATOL, and the refusals of lib.f0_range_curve, lib.range_scale and the driver's options, none of which needs a GPU."""
import contextlib
import ctypes as C
import io
import os
import re

import numpy as np
import pytest
import torch

from tests import f0_range_cases as rc
from tests import f0_range_ref as rr

CASES = list(rc.all_cases())


def test_the_cases_cover_what_they_claim():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    Fs = {c.period.shape[1] for c in CASES}
    assert set(rc.FS) <= Fs
    assert {c.period.shape[0] for c in CASES} == {1, 2, 3}
    assert {c.smooth for c in CASES} == set(rc.SMOOTHS)
    used = {rr.clamp_scale(q) for c in CASES if c.scale_q is not None for q in c.scale_q}
    assert {rc.q(k) for k in rc.SCALES} <= used
    assert any(c.base_q is None for c in CASES) and any(c.base_q is not None for c in CASES)
    assert any(c.base_q is not None and (c.base_q < rr.MIN_STEP).any() and (c.base_q > rr.MAX_STEP).any() for c in CASES)
    assert any(c.frames is not None and 0 in c.frames for c in CASES)
    assert any(np.isnan(c.period).any() for c in CASES)
    live = np.concatenate([c.period[np.isfinite(c.period) & (c.period > 0)] for c in CASES])
    assert live.min() >= rc.LO and live.max() <= rc.HI       # the tracker's range
    hit = 0
    for c in CASES:   # contours whose excursion hits the limit, on both sides
        if c.base_q is None and c.name.startswith('limit_'):
            step = rr.curve(c.period, c.frames, c.per_unit, c.scale_q, None, c.smooth, c.limit)[0]
            top, bottom = int(round(65536 * 2.0 ** c.limit)), int(round(65536 * 2.0 ** -c.limit))
            assert step.max() == top and step.min() == bottom, c.name
            hit += 1
    assert hit == 3


def test_neighbours_against_the_brute_force():
    rng = np.random.default_rng(0)
    masks = [c.period[b, :rr.row_frames(None if c.frames is None else c.frames[b], c.per_unit, c.period.shape[1])] > 0
             for c in CASES for b in range(c.period.shape[0]) if c.period.shape[1] <= 700]
    masks += [rng.random(n) < p for n in (1, 2, 64, 129, 300) for p in (0.0, 0.02, 0.5, 1.0)]
    masks.append(np.zeros(0, dtype=bool))
    for m in masks:
        got, want = rr.neighbours(m), rr.neighbours_brute(m)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_a_wrong_neighbour_is_thousands_of_steps():
    """the integer search is tested by a bar of a few steps: taking the voiced frame one further away moves the line by far more"""
    c = next(c for c in CASES if c.name == 'gap_70_250_F257')
    p = c.period[:1].copy()
    want = rr.curve(p, None, 1, (rc.q(4.0),), None, 0, 1.0)[0]
    p[0, 251] = 0.0            # the gap's far neighbour becomes frame 252
    moved = rr.curve(p, None, 1, (rc.q(4.0),), None, 0, 1.0)[0]
    assert np.abs(moved[0, 70:251].astype(np.int64) - want[0, 70:251]).max() > 100 * rr.F0_RANGE_STEP_ATOL


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_neutral_scale_copies(dtype):
    for c in CASES:
        B, F = c.period.shape
        step, stats, _ = rr.curve(c.period, c.frames, c.per_unit, (65536,) * B, c.base_q, c.smooth, c.limit, dtype=dtype)
        null = rr.curve(c.period, c.frames, c.per_unit, None, c.base_q, c.smooth, c.limit, dtype=dtype)[0]
        assert np.array_equal(step, null)
        for b in range(B):
            Fb = rr.row_frames(None if c.frames is None else c.frames[b], c.per_unit, F)
            want = np.full(F, rr.ONE) if c.base_q is None else np.clip(c.base_q[b], rr.MIN_STEP, rr.MAX_STEP)
            assert np.array_equal(step[b, :Fb], want[:Fb]) and (step[b, Fb:] == rr.ONE).all()


def test_zero_scale_flattens_the_contour():
    """k = 0 at W = 0 under a limit the contour never reaches: period * step / 65536 is one value over the voiced frames, to the
    rounding of step_q (half a step in at least 32768: 2.2e-5 octaves)"""
    for name in ('F700', 'F65', 'random_F257', 'gap_64_255_F700'):
        c = next(c for c in CASES if c.name == name)
        B = c.period.shape[0]
        step, stats, _ = rr.curve(c.period, c.frames, c.per_unit, (0,) * B, None, 0, 1.0)
        for b, x in enumerate(rr.excursions(c.period, step, c.frames, c.per_unit)):
            if len(x):
                assert np.abs(x - stats[b, 1]).max() <= 2.3e-5, name
    # and k scales the deviation: 1.5 at W = 0 widens it by 1.5
    c = next(c for c in CASES if c.name == 'F700')
    step, stats, _ = rr.curve(c.period[:1], None, 1, (rc.q(1.5),), None, 0, 1.0)
    x = rr.excursions(c.period[:1], step)[0]
    assert abs(x.std() / stats[0, 2] - 1.5) < 1e-3 and abs(x.mean() - stats[0, 1]) < 1e-4


def test_a_base_adds_its_shift():
    """with a base the excursion is the sum of the two shifts: the unrounded step is the one without a base times clamp(base) / 65536,
    wherever neither is clamped"""
    n = 0
    for c in CASES:
        if c.base_q is None:
            continue
        _, _, with_base = rr.curve(c.period, c.frames, c.per_unit, c.scale_q, c.base_q, c.smooth, c.limit)
        _, _, alone = rr.curve(c.period, c.frames, c.per_unit, c.scale_q, None, c.smooth, c.limit)
        want = alone * np.clip(c.base_q.astype(np.float64), rr.MIN_STEP, rr.MAX_STEP) / 65536.0
        B, F = c.period.shape
        for b in range(B):
            Fb = rr.row_frames(None if c.frames is None else c.frames[b], c.per_unit, F)
            free = (want[b, :Fb] > rr.MIN_STEP) & (want[b, :Fb] < rr.MAX_STEP)
            assert np.allclose(with_base[b, :Fb][free], want[b, :Fb][free], rtol=1e-12, atol=0)
            n += int(free.sum())
    assert n > 10000


def test_the_bar_is_the_measured_float32_error():
    """the measurement behind F0_RANGE_STEP_ATOL, repeated: the float32 restatement against the float64 one over every case, in front
    of the final rintf; the constant is that value rounded up, and the bar 1 + 2 x it"""
    worst, at = 0.0, None
    for c in CASES:
        a = rr.curve(c.period, c.frames, c.per_unit, c.scale_q, c.base_q, c.smooth, c.limit)
        b = rr.curve(c.period, c.frames, c.per_unit, c.scale_q, c.base_q, c.smooth, c.limit, dtype=np.float32)
        assert b[2].dtype == np.float32 and b[1].dtype == np.float32
        assert np.array_equal(a[1][:, 0], b[1][:, 0])
        err = rc.step_err(b[2], a[2])
        assert rc.step_err(b[0], a[0]) <= 1.0 + err
        if err > worst:
            worst, at = err, c.name
    print('  worst |float32 - float64| in front of rintf: %.4f steps (%s); constant %.2f, bar %.2f'
          % (worst, at, rr.MEASURED_FLOAT32_STEP_ERROR, rr.F0_RANGE_STEP_ATOL))
    assert worst <= rr.MEASURED_FLOAT32_STEP_ERROR <= 1.05 * worst + 0.01
    assert rr.F0_RANGE_STEP_ATOL == 1.0 + 2.0 * rr.MEASURED_FLOAT32_STEP_ERROR


def test_range_scale(built_lib):
    lib = built_lib
    assert [lib.range_scale(k) for k in (0, 0.5, 1, 1.5, 4)] == [0, 32768, 65536, 98304, 262144]
    for bad in (-0.01, 4.01, float('nan'), float('inf'), None, 'wide', True):
        with pytest.raises(ValueError, match=r'\[0, 4\]'):
            lib.range_scale(bad)
    assert (lib.F0_RANGE_SMOOTH, lib.F0_RANGE_LIMIT, lib.F0_RANGE_MAX_SMOOTH) == (rr.SMOOTH, rr.LIMIT, rr.MAX_SMOOTH)


def test_f0_range_curve_refuses_before_the_library(built_lib):
    """every refusal of the wrapper names the argument, and comes before the device check: these tensors are on the CPU"""
    lib = built_lib
    p = torch.full((2, 6), 100.0)
    i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32)   # noqa: E731
    bad = [(dict(period=p.double()), 'period'), (dict(period=p[0]), 'period'), (dict(period=p[:, ::2]), 'period'),
           (dict(period=torch.zeros(1, 8193)), 'frames'), (dict(frames=i32(3)), 'frames'), (dict(frames=torch.zeros(2)), 'frames'),
           (dict(frames_per_unit=0), 'frames_per_unit'), (dict(frames_per_unit=1.5), 'frames_per_unit'),
           (dict(scale_q=[1, 2, 3]), 'scale_q'), (dict(scale_q=-1), 'scale_q'), (dict(scale_q=[0, 262145]), 'scale_q'),
           (dict(scale_q=0.5), 'scale_q'), (dict(base_q=i32(2, 5)), 'base_q'), (dict(base_q=torch.zeros(2, 6)), 'base_q'),
           (dict(smooth=-1), 'smooth'), (dict(smooth=9), 'smooth'), (dict(smooth=1.5), 'smooth'),
           (dict(limit=0.0), 'limit'), (dict(limit=-0.1), 'limit'), (dict(limit=1.01), 'limit'), (dict(limit=float('nan')), 'limit'),
           (dict(limit=None), 'limit'), (dict(out=i32(2, 5)), 'step_q'), (dict(out=torch.zeros(2, 6)), 'step_q'),
           (dict(out=i32(2, 6), want_stats=True), 'out'), (dict(out=(i32(2, 6), torch.zeros(2, 4)), want_stats=True), 'stats'),
           (dict(out=p.view(torch.int32)), 'overlap')]
    for kw, word in bad:
        args = dict(period=p)
        args.update(kw)
        with pytest.raises(ValueError, match=r'^f0_range_curve: ') as e:
            lib.f0_range_curve(**args)
        assert word in str(e.value), (kw, str(e.value))
    base = i32(2, 6)
    with pytest.raises(ValueError, match='step_q may not overlap base_q'):
        lib.f0_range_curve(p, base_q=base, out=base)
    with pytest.raises(ValueError, match='must be on the GPU'):   # the last check: everything else was in order
        lib.f0_range_curve(p, i32(2), 3, [0, 98304], base, 8, 1.0, want_stats=True)


def test_header_declares_the_entry_point(built_lib):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'include', 'taco_hip.h')) as f:
        text = f.read()
    assert re.search(r'int taco_f0_range_curve\(const float\* period, const int32_t\* frames, int frames_per_unit, const int32_t\* scale_q,\s+'
                     r'const int32_t\* base_q,\s+int smooth, float limit, int32_t\* step_q, float\* stats, int B, int F, void\* stream\);', text)
    assert '#define TACO_VERSION 120' in text and '#define TACO_F0_RANGE_MAX_SMOOTH 8' in text
    P, I = C.c_void_p, C.c_int
    assert built_lib.EXPORTS['taco_f0_range_curve'] == (C.c_int, [P, P, I, P, P, I, C.c_float, P, P, I, I, P])
    assert hasattr(C.CDLL(built_lib.LIB_PATH), 'taco_f0_range_curve')
    with open(os.path.join(root, 'tacotron_amd', 'csrc', 'UNITS')) as f:
        assert 'f0_curve' in f.read().split()


def test_driver_options(built_lib):
    """--pitch-range and its two settings: ranges, what needs what, 1 the run without it, and the line --f0 prints"""
    from tacotron_amd import test as drv
    assert drv.pitch_range_options(None) is None and drv.pitch_range_options(1.0) is None and drv.pitch_range_options(1) is None
    assert drv.pitch_range_options(1.5) == (98304, rr.SMOOTH, rr.LIMIT)
    assert drv.pitch_range_options(0, 8, 1.0) == (0, 8, 1.0)
    for args in ((-0.5,), (4.5,), (float('nan'),), (True,), (1.5, 9), (1.5, -1), (1.5, 2, 0.0), (1.5, 2, 1.5), (1.5, 2, float('nan'))):
        with pytest.raises(ValueError, match='pitch.range'):
            drv.pitch_range_options(*args)
    with pytest.raises(ValueError, match='needs vocode'):
        drv.pitch_range_options(1.5, vocode=False)
    a = drv.parse_args(['--pitch-range', '1.5'])
    assert (a.pitch_range, a.pitch_range_smooth, a.pitch_range_limit) == (1.5, rr.SMOOTH, rr.LIMIT)
    a = drv.parse_args(['--pitch-range', '0', '--pitch-range-smooth', '0', '--pitch-range-limit', '1', '--pitch', '2', '--f0', '--rate', '0.8'])
    assert (a.pitch_range, a.pitch_range_smooth, a.pitch_range_limit) == (0.0, 0, 1.0)
    assert drv.parse_args([]).pitch_range is None
    for argv in (['--pitch-range', '5'], ['--pitch-range-smooth', '2'], ['--pitch-range-limit', '0.5'], ['--pitch-range', '1.5', '--pitch-range-smooth', '9'],
                 ['--pitch-range', '1.5', '--pitch-range-limit', '0']):
        with pytest.raises(SystemExit):
            drv.parse_args(argv)
    opt = drv.Options().resolved(pitch_range=1.5, pitch_range_smooth=3)
    assert opt.pitch_range == (98304, 3, rr.LIMIT) and drv.Options().resolved().pitch_range is None
    line = drv.range_line('prompt 3', (98304, np.array([212.0, 2.1 / 12.0, 3.1 / 12.0, 1.46], dtype=np.float32)))
    assert line == 'prompt 3 range asked x1.50, measured x1.46 (2.1 -> 3.1 semitones) over 212 voiced frames'
    buf = io.StringIO()   # the help text says what nobody has done
    with contextlib.redirect_stdout(buf), pytest.raises(SystemExit):
        drv.parse_args(['--help'])
    helped = ' '.join(buf.getvalue().split())
    assert 'untuned' in helped and 'nobody has listened' in helped and 'on an untrained model' in helped and '--pitch-range K' in helped
