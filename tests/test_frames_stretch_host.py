"""CPU: the speaking-rate stretch without a GPU -- properties of the NumPy restatement (tests/stretch_ref.py), the host arithmetic
of tacotron_amd.lib (stretch_step / stretch_frames / stretch_capacity), the header's declaration and constants, and the driver's
--rate option.  No compute calls."""
import os
import re

import numpy as np
import pytest

from tests import stretch_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STEPS = (16384, 65535, 65536, 65537, 77777, 262144)
LENGTHS = (1, 2, 5, 360, 8192)


def _rows(B, C, F, seed=0):
    rng = np.random.default_rng(seed)
    return np.exp(rng.standard_normal((B, C, F)) * 2.0).astype(np.float32)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def test_step_one_is_the_identity():
    x = _rows(3, 4, 11)
    out, n = sr.stretch(x, frames=[11, 7, 0], step_q=[65536] * 3, Fo=14)
    assert n.tolist() == [11, 7, 0]
    assert np.array_equal(out[0, :, :11].view(np.uint32), x[0].view(np.uint32))
    assert np.array_equal(out[1, :, :7].view(np.uint32), x[1, :, :7].view(np.uint32))
    assert not out[0, :, 11:].any() and not out[1, :, 7:].any() and not out[2].any()
    both_null, n2 = sr.stretch(x)
    assert n2.tolist() == [11] * 3 and np.array_equal(both_null.view(np.uint32), x.view(np.uint32))


def test_mixed_batch_frame_counts():
    """the expected frames_out of the GPU suite's mixed batch, by hand: 22 * 4 + 1 = 89 is the capacity; (4 << 16) // 16384 + 1 = 17;
    (12 << 16) // 262144 + 1 = 4; (22 << 16) // 77777 + 1 = 19"""
    frames, steps = (23, 0, 5, 13, 23), (65536, 65536, 16384, 262144, 77777)
    assert [sr.out_frames(sr.row_frames(f, 1, 23), s, 89) for f, s in zip(frames, steps)] == [23, 0, 17, 4, 19]
    assert sr.out_frames(23, 16384) == 89


def test_out_frames_is_monotone_in_the_step():
    for F_b in LENGTHS:
        last = None
        for s in sorted(set(STEPS) | set(range(16384, 262145, 4099))):
            n = sr.out_frames(F_b, s)
            assert n >= 1 and (last is None or n <= last), (F_b, s)
            last = n


@pytest.mark.parametrize('F_b', LENGTHS)
@pytest.mark.parametrize('step', STEPS)
def test_last_output_frame_stays_inside_the_row(F_b, step):
    n = sr.out_frames(F_b, step)
    i, frac = sr.positions(n, step)
    assert int(i[-1]) <= F_b - 1
    at_end = i == F_b - 1
    assert (frac[at_end] == 0).all()                      # on the last source frame only with w == 0: frame F_b is never read
    assert n * sr.clamp_step(step) > (F_b - 1) << 16      # and one more output frame would lie behind it: Fo_b is the largest count
    assert (min(n, sr.MAX_FRAMES) - 1) * sr.clamp_step(step) < 2 ** 31 and (F_b - 1) << 16 < 2 ** 31   # what the kernel forms in 32 bits
    w = frac.astype(np.float32) * np.float32(2.0 ** -16)
    assert np.array_equal(w.astype(np.float64) * 65536.0, frac.astype(np.float64))     # the weight is exact in fp32


def test_nan_behind_the_row_never_reaches_the_output():
    x = _rows(4, 3, 23, seed=1)
    frames, steps = [23, 5, 13, 0], [77777, 16384, 262144, 65536]
    clean, n = sr.stretch(x, frames, steps, Fo=89)
    dirty = x.copy()
    for b, f in enumerate(frames):
        dirty[b, :, f:] = np.nan
    got, n2 = sr.stretch(dirty, frames, steps, Fo=89)
    assert np.isfinite(got).all() and n.tolist() == n2.tolist()
    assert np.array_equal(got.view(np.uint32), clean.view(np.uint32))


def test_the_three_operations_are_rounded_separately():
    """a case where a fused multiply-add gives other bits: the restatement must be the three-operation form"""
    a, c, w = np.float32(1.0), np.float32(1.0 + 2.0 ** -23), np.float32(0.75)
    x = np.array([[[a, c]]], dtype=np.float32)
    out, _ = sr.stretch(x, step_q=[49152], Fo=2)
    want = np.float32(a + np.float32(w * np.float32(c - a)))
    assert out[0, 0, 1] == want
    bound = abs(float(c) - float(a))
    assert abs(float(out[0, 0, 1]) - (float(a) + 0.75 * (float(c) - float(a)))) <= bound


def test_out_of_range_steps_clamp():
    x = _rows(3, 2, 9, seed=2)
    got = sr.stretch(x, step_q=[0, -5, 2 ** 30], Fo=33)
    want = sr.stretch(x, step_q=[16384, 16384, 262144], Fo=33)
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and got[1].tolist() == want[1].tolist() == [33, 33, 3]


# ---- tacotron_amd.lib ----------------------------------------------------------------------------------------------------------------
def test_stretch_step(built_lib):
    lib = built_lib
    assert (lib.STRETCH_ONE, lib.STRETCH_MIN_STEP, lib.STRETCH_MAX_STEP, lib.STRETCH_MAX_FRAMES) == (sr.ONE, sr.MIN_STEP, sr.MAX_STEP,
                                                                                                   sr.MAX_FRAMES)
    assert lib.stretch_step(1.0) == 65536 and lib.stretch_step(0.25) == 16384 and lib.stretch_step(4) == 262144
    assert lib.stretch_step(0.5) == 32768 and lib.stretch_step(1.25) == 81920 and lib.stretch_step(0.8) == 52429
    assert lib.stretch_step(1.0 + 0.4 / 65536) == 65536 and lib.stretch_step(1.0 + 0.6 / 65536) == 65537
    for q in (16384, 52429, 65537, 262144):
        assert lib.stretch_step(q / 65536.0) == q                       # a step survives the way through a rate
    for bad in (0.2499, 4.0001, 0.0, -1.0, float('nan'), float('inf'), None, 'fast'):
        with pytest.raises(ValueError):
            lib.stretch_step(bad)


def test_stretch_frames_and_capacity(built_lib):
    lib = built_lib
    for F_b in (0, -3) + LENGTHS:
        for s in STEPS + (0, -5, 2 ** 30):
            assert lib.stretch_frames(F_b, s) == sr.out_frames(F_b, s)
            assert lib.stretch_frames(F_b, s, cap=7) == sr.out_frames(F_b, s, 7)
    assert lib.stretch_capacity(23, 16384) == 89 and lib.stretch_capacity(360, 32768) == 719 and lib.stretch_capacity(16, 65536) == 16
    x = _rows(1, 2, 37, seed=3)
    for s in STEPS:
        assert sr.stretch(x, step_q=[s])[0].shape[2] == lib.stretch_capacity(37, s)


def test_frames_stretch_refuses_before_the_library(built_lib):
    import torch
    lib = built_lib
    x = torch.ones(2, 3, 8)
    for kw in (dict(step_q=100), dict(step_q=[65536]), dict(step_q=[65536, 300000]), dict(step_q=[65536.5, 65536]),
               dict(frames=torch.ones(2, dtype=torch.int64)), dict(frames_per_unit=0), dict(Fo=0), dict(Fo=8193),
               dict(out=torch.ones(2, 3, 9), Fo=8), dict(frames_out=torch.ones(3, dtype=torch.int32))):
        with pytest.raises(ValueError):
            lib.frames_stretch(x, **kw)
    with pytest.raises(ValueError):
        lib.frames_stretch(x.double())
    with pytest.raises(ValueError):
        lib.frames_stretch(torch.ones(1, 1, 4000), step_q=16384)        # 15997 output frames: more than one call holds
    with pytest.raises(ValueError, match='no CPU fallback'):
        lib.frames_stretch(x, step_q=32768)


# ---- header and binding ------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_point(built_lib):
    import ctypes as C
    hdr = open(os.path.join(ROOT, 'include', 'taco_hip.h')).read()
    for name, value in (('TACO_STRETCH_ONE', 65536), ('TACO_STRETCH_MIN_STEP', 16384), ('TACO_STRETCH_MAX_STEP', 262144),
                        ('TACO_STRETCH_MAX_FRAMES', 8192)):
        m = re.search(r'#define\s+%s\s+(\d+)' % name, hdr)
        assert m and int(m.group(1)) == value, name
    decl = re.search(r'int\s+taco_frames_stretch\s*\(([^)]*)\)\s*;', hdr)
    assert decl, 'include/taco_hip.h does not declare taco_frames_stretch'
    args = [' '.join(a.split()) for a in decl.group(1).split(',')]
    assert args == ['const float* mag_t', 'const int32_t* frames', 'int frames_per_unit', 'const int32_t* step_q', 'float* out',
                    'int32_t* frames_out', 'int B', 'int C', 'int F', 'int Fo', 'void* stream']
    assert hdr.index('taco_denorm_unframe(const float* output') < decl.start() < hdr.index('int taco_corpus_batch(')
    P, I = C.c_void_p, C.c_int
    assert built_lib.EXPORTS['taco_frames_stretch'] == (C.c_int, [P, P, I, P, P, P, I, I, I, I, P])
    assert hasattr(C.CDLL(built_lib.LIB_PATH), 'taco_frames_stretch')


# ---- the driver's option -------------------------------------------------------------------------------------------------------------
def test_rate_option(built_lib):
    from tacotron_amd import test as drv
    assert drv.parse_args([]).rate is None
    assert drv.parse_args(['--rate', '0.8']).rate == 0.8
    assert drv.parse_args(['--rate', '1.25', '--stop', '--vocode-lengths', '--gl-momentum', '0.99', '--deemphasis', '--long']).rate == 1.25
    for bad in ('0.2', '4.5', 'nan', '-1'):
        with pytest.raises(SystemExit):
            drv.parse_args(['--rate', bad])
    drv.check_options()
    drv.check_options(rate=0.25)
    drv.check_options(rate=[0.5, 4.0, 1.0])
    for kw in (dict(rate=0.1), dict(rate=float('nan')), dict(rate=[1.0, 5.0]), dict(rate=1.0, vocode=False)):
        with pytest.raises(ValueError, match='rate'):
            drv.check_options(**kw)
    assert drv.rate_steps(None, 3) is None and drv.rate_steps(0.5, 3) == [32768] * 3 and drv.rate_steps([1.0, 2.0], 2) == [65536, 131072]
    with pytest.raises(ValueError):
        drv.rate_steps([1.0, 2.0], 3)
