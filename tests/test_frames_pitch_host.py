"""CPU: the pitch shift without a GPU -- what the float64 restatement (tests/pitch_ref.py) does to a harmonic comb, the measurement
that sizes PITCH_RTOL, the reference chain of the acoustic check, the host arithmetic of tacotron_amd.lib, the header's declaration and
constants, and the driver's --pitch / --lifter options.  No compute calls."""
import os
import re

import numpy as np
import pytest

from tests import pitch_cases as pc
from tests import pitch_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def test_envelope_is_the_liftered_fft_form():
    """steps 2 and 3 of the definition equal ifft of the even extension, |n| > Q zeroed, fft"""
    m = pr.comb(129, 3, spacing=9.3)[0].astype(np.float64)
    for Q in (1, 7, 32, 64):
        L, E = pr.log_envelope(m, Q)
        c = np.fft.ifft(np.concatenate([L, L[-2:0:-1]], axis=0), axis=0)
        c[Q + 1:-Q] = 0.0
        assert np.abs(np.fft.fft(c, axis=0).real[:129] - E).max() < 1e-12


@pytest.mark.parametrize('semitones', [4, -5])
def test_comb_moves_and_envelope_stays(semitones):
    """a comb of 12.8 bins under a smooth envelope of spread 1.0, Q = 32: the peak spacing follows 65536 / step_q within 2 %, and the
    log-envelope estimated again from the output stays within 0.2 rms of the input's (measured here: 0.002 and 0.003)"""
    mag, env = pr.comb()
    assert abs(env.std() - 1.0) < 1e-3 and abs(pr.peak_spacing(mag[:, 0], 30, 900) - 12.8) < 0.05
    step = pr.pitch_step(semitones)
    out = pr.shift_frames(mag, step, 32)
    want = 12.8 * 65536.0 / step
    got = pr.peak_spacing(out[:, 0], 30, 900)
    print('  %+d semitones: step %d, peak spacing %.3f, wanted %.3f' % (semitones, step, got, want))
    assert abs(got / want - 1.0) < 0.02
    rms = float(np.sqrt(((pr.log_envelope(out, 32)[1] - pr.log_envelope(mag, 32)[1]) ** 2).mean()))
    print('  re-estimated log-envelope: %.4f rms from the original' % rms)
    assert rms < 0.2
    assert np.abs(np.log(out[:, 0]) - np.log(mag[:, 0])).max() > 1.0          # (and the frame did change)


def test_step_one_is_the_identity():
    x = pc.mags(3, 17, 11, seed=1, zeros=0.2)
    out = pr.shift(x, frames=[11, 7, 0], step_q=[65536] * 3, lifter=8)
    assert np.array_equal(out[0], x[0]) and np.array_equal(out[1, :, :7], x[1, :, :7])
    assert not out[1, :, 7:].any() and not out[2].any()
    assert np.array_equal(pr.shift(x, lifter=8, dtype=np.float32).view(np.uint32), x.view(np.uint32))
    # and the definition itself at step 65536 is the identity up to rounding: R' = R, out = exp(L) (zeros come back as the floor)
    again = pr.shift_frames(x[0], 65536, 8)
    assert np.allclose(again, np.maximum(x[0], 1e-8), rtol=1e-12)


def test_nan_behind_the_row_never_reaches_the_output():
    x, frames, steps, r, Q = next(c[1:] for c in pc.all_cases() if c[0] == 'small_C33_Q16_F33')
    assert np.isnan(x[0, :, frames[0]:]).all()
    assert np.isfinite(pr.shift(x, frames, steps, r, Q)).all()


def test_rtol_is_four_times_the_float32_error():
    """PITCH_RTOL comes from the restatements alone: the float32 form against the float64 one on every input of the GPU tests"""
    worst, where = 0.0, None
    for name, x, frames, steps, r, Q in pc.all_cases():
        e = pc.rel_err(pr.shift(x, frames, steps, r, Q, dtype=np.float32), pr.shift(x, frames, steps, r, Q))
        if e > worst:
            worst, where = e, name
    print('  largest float32 error %.3g on %s; PITCH_RTOL %.3g' % (worst, where, pr.PITCH_RTOL))
    assert pr.PITCH_RTOL == 4.0 * pr.MEASURED_FLOAT32_ERROR
    # (NumPy's float32 log and exp differ in the last bit between CPUs and builds: the recorded figure is held to a fifth)
    assert 0.8 * pr.MEASURED_FLOAT32_ERROR <= worst <= 1.2 * pr.MEASURED_FLOAT32_ERROR


def test_reference_chain_of_the_acoustic_check():
    """the comb (100 Hz at 16 kHz), the float64 shift at +4 semitones and the NumPy Griffin-Lim: the largest normalised
    autocorrelation between 60 and 400 Hz sits at lag 160 unshifted and 127 shifted, +-2, with a peak above 0.5"""
    from oracle import griffinlim_numpy as gl
    mag = pr.comb(1025, 24)[0]
    phase = 2.0 * np.pi * np.random.default_rng(0).random(mag.shape)
    plain = pr.f0_lag(gl.griffinlim(mag, phase, 10))
    moved = pr.f0_lag(gl.griffinlim(pr.shift(mag[None], None, [pr.pitch_step(4)])[0], phase, 10))
    print('  lag / peak unshifted %s, shifted %s' % (plain, moved))
    assert abs(plain[0] - 160) <= 2 and abs(moved[0] - 127) <= 2 and min(plain[1], moved[1]) > 0.5


# ---- tacotron_amd.lib ----------------------------------------------------------------------------------------------------------------
def test_pitch_step(built_lib):
    lib = built_lib
    assert (lib.PITCH_ONE, lib.PITCH_MIN_STEP, lib.PITCH_MAX_STEP, lib.PITCH_MAX_LIFTER) == (pr.ONE, pr.MIN_STEP, pr.MAX_STEP, pr.MAX_LIFTER)
    assert lib.pitch_step(0) == 65536 and lib.pitch_step(12) == 32768 and lib.pitch_step(-12) == 131072
    assert lib.pitch_step(4) == 52016 and lib.pitch_step(-5) == 87480 and lib.pitch_step(0.5) == round(65536 * 2 ** (-0.5 / 12))
    for x in (-12, -7.25, -1, 0, 3, 11.9, 12):
        assert lib.pitch_step(x) == pr.pitch_step(x) and pr.MIN_STEP <= lib.pitch_step(x) <= pr.MAX_STEP
    for bad in (12.001, -12.5, float('nan'), float('inf'), float('-inf'), None, 'high'):
        with pytest.raises(ValueError):
            lib.pitch_step(bad)


def test_frames_pitch_refuses_before_the_library(built_lib):
    import torch
    lib = built_lib
    x = torch.ones(2, 17, 8)
    for kw in (dict(step_q=100), dict(step_q=[65536]), dict(step_q=[65536, 200000]), dict(step_q=[65536.5, 65536]),
               dict(frames=torch.ones(2, dtype=torch.int64)), dict(frames_per_unit=0), dict(lifter=0), dict(lifter=9), dict(lifter=2.5),
               dict(out=torch.ones(2, 17, 9)), dict(out=x)):
        with pytest.raises(ValueError):
            lib.frames_pitch(x, lifter=kw.pop('lifter', 4), **kw)
    with pytest.raises(ValueError):
        lib.frames_pitch(x)                                              # the default lifter 32 needs C >= 65
    for bad in (x.double(), torch.ones(2, 16, 8), torch.ones(2, 2049, 8), torch.ones(2, 5, 8)):
        with pytest.raises(ValueError):
            lib.frames_pitch(bad, lifter=2)
    with pytest.raises(ValueError, match='no CPU fallback'):
        lib.frames_pitch(x, step_q=40000, lifter=4)


# ---- header and binding ------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_point(built_lib):
    import ctypes as C
    hdr = open(os.path.join(ROOT, 'include', 'taco_hip.h')).read()
    for name, value in (('TACO_PITCH_ONE', 65536), ('TACO_PITCH_MIN_STEP', 32768), ('TACO_PITCH_MAX_STEP', 131072),
                        ('TACO_PITCH_MAX_LIFTER', 64)):
        m = re.search(r'#define\s+%s\s+(\d+)' % name, hdr)
        assert m and int(m.group(1)) == value, name
    m = re.search(r'#define\s+TACO_PITCH_FLOOR\s+(\S+)', hdr)
    assert m and float(m.group(1).rstrip('f')) == pr.FLOOR
    decl = re.search(r'int\s+taco_frames_pitch\s*\(([^)]*)\)\s*;', hdr)
    assert decl, 'include/taco_hip.h does not declare taco_frames_pitch'
    args = [' '.join(a.split()) for a in decl.group(1).split(',')]
    assert args == ['const float* mag_t', 'const int32_t* frames', 'int frames_per_unit', 'const int32_t* step_q', 'int lifter',
                    'float* out', 'int B', 'int C', 'int F', 'void* stream']
    assert hdr.index('int taco_frames_stretch(') < decl.start() < hdr.index('int taco_corpus_batch(')
    assert 'Not here: pitch' not in hdr and int(re.search(r'#define\s+TACO_VERSION\s+(\d+)', hdr).group(1)) == 120
    P, I = C.c_void_p, C.c_int
    assert built_lib.EXPORTS['taco_frames_pitch'] == (C.c_int, [P, P, I, P, I, P, I, I, I, P])
    assert hasattr(C.CDLL(built_lib.LIB_PATH), 'taco_frames_pitch')


# ---- the driver's option -------------------------------------------------------------------------------------------------------------
def test_pitch_option(built_lib):
    from tacotron_amd import test as drv
    a = drv.parse_args([])
    assert a.pitch is None and a.lifter == 32
    assert drv.parse_args(['--pitch', '3']).pitch == 3.0 and drv.parse_args(['--pitch', '-2.5', '--lifter', '40']).lifter == 40
    a = drv.parse_args(['--pitch', '3', '--rate', '0.9', '--stop', '--vocode-lengths', '--gl-momentum', '0.99', '--deemphasis', '--long'])
    assert (a.pitch, a.rate) == (3.0, 0.9)
    for bad in (['--pitch', '12.5'], ['--pitch', 'nan'], ['--pitch', '-13'], ['--pitch', '1', '--lifter', '0'],
                ['--pitch', '1', '--lifter', '65']):
        with pytest.raises(SystemExit):
            drv.parse_args(bad)
    drv.check_options()
    drv.check_options(pitch=-12)
    drv.check_options(pitch=[0.5, 12, 0.0], lifter=64, rate=[1.0, 2.0, 0.5])
    for kw in (dict(pitch=12.1), dict(pitch=float('nan')), dict(pitch=[1.0, 15.0]), dict(pitch=1.0, vocode=False)):
        with pytest.raises(ValueError, match='pitch'):
            drv.check_options(**kw)
    for lifter in (0, 65, 2.5, True):
        with pytest.raises(ValueError, match='lifter'):
            drv.check_options(pitch=1.0, lifter=lifter)
    assert drv.pitch_steps(None, 3) is None and drv.pitch_steps(12, 3) == [32768] * 3 and drv.pitch_steps([0, -12], 2) == [65536, 131072]
    with pytest.raises(ValueError):
        drv.pitch_steps([1.0, 2.0], 3)
