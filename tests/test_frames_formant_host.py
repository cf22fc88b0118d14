"""CPU: the formant shift without a GPU -- what the float64 restatement (tests/formant_ref.py) does to a comb (the envelope's peak moves
by the ratio, the harmonics stay, the energy stays, a zero stays), the measurement that sizes FORMANT_RTOL, the header's declaration
and constants, the host checks of tacotron_amd.lib, and the driver's --formant.  No compute calls."""
import os
import re

import numpy as np
import pytest

from tests import formant_ref as fr
from tests import pitch_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('semitones', [-12, -4, -2, 2, 4, 12])
def test_the_envelope_moves_and_the_harmonics_stay(semitones):
    C, Q = 1025, 32
    m, _ = pr.comb(C=C, spacing=12.8)
    m = m[:, :4].copy()
    m[200, 1] = 0.0
    ratio = 2.0 ** (semitones / 12.0)
    y = fr.formant(m[None], None, [fr.formant_step(semitones)], 1, Q)[0]
    hi = int(0.3 * C * max(ratio, 1.0))
    whole = [0, 2, 3]                                                                       # (frame 1 has the zero bin: a dent of 18 in its L)
    peak_in = pr.log_envelope(m[:, whole], Q)[1][:int(0.3 * C)].argmax(axis=0)
    peak_out = pr.log_envelope(y[:, whole], Q)[1][:hi].argmax(axis=0)
    assert (peak_in == 118).all()
    assert np.abs(peak_out - ratio * peak_in).max() <= 2.0, (peak_out, ratio * peak_in)
    for f in whole:
        assert abs(pr.peak_spacing(y[:, f], 20, C - 20) - pr.peak_spacing(m[:, f], 20, C - 20)) <= 0.05
    m64 = m.astype(np.float64)
    assert np.abs((y * y).sum(axis=0) / (m64 * m64).sum(axis=0) - 1.0).max() <= 1e-12
    assert y[200, 1] == 0.0 and (y[:, 0] > 0).all()                                         # a zero bin stays zero


def test_peak_spacing_of_the_combs():
    """the harmonics of the small comb (6.4 bins apart at C = 129, the frames the device's F0 test uses) are as far apart behind a
    shift as in front of it"""
    C = 129
    m, _ = pr.comb(C=C, spacing=6.4)
    for semitones in (-3, 3):
        y = fr.formant(m[None, :, :1], None, [fr.formant_step(semitones)], 1, 32)[0]
        assert abs(pr.peak_spacing(m[:, 0], 8, C - 8) - 6.4) <= 0.1
        assert abs(pr.peak_spacing(y[:, 0], 8, C - 8) - pr.peak_spacing(m[:, 0], 8, C - 8)) <= 0.05


def test_one_is_the_identity_and_rows_end_where_they_end():
    x = fr.small_batch(1, B=3, C=17, F=11)
    x[0, 3, 2] = 0.0
    x[1, :, 7:] = np.nan
    out = fr.formant(x, [11, 7, 0], [fr.ONE] * 3, 1, 8)
    assert np.array_equal(out[0], x[0]) and np.array_equal(out[1, :, :7], x[1, :, :7])
    assert not out[1, :, 7:].any() and not out[2].any()
    assert np.array_equal(fr.formant(x[:1], None, None, 1, 8, dtype=np.float32).view(np.uint32), x[:1].view(np.uint32))
    out = fr.formant(x, [11, 7, 0], [40000, 100000, 50000], 1, 8)
    assert np.isfinite(out).all() and out[0, 3, 2] == 0.0 and not out[1, :, 7:].any()       # a zero bin stays zero; NaN is never read
    assert not fr.formant(np.zeros((1, 17, 4), dtype=np.float32), None, [40000], 1, 8).any()   # P1 == 0: g = 1
    # the envelope is held beyond the top bin: at the largest step the upper half of the output reads E[C - 1]
    E = np.linspace(0.0, 1.0, 17)[:, None]
    Ep = fr.moved_envelope(E, fr.MAX_STEP)
    assert np.array_equal(Ep[:8, 0], E[0:16:2, 0]) and (Ep[8:, 0] == E[16, 0]).all()
    assert np.allclose(fr.moved_envelope(E, fr.MIN_STEP)[:, 0], np.linspace(0.0, 0.5, 17))
    # a step outside the range is the clamped one
    assert np.array_equal(fr.formant(x[:1], None, [5], 1, 8), fr.formant(x[:1], None, [fr.MIN_STEP], 1, 8))
    assert np.array_equal(fr.formant(x[:1], None, [2 ** 30], 1, 8), fr.formant(x[:1], None, [fr.MAX_STEP], 1, 8))


def test_rtol_is_four_times_the_float32_error():
    """FORMANT_RTOL comes from the restatement alone: the float32 form against the float64 one on every input of the GPU tests; the
    record is the measurement rounded up"""
    worst, where, names = 0.0, None, []
    for name, x, frames, r, steps, Q in fr.all_cases():
        names.append(name)
        e = fr.rel_err(fr.formant(x, frames, steps, r, Q, dtype=np.float32), fr.formant(x, frames, steps, r, Q))
        if e > worst:
            worst, where = e, name
    assert len(names) == len(set(names)) == 8 * 5 + 8
    print('  largest float32 error %.3g on %s; recorded %.3g' % (worst, where, fr.MEASURED_FLOAT32_ERROR))
    assert 0.8 * fr.MEASURED_FLOAT32_ERROR <= worst <= fr.MEASURED_FLOAT32_ERROR
    assert fr.FORMANT_RTOL == 4.0 * fr.MEASURED_FLOAT32_ERROR


def test_the_cases_cover_what_they_must():
    cases = {c[0]: c[1:] for c in fr.all_cases()}
    seen = set()
    for C, Qs in fr.SHAPES:
        assert Qs[0] == 1 and Qs[-1] == min(fr.MAX_LIFTER, (C - 1) // 2)
        for Q in Qs:
            for F in fr.EDGE_F:
                x, frames, r, steps, q = cases['mixed_C%d_Q%d_F%d' % (C, Q, F)]
                assert x.shape == (3, C, F) and len(set(frames)) == (3 if F > 1 else 2) and 0 in frames and not x[1].any() and q == Q
                assert fr.clamp_step(steps[0]) != fr.ONE
                seen.add(steps[0])
                live = x[0, :, :frames[0]]                                                  # and the reference does move the live row
                assert np.abs(fr.formant(x, frames, steps, r, Q)[0, :, :frames[0]] / live - 1.0).max() > 0.01
    assert seen == set(fr.STEPS) and min(seen) < fr.MIN_STEP and max(seen) > fr.MAX_STEP
    assert {fr.formant_step(3), fr.formant_step(-3), fr.MIN_STEP, fr.MAX_STEP} <= seen
    assert [C for C, _ in fr.SHAPES] == [9, 17, 129] and fr.SHAPES[2][1] == (1, 32, 33, 64) and fr.EDGE_F == (1, 31, 32, 33, 65)
    x, frames, r, steps, Q = cases['production']
    assert x.shape == (2, 1025, 40) and Q == 32 and frames == (40, 37)
    x = cases['floor'][0]
    out = fr.formant(x, None, cases['floor'][3], 1, 32)
    assert out[out > 0].min() > 1.2e-38                                                     # every output a normal float32
    assert cases['per_unit_3'][2] == 3 and cases['past_2_31'][1][0] * cases['past_2_31'][2] > 2 ** 31 > 0 > cases['past_2_31'][1][1]


# ---- header and binding ------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_point(built_lib):
    import ctypes as C
    lib = built_lib
    hdr = open(os.path.join(ROOT, 'include', 'taco_hip.h')).read()
    for name, value, mine in (('TACO_PITCH_ONE', fr.ONE, lib.PITCH_ONE), ('TACO_PITCH_MIN_STEP', fr.MIN_STEP, lib.PITCH_MIN_STEP),
                              ('TACO_PITCH_MAX_STEP', fr.MAX_STEP, lib.PITCH_MAX_STEP), ('TACO_PITCH_MAX_LIFTER', fr.MAX_LIFTER, lib.PITCH_MAX_LIFTER)):
        m = re.search(r'#define\s+%s\s+(\d+)' % name, hdr)
        assert m and int(m.group(1)) == value == mine, name
    assert float(re.search(r'#define\s+TACO_PITCH_FLOOR\s+(\S+)', hdr).group(1).rstrip('f')) == fr.FLOOR
    decl = re.search(r'int\s+taco_frames_formant\s*\(([^)]*)\)\s*;', hdr)
    assert decl, 'include/taco_hip.h does not declare taco_frames_formant'
    args = [' '.join(a.split()) for a in decl.group(1).split(',')]
    assert args == ['const float* mag_t', 'const int32_t* frames', 'int frames_per_unit', 'const int32_t* step_q', 'int lifter', 'float* out',
                    'int B', 'int C', 'int F', 'void* stream']
    pitch = re.search(r'int\s+taco_frames_pitch\s*\(([^)]*)\)\s*;', hdr)
    assert args == [' '.join(a.split()) for a in pitch.group(1).split(',')]                 # exactly taco_frames_pitch's arguments
    assert hdr.index('int taco_frames_pitch(') < hdr.index('int taco_frames_formant(') < hdr.index('int taco_path_curve(')
    assert int(re.search(r'#define\s+TACO_VERSION\s+(\d+)', hdr).group(1)) == 120           # detected by the symbol, not the version
    doc = hdr[hdr.index('Timbre at synthesis'):hdr.index('int taco_frames_formant(')]
    for word in ('per-frame or per-word formant curve', 'fused pitch + formant', 'mel frames', 'tapered', 'Nobody has listened', 'untuned'):
        assert word in ' '.join(doc.replace('*', ' ').split()), word
    P, I = C.c_void_p, C.c_int
    assert lib.EXPORTS['taco_frames_formant'] == (C.c_int, [P, P, I, P, I, P, I, I, I, P]) == lib.EXPORTS['taco_frames_pitch']
    assert hasattr(C.CDLL(lib.LIB_PATH), 'taco_frames_formant')


def test_formant_step(built_lib):
    lib = built_lib
    for st in (-12, -7.5, -3, 0, 0.01, 2, 3, 12):
        assert lib.formant_step(st) == fr.formant_step(st) == lib.pitch_step(st) == pr.pitch_step(st)
    assert (lib.formant_step(12), lib.formant_step(0), lib.formant_step(-12)) == (fr.MIN_STEP, fr.ONE, fr.MAX_STEP)
    assert lib.formant_step(3) < fr.ONE < lib.formant_step(-3)                              # up: fewer source bins per output bin
    for bad in (12.01, -12.01, float('nan'), float('inf'), 'x', None):
        with pytest.raises(ValueError, match='formant'):
            lib.formant_step(bad)
    assert lib.steps_of(None, lib.formant_step) is None and lib.steps_of(2, lib.formant_step) == fr.formant_step(2)
    assert lib.steps_of([0, -3.0], lib.formant_step, 2) == [fr.ONE, fr.formant_step(-3)]
    with pytest.raises(ValueError):
        lib.steps_of([0, 1, 2], lib.formant_step, 2)
    with pytest.raises(ValueError, match='formant'):
        lib.steps_of([0, 13], lib.formant_step, 2)


def test_wrapper_refuses_before_the_library(built_lib):
    import torch
    lib = built_lib
    x = torch.ones(2, 17, 8)
    for kw in (dict(step_q=32767), dict(step_q=131073), dict(step_q=[65536]), dict(step_q=[65536, 1]), dict(step_q=2.5),
               dict(step_q=torch.ones(2, dtype=torch.int64)), dict(frames=torch.ones(2, dtype=torch.int64)),
               dict(frames=torch.ones(3, dtype=torch.int32)), dict(frames_per_unit=0), dict(lifter=0), dict(lifter=9), dict(lifter=2.5),
               dict(out=torch.ones(2, 17, 9)), dict(out=x)):
        with pytest.raises(ValueError, match='frames_formant'):
            lib.frames_formant(x, **dict(dict(lifter=4), **kw))
    with pytest.raises(ValueError, match='lifter'):
        lib.frames_formant(x)                                            # the default lifter 32 needs C >= 65
    for bad in (x.double(), torch.ones(2, 16, 8), torch.ones(2, 2049, 8), torch.ones(2, 5, 8), torch.ones(2, 17, 8193), torch.ones(17, 8)):
        with pytest.raises(ValueError):
            lib.frames_formant(bad, lifter=2)
    for call in (lambda: lib.frames_formant(x, lifter=4), lambda: lib.frames_formant(x, None, 40000, 1, 4)):
        with pytest.raises(ValueError, match='no CPU fallback'):
            call()


# ---- the driver's option -------------------------------------------------------------------------------------------------------------
def test_formant_option(built_lib, tmp_path):
    from tacotron_amd import test as drv
    from tacotron_amd.config import Config
    a = drv.parse_args([])
    assert a.formant is None and a.formant_lifter == 32 and (Config.formant, Config.formant_lifter) == (None, 32) and drv.FORMANT_LIFTER == 32
    a = drv.parse_args(['--formant', '2', '--formant-lifter', '24', '--sharpen', '0.4', '--pitch', '3', '--rate', '0.9', '--stop',
                        '--vocode-lengths', '--f0', '--gl-momentum', '0.99', '--deemphasis', '--long', '--loudness', '-16', '--limit'])
    assert (a.formant, a.formant_lifter, a.sharpen, a.pitch, a.rate) == (2.0, 24, 0.4, 3.0, 0.9)
    for bad in (['--formant', '12.5'], ['--formant', 'nan'], ['--formant', '-13'], ['--formant', '2', '--formant-lifter', '0'],
                ['--formant', '2', '--formant-lifter', '65'], ['--formant-lifter', '16']):
        with pytest.raises(SystemExit):
            drv.parse_args(bad)
    assert drv.formant_options() is None and drv.formant_options(0) is None and drv.formant_options(-0.0, 16) is None
    assert drv.formant_options(2) == (fr.formant_step(2), 32) and drv.formant_options(-12, 1) == (fr.MAX_STEP, 1)
    assert drv.formant_options(12.0, 64) == (fr.MIN_STEP, 64)
    for kw in (dict(formant=12.01), dict(formant=float('nan')), dict(formant='x'), dict(formant=True), dict(formant=2, vocode=False)):
        with pytest.raises(ValueError, match='formant'):
            drv.formant_options(**kw)
    for lifter in (0, 65, 2.5, True):
        with pytest.raises(ValueError, match='formant_lifter'):
            drv.formant_options(2, lifter)
    o = drv.Options(pitch=2.0).resolved(0.4, 16, -3, 20)
    assert o.sharpen == (0.4, 16) and o.formant == (fr.formant_step(-3), 20) and o.pitch == 2.0
    assert drv.Options().resolved().formant is None and drv.Options().resolved(formant=0.0).formant is None
    with pytest.raises(ValueError, match='formant'):
        drv.Options(vocode=False).resolved(formant=2)
    c = Config()
    c.formant = 20.0
    with pytest.raises(ValueError, match='formant'):   # test() validates in the same place, before anything is loaded
        drv.test(c, [])
    spec, align = np.zeros((8, 1025), np.float32), np.zeros((4, 5), np.float32)
    drv.write_prompt(str(tmp_path), 0, 2, spec, align)
    assert not (tmp_path / 'prompt_000_formant.npy').exists()
    drv.write_prompt(str(tmp_path), 1, 2, spec, align, formant=(fr.formant_step(2), 32))
    got = np.load(tmp_path / 'prompt_001_formant.npy')
    assert got.dtype == np.int32 and got.tolist() == [fr.formant_step(2), 32]
    drv.write_prompt(str(tmp_path), 2, 2, spec, align, piece=1, formant=(fr.formant_step(2), 32))
    assert (tmp_path / 'prompt_002_k01_formant.npy').exists()
    assert drv.formant_line('prompt 3', fr.formant_step(2), [57.0, 0.0025, 0.01]) == (
        'prompt 3 formant asked +2.00 semitones, F0 moved +3 cents over 57 voiced frames')
    assert '--formant SEMITONES' in drv.__doc__ and 'UNTUNED' in drv.__doc__[drv.__doc__.index('--formant SEMITONES'):]
