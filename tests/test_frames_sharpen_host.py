"""CPU: spectral sharpening and the global variance without a GPU -- what the float64 restatements (tests/sharpen_ref.py) do to moving
combs, the measure and the cure together, the measurement that sizes SHARPEN_RTOL and CEPSTATS_RTOL, the header's declarations and
constants, the host checks of tacotron_amd.lib, the driver's --sharpen and evaluate's --gv helpers.  No compute calls."""
import os
import re

import numpy as np
import pytest

from tests import sharpen_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C,Q,beta', [(129, 32, 0.4), (129, 64, -0.4), (33, 2, 1.0), (1025, 32, -1.0), (17, 8, 0.25)])
def test_cepstral_and_energy_identity(C, Q, beta):
    """in float64: c'[n] = (1 + beta) c[n] for 2 <= n <= Q, every other quefrency but 0 stays, and the frame keeps its energy"""
    m = sr.moving_comb(C, 5, seed=C + Q)
    y = sr.sharpen(m[None], beta, lifter=Q)[0]
    c, cy = sr.cepstra(m, C - 1), sr.cepstra(y, C - 1)
    scale = np.ones((C, 1))
    scale[sr.FIRST:Q + 1] = 1.0 + beta
    assert np.abs(cy[1:] - (scale * c)[1:]).max() < 1e-9
    m64 = m.astype(np.float64)
    assert np.abs((y * y).sum(axis=0) / (m64 * m64).sum(axis=0) - 1.0).max() < 1e-9
    assert np.abs(np.log(y) - np.log(m64)).max() > 0.01                                    # (and the frame did change)


def test_beta_zero_is_the_identity_and_rows_end_where_they_end():
    x = sr.small_batch(1, B=3, C=17, F=11)
    x[0, 3, 2] = 0.0
    x[1, :, 7:] = np.nan
    out = sr.sharpen(x, 0.0, frames=[11, 7, 0], lifter=8)
    assert np.array_equal(out[0], x[0]) and np.array_equal(out[1, :, :7], x[1, :, :7])
    assert not out[1, :, 7:].any() and not out[2].any()
    assert np.array_equal(sr.sharpen(x[:1], 0.0, lifter=8, dtype=np.float32).view(np.uint32), x[:1].view(np.uint32))
    out = sr.sharpen(x, 0.5, frames=[11, 7, 0], lifter=8)
    assert np.isfinite(out).all() and out[0, 3, 2] == 0.0 and not out[1, :, 7:].any()      # a zero bin stays zero; NaN is never read
    assert not sr.sharpen(np.zeros((1, 17, 4), dtype=np.float32), 0.5, lifter=8).any()     # P1 == 0: g = 1


def test_measure_and_cure_round_trip():
    """frames flattened with beta = -0.4 have 0.6^2 of the originals' variance in every scaled quefrency 2 .. Q; quefrency 1 is never
    scaled, so the GV ratio over n = 1 .. Q -- a geometric mean with that one factor of 1 in it -- is 0.36^((Q - 1) / Q), exactly;
    sharpening the flattened frames with beta = 2/3 brings the ratio back to 1 within 1e-6"""
    Q = 32
    x = np.stack([sr.moving_comb(129, 40, seed=3), sr.moving_comb(129, 40, seed=4)])
    x[1, :, 25:] = np.nan
    frames = [40, 25]
    flat = sr.sharpen(x, -0.4, frames, lifter=Q).astype(np.float32)
    s0, n0 = sr.cepstats(x, frames, lifter=Q)
    s1, n1 = sr.cepstats(flat, frames, lifter=Q)
    assert n0.tolist() == n1.tolist() == frames
    v0, v1 = sr.variance(s0, n0), sr.variance(s1, n1)
    assert np.abs(v1[:, sr.FIRST:] / v0[:, sr.FIRST:] / 0.36 - 1.0).max() < 1e-5           # (flat was rounded to float32)
    assert np.abs(v1[:, 1] / v0[:, 1] - 1.0).max() < 1e-5
    ratio = sr.gv_ratio(s1, n1, s0, n0)
    assert np.abs(ratio / 0.36 ** ((Q - 1) / Q) - 1.0).max() < 1e-5 and (ratio < 0.8).all()
    # the same in float64 throughout, where the statement is exact
    flat64 = sr.sharpen_frames(x[0], -0.4, Q)
    c0, c1 = sr.cepstra(x[0], Q), sr.cepstra(flat64, Q)
    assert np.abs(c1[sr.FIRST:].var(axis=1) / c0[sr.FIRST:].var(axis=1) / 0.36 - 1.0).max() < 1e-9
    back = sr.sharpen(flat, 2.0 / 3.0, frames, lifter=Q).astype(np.float32)
    s2, n2 = sr.cepstats(back, frames, lifter=Q)
    assert np.abs(sr.gv_ratio(s2, n2, s0, n0) - 1.0).max() < 1e-6
    # fewer than two frames on either side: no ratio
    assert np.isnan(sr.gv_ratio(s0, [1, 25], s0, n0)[0]) and np.isnan(sr.gv_ratio(s0, n0, s0, [40, 0])[1])


def test_rtols_are_four_times_the_float32_error():
    """SHARPEN_RTOL and CEPSTATS_RTOL come from the restatements alone: the float32 forms against the float64 ones on every input of
    the GPU tests; the records are the measurements rounded up"""
    worst, where = {'sharpen': 0.0, 'cepstats': 0.0}, {}
    names = []
    for name, x, frames, r, beta, Q in sr.all_cases():
        names.append(name)
        e = sr.rel_err(sr.sharpen(x, beta, frames, r, Q, dtype=np.float32), sr.sharpen(x, beta, frames, r, Q))
        s32, n32 = sr.cepstats(x, frames, r, Q, dtype=np.float32)
        s64, n64 = sr.cepstats(x, frames, r, Q)
        for key, err in (('sharpen', e), ('cepstats', sr.var_err(s32, n32, s64, n64))):
            if err > worst[key]:
                worst[key], where[key] = err, name
    assert len(names) == len(set(names)) == 8 * 5 + 6
    for key in worst:
        print('  %s: largest float32 error %.3g on %s; recorded %.3g' % (key, worst[key], where[key], sr.MEASURED_FLOAT32_ERROR[key]))
        assert 0.8 * sr.MEASURED_FLOAT32_ERROR[key] <= worst[key] <= sr.MEASURED_FLOAT32_ERROR[key]
    assert sr.SHARPEN_RTOL == 4.0 * sr.MEASURED_FLOAT32_ERROR['sharpen'] and sr.CEPSTATS_RTOL == 4.0 * sr.MEASURED_FLOAT32_ERROR['cepstats']


def test_the_cases_cover_what_they_must():
    cases = {c[0]: c[1:] for c in sr.all_cases()}
    for C, Qs in sr.SHAPES:
        assert Qs[0] == sr.FIRST and Qs[-1] == min(sr.MAX_LIFTER, (C - 1) // 2)
        for Q in Qs:
            for F in sr.EDGE_F:
                x, frames, r, beta, q = cases['mixed_C%d_Q%d_F%d' % (C, Q, F)]
                assert x.shape == (3, C, F) and len(set(frames)) == (3 if F > 1 else 2) and 0 in frames and not x[1].any() and beta != 0
    assert [C for C, _ in sr.SHAPES] == [9, 17, 129] and sr.SHAPES[2][1] == (2, 32, 33, 64) and sr.EDGE_F == (1, 31, 32, 33, 65)
    x, frames, r, _, Q = cases['production']
    assert x.shape == (2, 1025, 40) and Q == 32
    # the variance of every coefficient of a moving comb is not tiny against its squared mean
    s, n = sr.cepstats(cases['production'][0], cases['production'][1], lifter=32)
    v = sr.variance(s, n)[:, 1:]
    assert (v / (s[:, 1:, 0] / n[:, None]) ** 2 > 0.05).all()


# ---- header and binding ------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points(built_lib):
    import ctypes as C
    lib = built_lib
    hdr = open(os.path.join(ROOT, 'include', 'taco_hip.h')).read()
    m = re.search(r'#define\s+TACO_SHARPEN_FIRST\s+(\d+)', hdr)
    assert m and int(m.group(1)) == sr.FIRST == lib.SHARPEN_FIRST
    for name, value, mine in (('TACO_SHARPEN_MIN_BETA', sr.MIN_BETA, lib.SHARPEN_MIN_BETA), ('TACO_SHARPEN_MAX_BETA', sr.MAX_BETA, lib.SHARPEN_MAX_BETA)):
        m = re.search(r'#define\s+%s\s+(\S+)' % name, hdr)
        assert m and float(m.group(1).rstrip('f')) == value == mine, name
    assert lib.PITCH_MAX_LIFTER == sr.MAX_LIFTER and float(re.search(r'#define\s+TACO_PITCH_FLOOR\s+(\S+)', hdr).group(1).rstrip('f')) == sr.FLOOR
    decl = re.search(r'int\s+taco_frames_sharpen\s*\(([^)]*)\)\s*;', hdr)
    assert decl, 'include/taco_hip.h does not declare taco_frames_sharpen'
    assert [' '.join(a.split()) for a in decl.group(1).split(',')] == [
        'const float* mag_t', 'const int32_t* frames', 'int frames_per_unit', 'float beta', 'int lifter', 'float* out', 'int B', 'int C',
        'int F', 'void* stream']
    decl = re.search(r'int\s+taco_frames_cepstats\s*\(([^)]*)\)\s*;', hdr)
    assert [' '.join(a.split()) for a in decl.group(1).split(',')] == [
        'const float* mag_t', 'const int32_t* frames', 'int frames_per_unit', 'int lifter', 'double* sums', 'int32_t* count',
        'void* workspace', 'int B', 'int C', 'int F', 'void* stream']
    assert re.search(r'int64_t\s+taco_frames_cepstats_workspace_bytes\s*\(\s*int B,\s*int C,\s*int F,\s*int lifter\s*\)\s*;', hdr)
    assert int(re.search(r'#define\s+TACO_VERSION\s+(\d+)', hdr).group(1)) == 120           # detected by the symbol, not the version
    for word in ('per-row or per-frame beta', 'tapered lifter', 'mel frames'):
        assert word in hdr[hdr.index('taco_frames_sharpen:'):hdr.index('int taco_frames_sharpen(')]
    P, I = C.c_void_p, C.c_int
    assert lib.EXPORTS['taco_frames_sharpen'] == (C.c_int, [P, P, I, C.c_float, I, P, I, I, I, P])
    assert lib.EXPORTS['taco_frames_cepstats'] == (C.c_int, [P, P, I, I, P, P, P, I, I, I, P])
    raw = C.CDLL(lib.LIB_PATH)
    assert all(hasattr(raw, n) for n in ('taco_frames_sharpen', 'taco_frames_cepstats', 'taco_frames_cepstats_workspace_bytes'))
    # the size function needs no device: (Q + 1) pairs of fp64 per tile of 32 frames and row, and the slack that aligns them
    assert lib.frames_cepstats_workspace_bytes(2, 1025, 40, 32) == 2 * 2 * 33 * 16 + 8
    assert lib.frames_cepstats_workspace_bytes(3, 17, 32, 8) == 3 * 9 * 16 + 8 and lib.frames_cepstats_workspace_bytes(3, 17, 33, 8) == 2 * 3 * 9 * 16 + 8
    for bad in ((0, 17, 8, 4), (2, 16, 8, 4), (2, 17, 0, 4), (2, 17, 8193, 4), (2, 17, 8, 1), (2, 17, 8, 9), (2, 1025, 8, 65)):
        with pytest.raises(lib.TacoError):
            lib.frames_cepstats_workspace_bytes(*bad)


def test_wrappers_refuse_before_the_library(built_lib):
    import torch
    lib = built_lib
    x = torch.ones(2, 17, 8)
    for kw in (dict(beta=1.5), dict(beta=-1.01), dict(beta=float('nan')), dict(beta=None), dict(beta='much'), dict(beta=True),
               dict(frames=torch.ones(2, dtype=torch.int64)), dict(frames=torch.ones(3, dtype=torch.int32)), dict(frames_per_unit=0),
               dict(lifter=1), dict(lifter=9), dict(lifter=2.5), dict(out=torch.ones(2, 17, 9)), dict(out=x)):
        with pytest.raises(ValueError, match='frames_sharpen'):
            lib.frames_sharpen(x, kw.pop('beta', 0.4), kw.pop('lifter', 4), **kw)
    with pytest.raises(ValueError, match='lifter'):
        lib.frames_sharpen(x, 0.4)                                       # the default lifter 32 needs C >= 65
    for bad in (x.double(), torch.ones(2, 16, 8), torch.ones(2, 2049, 8), torch.ones(2, 5, 8), torch.ones(2, 17, 8193)):
        with pytest.raises(ValueError):
            lib.frames_sharpen(bad, 0.4, 2)
        with pytest.raises(ValueError):
            lib.frames_cepstats(bad, 2)
    for kw in (dict(lifter=1), dict(lifter=9), dict(frames=torch.ones(2, dtype=torch.int64)), dict(frames_per_unit=0),
               dict(out=(torch.ones(2, 5, 2),)), dict(out=(torch.ones(2, 5, 2), torch.ones(2, dtype=torch.int32))),
               dict(workspace=torch.ones(64))):
        with pytest.raises(ValueError, match='frames_cepstats'):
            lib.frames_cepstats(x, kw.pop('lifter', 4), **kw)
    for call in (lambda: lib.frames_sharpen(x, 0.4, 4), lambda: lib.frames_sharpen(x, 0.0, 4), lambda: lib.frames_cepstats(x, 4)):
        with pytest.raises(ValueError, match='no CPU fallback'):
            call()


def test_host_arithmetic_of_the_ratio(built_lib):
    """lib.gv_variance / lib.gv_ratio against the restatement on made-up sums"""
    lib = built_lib
    rng = np.random.default_rng(5)
    c = rng.standard_normal((4, 9, 30)) * 0.1 + rng.standard_normal((4, 9, 1))
    n = np.array([30, 2, 1, 0])
    sums = np.stack([np.stack([(c[b, :, :n[b]]).sum(axis=1), (c[b, :, :n[b]] ** 2).sum(axis=1)], axis=1) for b in range(4)])
    var = lib.gv_variance(sums, n)
    assert np.allclose(var[0], c[0].var(axis=1), rtol=1e-9) and np.allclose(var[1], c[1, :, :2].var(axis=1), rtol=1e-9)
    assert np.isnan(var[2:]).all() and np.array_equal(var, sr.variance(sums, n), equal_nan=True)
    half = sums.copy()
    half[..., 0] *= 0.5
    half[..., 1] *= 0.25
    got = lib.gv_ratio(half, n, sums, n)
    assert np.allclose(got[:2], 0.25, rtol=1e-9) and np.isnan(got[2:]).all()
    assert np.array_equal(got, sr.gv_ratio(half, n, sums, n), equal_nan=True)


# ---- evaluate's helpers --------------------------------------------------------------------------------------------------------------
def test_evaluate_columns_and_lines(built_lib):
    from tacotron_amd import evaluate as ev
    rng = np.random.default_rng(6)
    c = rng.standard_normal((3, 5, 20))
    n = np.array([20, 20, 1])
    sums = np.stack([c.sum(axis=2), (c ** 2).sum(axis=2)], axis=2)
    low = sums * np.array([0.7, 0.49])
    cols = ev.gv_columns(low, n, sums, n)
    assert cols.shape == (3, 1) and cols.dtype == np.float64 and np.allclose(cols[:2, 0], 0.49) and np.isnan(cols[2, 0])
    both = ev.gv_columns(low, n, sums, n, sums)
    assert both.shape == (3, 2) and np.array_equal(both[:, :1], cols, equal_nan=True) and np.allclose(both[:2, 1], 1.0)
    assert ev.GV_COLUMNS == ('gv_ratio',) and ev.GV_SHARPEN_COLUMNS == ('gv_ratio', 'gv_ratio_sharpened') and ev.GV_LOW == 0.8
    assert np.allclose(ev.gv_summary(cols), (0.49, 1.0)) and np.allclose(ev.gv_summary(both), (0.49, 1.0, 1.0, 0.0))
    assert all(np.isnan(v) for v in ev.gv_summary(np.full((2, 1), np.nan)))
    assert np.allclose(ev.gv_summary(np.array([[0.5], [0.9], [np.nan], [1.1]])), (2.5 / 3, 1.0 / 3))
    assert ev.gv_line((0.61, 0.75)) == 'GV ratio 0.61 (0.750 of the utterances below 0.8)'
    assert ev.gv_line((0.61, 0.75, 0.97, 0.0), 0.4) == ('GV ratio 0.61, with --sharpen 0.40: 0.97 (share of the utterances below 0.8: '
                                                           '0.750, 0.000)')
    a = ev.parse_args(['--gv'])
    assert a.gv and a.gv_lifter == 32 and a.sharpen is None
    a = ev.parse_args(['--gv', '--gv-lifter', '20', '--sharpen', '0.4', '--f0'])
    assert (a.gv_lifter, a.sharpen, a.f0) == (20, 0.4, True)
    assert not ev.parse_args([]).gv
    for bad in (['--sharpen', '0.4'], ['--gv-lifter', '20']):
        with pytest.raises(SystemExit):
            ev.parse_args(bad)
    for kw in (dict(sharpen=0.4), dict(gv=True, gv_lifter=1), dict(gv=True, gv_lifter=65), dict(gv=True, sharpen=1.5),
               dict(gv=True, sharpen=float('nan'))):
        with pytest.raises(ValueError):
            ev.evaluate(None, **kw)
    doc = ev.__doc__ + ev.parse_args.__doc__ if ev.parse_args.__doc__ else ev.__doc__
    assert 'NOT with published mel-cepstral GV figures' in doc and 'untrained' in doc


# ---- the driver's option -------------------------------------------------------------------------------------------------------------
def test_sharpen_option(built_lib, tmp_path):
    from tacotron_amd import test as drv
    from tacotron_amd.config import Config
    a = drv.parse_args([])
    assert a.sharpen is None and a.sharpen_lifter == 32 and (Config.sharpen, Config.sharpen_lifter) == (None, 32)
    a = drv.parse_args(['--sharpen', '0.4', '--sharpen-lifter', '24', '--pitch', '3', '--rate', '0.9', '--stop', '--vocode-lengths', '--f0',
                        '--gl-momentum', '0.99', '--deemphasis', '--long', '--loudness', '-16', '--limit'])
    assert (a.sharpen, a.sharpen_lifter, a.pitch, a.rate) == (0.4, 24, 3.0, 0.9)
    for bad in (['--sharpen', '1.5'], ['--sharpen', 'nan'], ['--sharpen', '-1.1'], ['--sharpen', '0.4', '--sharpen-lifter', '1'],
                ['--sharpen', '0.4', '--sharpen-lifter', '65'], ['--sharpen-lifter', '16']):
        with pytest.raises(SystemExit):
            drv.parse_args(bad)
    assert drv.sharpen_options() is None and drv.sharpen_options(0) is None and drv.sharpen_options(-0.0, 16) is None
    assert drv.sharpen_options(0.4) == (0.4, 32) and drv.sharpen_options(-1, 2) == (-1.0, 2) and drv.sharpen_options(1.0, 64) == (1.0, 64)
    for kw in (dict(sharpen=1.01), dict(sharpen=float('nan')), dict(sharpen='x'), dict(sharpen=True), dict(sharpen=0.4, vocode=False)):
        with pytest.raises(ValueError, match='sharpen'):
            drv.sharpen_options(**kw)
    for lifter in (1, 65, 2.5, True):
        with pytest.raises(ValueError, match='sharpen_lifter'):
            drv.sharpen_options(0.4, lifter)
    o = drv.Options(pitch=2.0).resolved(0.4, 16)
    assert o.sharpen == (0.4, 16) and o.pitch == 2.0 and drv.Options().resolved().sharpen is None and drv.Options().resolved(0.0).sharpen is None
    c = Config()
    c.sharpen = 2.0
    with pytest.raises(ValueError, match='sharpen'):   # test() validates in the same place, before anything is loaded
        drv.test(c, [])
    spec, align = np.zeros((8, 1025), np.float32), np.zeros((4, 5), np.float32)
    drv.write_prompt(str(tmp_path), 0, 2, spec, align)
    assert not (tmp_path / 'prompt_000_sharpen.npy').exists()
    drv.write_prompt(str(tmp_path), 1, 2, spec, align, sharpen=(0.4, 32))
    got = np.load(tmp_path / 'prompt_001_sharpen.npy')
    assert got.dtype == np.float64 and got.tolist() == [0.4, 32.0]
    assert '--sharpen BETA' in drv.__doc__ and 'UNTUNED' in drv.__doc__
