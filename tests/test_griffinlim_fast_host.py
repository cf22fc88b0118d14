"""CPU checks of fast Griffin-Lim (taco_griffinlim_fast): the C ABI declaration and its version, the Python binding's argument
checks, the driver's options, and the fp64 restatement (tests/fgl_ref.py) -- including the claim the entry point rests on:
momentum 0.99 reaches in 30 rounds what the plain algorithm needs more than 50 for."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from oracle import griffinlim_numpy as gl
from tests import fgl_ref

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'taco_hip.h')


def _args(decl):
    return [' '.join(a.split()) for a in decl.replace('\n', ' ').split(',')]


def test_header_declares_both_entry_points():
    hdr = open(HDR).read()
    ws = re.search(r'int64_t taco_griffinlim_fast_workspace_bytes\(([^)]*)\);', hdr)
    assert ws and _args(ws.group(1)) == ['int B', 'int F']
    fn = re.search(r'\bint taco_griffinlim_fast\(([^)]*)\);', hdr)
    assert fn
    assert _args(fn.group(1)) == ['const float* mag_t', 'const float* phase0', 'uint64_t seed', 'const int32_t* frames',
                                  'int frames_per_unit', 'float momentum', 'float* wave', 'float* conv', 'void* workspace', 'int B',
                                  'int F', 'int n_iter', 'void* stream']
    assert int(re.search(r'#define\s+TACO_VERSION\s+(\d+)', hdr).group(1)) == 120
    assert 'Perraudin' in hdr and 'librosa' in hdr


def test_library_exports_them_at_version_120(built_lib):
    assert built_lib.version() == 120
    for name in ('taco_griffinlim_fast_workspace_bytes', 'taco_griffinlim_fast'):
        assert name in built_lib.EXPORTS
        assert hasattr(C.CDLL(built_lib.LIB_PATH), name)
    res, args = built_lib.EXPORTS['taco_griffinlim_fast']
    P, I = C.c_void_p, C.c_int
    assert res is C.c_int and args == [P, P, C.c_uint64, P, I, C.c_float, P, P, P, I, I, I, P]
    assert built_lib.EXPORTS['taco_griffinlim_fast_workspace_bytes'] == (C.c_int64, [I, I])


def test_workspace_size(built_lib):
    """the per-utterance layout + a second spectrum (B, F, 1025, 2) + two (B, F) tables of partial sums + B; no n_iter in it"""
    for B, F in ((1, 5), (5, 41), (32, 360)):
        n = built_lib.griffinlim_fast_workspace_floats(B, F)
        assert n - built_lib.griffinlim_rows_workspace_floats(B, F) == B * F * 1025 * 2 + 2 * B * F + B
    for B, F in ((0, 41), (-1, 41), (2, 4), (2, 0)):
        with pytest.raises(built_lib.TacoError):
            built_lib.griffinlim_fast_workspace_floats(B, F)


def test_wrapper_refuses_bad_arguments_before_any_device_call(built_lib):
    """every refusal is raised on the host before the entry point is called (CPU tensors never reach it)"""
    B, F = 2, 8
    mag = torch.ones(B, 1025, F)
    frames = torch.tensor([8, 5], dtype=torch.int32)
    called = []
    real = built_lib._lib.taco_griffinlim_fast
    bad = [
        dict(mag_t=torch.ones(B, 1024, F)),                                     # not 1025 bins
        dict(mag_t=torch.ones(1025, F)),                                        # no batch dimension
        dict(mag_t=mag.double()),                                               # not float32
        dict(mag_t=mag, frames=frames.long()),                                  # int64 lengths
        dict(mag_t=mag, frames=torch.tensor([8, 5, 5], dtype=torch.int32)),     # B + 1 lengths
        dict(mag_t=mag, frames=frames.view(B, 1)),                              # (B, 1)
        dict(mag_t=mag, phase0=torch.zeros(B, 1025, F + 1)),                    # phases of another shape
        dict(mag_t=mag, phase0=torch.zeros(B, 1025, F, dtype=torch.float64)),
        dict(mag_t=mag, frames=frames, frames_per_unit=0),
        dict(mag_t=mag, frames_per_unit=0),                                     # (>= 1 even where it is ignored)
        dict(mag_t=mag, n_iter=-1),
        dict(mag_t=mag, momentum=-0.01),
        dict(mag_t=mag, momentum=1.0),
        dict(mag_t=mag, momentum=1.5),
        dict(mag_t=mag, momentum=float('nan')),
        dict(mag_t=mag, momentum=1.0 - 1e-12),                                  # 1 once it is a float
        dict(mag_t=mag, out=torch.zeros(B, 300 * F)),                           # waveform buffer of the wrong length
        dict(mag_t=mag, n_iter=3, conv=torch.zeros(B, 3)),                      # n_iter + 1 values per row
        dict(mag_t=mag, n_iter=3, conv=torch.zeros(B, 4, dtype=torch.float64)),
        dict(mag_t=mag, work=torch.zeros(built_lib.griffinlim_rows_workspace_floats(B, F))),   # the smaller workspace
    ]
    try:
        built_lib._lib.taco_griffinlim_fast = lambda *a: called.append(a) or 0
        for kw in bad:
            with pytest.raises(ValueError):
                built_lib.griffinlim_fast(**kw)
        with pytest.raises(built_lib.TacoError):   # F < 5
            built_lib.griffinlim_fast(torch.ones(B, 1025, 4))
    finally:
        built_lib._lib.taco_griffinlim_fast = real
    assert not called
    sig = inspect.signature(built_lib.griffinlim_fast).parameters
    assert [(k, sig[k].default) for k in list(sig)[1:]] == [
        ('frames', None), ('phase0', None), ('seed', 0), ('n_iter', 50), ('momentum', 0.99), ('frames_per_unit', 1),
        ('want_conv', False), ('out', None), ('conv', None), ('work', None)]


def test_invert_spectrogram_and_driver_signatures(built_lib):
    from tacotron_amd import test as drv
    from tacotron_amd.griffinlim import invert_spectrogram
    p = inspect.signature(invert_spectrogram).parameters
    assert p['momentum'].default is None and p['want_conv'].default is False and p['n_iter'].default == 50
    d = inspect.signature(drv.test).parameters
    assert d['gl_momentum'].default is None and d['n_iter'].default == 50
    for kw in (dict(gl_momentum=1.0), dict(gl_momentum=-0.5), dict(n_iter=-1)):   # refused before anything is loaded or built
        with pytest.raises(ValueError):
            drv.test(None, [], **kw)
    with pytest.raises(ValueError):
        invert_spectrogram(None, None, None, 2, want_conv=True)


def test_driver_options(built_lib, capsys):
    from tacotron_amd import test as drv
    a = drv.parse_args([])
    assert a.gl_momentum is None and a.gl_iters == 50 and not a.stop and not a.vocode_lengths
    a = drv.parse_args(['--stop', '--vocode-lengths', '--gl-momentum', '0.99', '--gl-iters', '30'])
    assert a.gl_momentum == 0.99 and a.gl_iters == 30 and a.stop and a.vocode_lengths
    assert drv.parse_args(['--gl-momentum', '0']).gl_momentum == 0.0
    assert drv.parse_args(['--gl-iters', '0']).gl_iters == 0
    for argv in (['--gl-iters', '-1'], ['--gl-momentum', '1'], ['--gl-momentum', '1.2'], ['--gl-momentum', '-0.1'],
                 ['--gl-momentum', 'nan'], ['--gl-momentum', 'x'], ['--vocode-lengths', '--gl-momentum', '0.5']):
        with pytest.raises(SystemExit) as e:
            drv.parse_args(argv)
        assert e.value.code == 2, argv
    capsys.readouterr()


def _inputs(fn, F, seed):
    mag, ph = fgl_ref.fp32_inputs(fn, F, seed)
    return mag.astype(np.float64), ph.astype(np.float64)


def test_restatement_momentum_0_is_the_oracle():
    mag, ph = _inputs(fgl_ref.case, 8, 3)
    for n_iter in (0, 1, 3):
        w, conv = fgl_ref.griffinlim_fast(mag, ph, n_iter, 0.0)
        assert np.array_equal(w, gl.griffinlim(mag, ph, n_iter))
        assert conv.shape == (n_iter + 1,) and np.isfinite(conv).all()


def test_restatement_first_round_has_no_predecessor():
    mag, ph = _inputs(fgl_ref.case, 8, 3)
    for n_iter in (0, 1):
        w0, c0 = fgl_ref.griffinlim_fast(mag, ph, n_iter, 0.0)
        w9, c9 = fgl_ref.griffinlim_fast(mag, ph, n_iter, 0.99)
        assert np.array_equal(w0, w9) and np.array_equal(c0, c9)
    w0, _ = fgl_ref.griffinlim_fast(mag, ph, 2, 0.0)
    w9, _ = fgl_ref.griffinlim_fast(mag, ph, 2, 0.99)
    assert not np.array_equal(w0, w9)


def test_restatement_last_value_is_the_convergence_of_the_waveform():
    mag, ph = _inputs(fgl_ref.case, 12, 5)
    for n_iter, a in ((0, 0.0), (1, 0.5), (4, 0.99)):
        w, conv = fgl_ref.griffinlim_fast(mag, ph, n_iter, a)
        assert abs(conv[-1] - gl.spectral_convergence(w, mag)) < 1e-12
    # the first value is that of the initial phases
    assert abs(conv[0] - gl.spectral_convergence(gl.istft(mag * np.exp(1j * ph)), mag)) < 1e-12
    # a zero matrix has no convergence to speak of
    w, conv = fgl_ref.griffinlim_fast(np.zeros_like(mag), ph, 2, 0.99)
    assert not w.any() and not conv.any()


@pytest.mark.parametrize('name,fn,F,seed', fgl_ref.CASES, ids=[c[0] for c in fgl_ref.CASES])
def test_momentum_30_rounds_beat_plain_50(name, fn, F, seed):
    """the claim of DESIGN.md 4b, in fp64: momentum 0.99 / 30 rounds ends below the plain algorithm's 50 rounds"""
    mag, ph = _inputs(fn, F, seed)
    _, fast = fgl_ref.griffinlim_fast(mag, ph, 30, 0.99)
    _, plain = fgl_ref.griffinlim_fast(mag, ph, 50, 0.0)
    print('  %s: plain 0 / 50 rounds %.4f / %.4f, momentum 0.99 at 30 rounds %.4f (%.1f %% below)'
          % (name, plain[0], plain[-1], fast[-1], 100 * (1 - fast[-1] / plain[-1])))
    assert fast[0] == plain[0]
    assert fast[-1] < plain[-1]
