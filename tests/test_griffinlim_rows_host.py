"""CPU checks of Griffin-Lim per utterance (taco_griffinlim_rows): the C ABI declaration and its version, the Python binding's
argument checks, and the NumPy restatement of the device phase hash (tests/phase_ref.py) against known values."""
import os
import re

import numpy as np
import pytest
import torch

from tests.phase_ref import phase_angles, phase_hash, phase_u, splitmix64

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'taco_hip.h')


def _args(decl):
    return [' '.join(a.split()) for a in decl.replace('\n', ' ').split(',')]


def test_header_declares_both_entry_points():
    hdr = open(HDR).read()
    ws = re.search(r'int64_t taco_griffinlim_rows_workspace_bytes\(([^)]*)\);', hdr)
    assert ws and _args(ws.group(1)) == ['int B', 'int F']
    fn = re.search(r'\bint taco_griffinlim_rows\(([^)]*)\);', hdr)
    assert fn
    assert _args(fn.group(1)) == ['const float* mag_t', 'const float* phase0', 'uint64_t seed', 'const int32_t* frames',
                                  'int frames_per_unit', 'float* wave', 'void* workspace', 'int B', 'int F', 'int n_iter',
                                  'void* stream']
    assert int(re.search(r'#define\s+TACO_VERSION\s+(\d+)', hdr).group(1)) == 120


def test_library_exports_them_at_version_120(built_lib):
    import ctypes as C
    assert built_lib.version() == 120
    for name in ('taco_griffinlim_rows_workspace_bytes', 'taco_griffinlim_rows'):
        assert name in built_lib.EXPORTS
        assert hasattr(C.CDLL(built_lib.LIB_PATH), name)
    res, args = built_lib.EXPORTS['taco_griffinlim_rows']
    assert res is C.c_int and len(args) == 11 and args[2] is C.c_uint64 and args[4] is C.c_int
    assert built_lib.EXPORTS['taco_griffinlim_rows_workspace_bytes'] == (C.c_int64, [C.c_int, C.c_int])


def test_workspace_size(built_lib):
    """angles (B, F, 1025, 2) + segments (B, F, 1200) + one window table of 2048 + 300 (F - 1) floats PER ROW; bad shapes refused"""
    for B, F in ((1, 5), (5, 41), (32, 360)):
        n = built_lib.griffinlim_rows_workspace_floats(B, F)
        assert n >= B * F * 1025 * 2 + B * F * 1200 + B * (2048 + 300 * (F - 1))
        assert n - built_lib.griffinlim_workspace_floats(B, F) == (B - 1) * (2048 + 300 * (F - 1))
    for B, F in ((0, 41), (-1, 41), (2, 4), (2, 0)):
        with pytest.raises(built_lib.TacoError):
            built_lib.griffinlim_rows_workspace_floats(B, F)


def test_wrapper_refuses_wrong_shapes_and_dtypes(built_lib):
    """every refusal is raised on the host before the library is called (CPU tensors never reach it)"""
    B, F = 2, 8
    mag = torch.ones(B, 1025, F)
    frames = torch.tensor([8, 5], dtype=torch.int32)
    bad = [
        dict(mag_t=torch.ones(B, 1024, F), frames=frames),                      # not 1025 bins
        dict(mag_t=torch.ones(1025, F), frames=frames),                         # no batch dimension
        dict(mag_t=mag.double(), frames=frames),                                # not float32
        dict(mag_t=mag, frames=frames.long()),                                  # int64 lengths
        dict(mag_t=mag, frames=torch.tensor([8, 5, 5], dtype=torch.int32)),     # B + 1 lengths
        dict(mag_t=mag, frames=frames.view(B, 1)),                              # (B, 1)
        dict(mag_t=mag, frames=frames, phase0=torch.zeros(B, 1025, F + 1)),     # phases of another shape
        dict(mag_t=mag, frames=frames, phase0=torch.zeros(B, 1025, F, dtype=torch.float64)),
        dict(mag_t=mag, frames=frames, frames_per_unit=0),
        dict(mag_t=mag, frames=frames, n_iter=-1),
        dict(mag_t=mag, frames=frames, out=torch.zeros(B, 300 * F)),            # waveform buffer of the wrong length
        dict(mag_t=mag, frames=frames, work=torch.zeros(built_lib.griffinlim_workspace_floats(B, F))),   # the smaller workspace
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            built_lib.griffinlim_rows(**kw)
    with pytest.raises(built_lib.TacoError):   # F < 5
        built_lib.griffinlim_rows(torch.ones(B, 1025, 4), frames)


def test_plain_wrapper_refuses_bad_arguments_before_any_device_call(built_lib):
    """lib.griffinlim, the oldest wrapper, refuses through the same check as the two above: ValueError (it used to assert, and to
    dereference phase0=None), before the entry point is called"""
    import inspect
    B, F = 2, 8
    mag, ph = torch.ones(B, 1025, F), torch.zeros(B, 1025, F)
    called = []
    real = built_lib._lib.taco_griffinlim
    bad = [
        dict(mag_t=torch.ones(B, 1024, F), phase0=torch.zeros(B, 1024, F)),    # not 1025 bins
        dict(mag_t=torch.ones(1025, F), phase0=torch.zeros(1025, F)),           # no batch dimension
        dict(mag_t=mag.double(), phase0=ph),                                    # not float32
        dict(mag_t=mag, phase0=None),
        dict(mag_t=mag, phase0=torch.zeros(B, 1025, F + 1)),                    # phases of another shape
        dict(mag_t=mag, phase0=ph.double()),
        dict(mag_t=mag, phase0=ph, n_iter=-1),
        dict(mag_t=mag, phase0=ph, out=torch.zeros(B, 300 * F)),                # waveform buffer of the wrong length
        dict(mag_t=mag, phase0=ph, work=torch.zeros(built_lib.griffinlim_workspace_floats(B, F) - 1)),   # too small a workspace
    ]
    try:
        built_lib._lib.taco_griffinlim = lambda *a: called.append(a) or 0
        for kw in bad:
            with pytest.raises(ValueError):
                built_lib.griffinlim(**kw)
        with pytest.raises(built_lib.TacoError):   # F < 5
            built_lib.griffinlim(torch.ones(B, 1025, 4), torch.zeros(B, 1025, 4))
    finally:
        built_lib._lib.taco_griffinlim = real
    assert not called
    sig = inspect.signature(built_lib.griffinlim).parameters
    assert [(k, sig[k].default) for k in list(sig)[2:]] == [('n_iter', 50), ('out', None), ('work', None)]
    assert list(sig)[:2] == ['mag_t', 'phase0'] and all(sig[k].default is inspect.Parameter.empty for k in list(sig)[:2])


def test_invert_spectrogram_and_driver_signatures(built_lib):
    import inspect
    from tacotron_amd import test as drv
    from tacotron_amd.griffinlim import invert_spectrogram
    assert inspect.signature(invert_spectrogram).parameters['lengths'].default is None
    assert inspect.signature(drv.test).parameters['vocode_lengths'].default is False
    with pytest.raises(ValueError):   # refused before anything is loaded or built
        drv.test(None, [], vocode_lengths=True)


def test_splitmix64_known_values():
    assert int(splitmix64(np.uint64(0))) == 0xE220A8397B1DCDAF          # the generator's published first output (state 0)
    # the next outputs of the same stream: state advances by the golden-ratio increment
    g = np.uint64(0x9E3779B97F4A7C15)
    with np.errstate(over='ignore'):
        assert int(splitmix64(g)) == 0x6E789E6AA1B965F4
        assert int(splitmix64(g + g)) == 0x06C45D188009454F


def test_phase_hash_known_values():
    h = phase_hash(5, 2, 41)
    u = phase_u(5, 2, 41)
    assert h.shape == u.shape == (2, 1025, 41)
    assert int(h[0, 0, 0]) == 0x3B95E0342328EDF3 and int(u[0, 0, 0]) == 3904992
    assert int(h[1, 1024, 40]) == 0xF4E3DCC441496511 and int(u[1, 1024, 40]) == 16049116
    # element (b, k, t) is the flat index of the (B, 1025, F) matrix
    with np.errstate(over='ignore'):
        base = np.uint64(5) * np.uint64(0xD1342543DE82EF95)
        i = np.uint64((1 * 1025 + 7) * 41 + 3)
        assert int(h[1, 7, 3]) == int(splitmix64(base + i))
    assert u.min() >= 0 and u.max() < (1 << 24)
    a = phase_angles(5, 2, 41)
    assert a.min() >= 0.0 and a.max() < 2 * np.pi and a[0, 0, 0] == 2 * np.pi * 3904992 / 2 ** 24
    # 2 u / 2^24, the argument the device gives sincospif, is exact in fp32
    x = (u.astype(np.float32) * np.float32(2.0 / 16777216.0)).astype(np.float64)
    assert np.array_equal(x, u / float(1 << 23))
    # 24 uniform bits: mean and spread of a uniform variable, and another seed gives other values
    assert abs(u.mean() / 2 ** 24 - 0.5) < 0.005 and abs(u.std() / 2 ** 24 - 12 ** -0.5) < 0.005
    assert (phase_u(6, 2, 41) != u).mean() > 0.99
