"""CPU checks of weight averaging (taco_param_ema): the header's declarations, lib.EXPORTS and the loaded symbols, the size function,
the warm-up of the decay, the NumPy restatement against TF's form of the update, the wrapper's refusals before any device call, and
the drivers' flags.  No compute call: there is no GPU here."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import ema_ref as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, 'include', 'taco_hip.h')
N_NANCY = 6926609


def _decl(hdr, name):
    """the argument list of the declaration of `name` (the one that ends in `);`), one normalised string per argument"""
    m = re.search(r'^(?:int|int64_t)\s+%s\s*\(([^;]*?)\)\s*;' % re.escape(name), hdr, re.M | re.S)
    assert m, 'no declaration of %s' % name
    return [' '.join(a.split()) for a in m.group(1).replace('\n', ' ').split(',')]


def test_header_exports_and_symbols(built_lib):
    hdr = open(HDR).read()
    assert _decl(hdr, 'taco_param_ema_workspace_bytes') == ['int64_t n']
    assert _decl(hdr, 'taco_param_ema') == ['float* ema', 'const float* params', 'int64_t n', 'float w', 'const int32_t* err_words',
                                            'double* stats', 'void* workspace', 'void* stream']
    assert re.search(r'^int64_t\s+taco_param_ema_workspace_bytes', hdr, re.M) and re.search(r'^int\s+taco_param_ema\s*\(', hdr, re.M)
    C = ctypes
    P = C.c_void_p
    assert built_lib.EXPORTS['taco_param_ema_workspace_bytes'] == (C.c_int64, [C.c_int64])
    assert built_lib.EXPORTS['taco_param_ema'] == (C.c_int, [P, P, C.c_int64, C.c_float, P, P, P, P])
    raw = C.CDLL(built_lib.LIB_PATH)
    assert hasattr(raw, 'taco_param_ema') and hasattr(raw, 'taco_param_ema_workspace_bytes')
    assert built_lib.version() == 120 and int(re.search(r'#define\s+TACO_VERSION\s+(\d+)', hdr).group(1)) == 120
    block = ' '.join(hdr[hdr.index('weight averaging (ema.hip)'):hdr.index('int64_t taco_param_ema_workspace_bytes(int64_t n);')].split())
    for said in ('d = params[i] - ema[i]', 't = w * d', 'ema[i] = ema[i] + t', 'err_words', '(-1, -1, 0)', 'no atomics', 'Not here',
                 'detect them by the symbol'):
        assert said in block, said


def test_workspace_bytes(built_lib):
    assert built_lib.param_ema_workspace_bytes(1) > 0
    assert built_lib.param_ema_workspace_bytes(N_NANCY) > 0
    assert built_lib.param_count(built_lib.make_shape(32, 200, 180, 2, 60)) == N_NANCY
    for bad in (0, -1):
        with pytest.raises(built_lib.TacoError):
            built_lib.param_ema_workspace_bytes(bad)


@pytest.mark.parametrize('decay', [0.999, 0.9999, 0.9])
def test_ema_decay_warm_up(built_lib, decay):
    assert built_lib.ema_decay(decay, 0) == 0.1 and built_lib.ema_decay(decay, 8) == 0.5
    assert built_lib.ema_decay(decay, 10 ** 9) == decay
    vals = [built_lib.ema_decay(decay, k) for k in range(0, 200000, 7)]
    assert all(a <= b for a, b in zip(vals, vals[1:])) and vals[-1] == decay and all(0.0 < v <= decay for v in vals)
    for k in (0, 1, 8, 9, 8990, 8991, 8992, 10 ** 6):
        assert built_lib.ema_decay(decay, k) == er.ema_decay(decay, k)
        w = built_lib.ema_weight(decay, k)
        assert isinstance(w, np.float32) and w == np.float32(1.0 - er.ema_decay(decay, k)) == er.ema_weight(decay, k)
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError):
            built_lib.ema_decay(decay, bad)
    for bad in (-0.1, 1.5, float('nan'), None):
        with pytest.raises(ValueError):
            built_lib.ema_decay(bad, 0)


@pytest.mark.parametrize('w', [0.001, 0.9, 0.1, 0.0, 1.0, 1.0 - 0.999])
def test_the_restatement_is_tf_s_update_bit_for_bit(w):
    rng = np.random.default_rng(3)
    p = (rng.standard_normal(200003) * 0.1).astype(np.float32)
    e = (p + rng.standard_normal(p.size).astype(np.float32) * np.float32(1e-3)).astype(np.float32)
    e[::11] = p[::11]
    p[::13] = 0.0
    e[::17] = 0.0
    got, tf = er.ema_update(e, p, np.float32(w)), er.ema_update_tf(e, p, np.float32(w))
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), tf.view(np.uint32))
    if w == 0.0:
        assert np.array_equal(got, e)
    same = e == p
    assert np.array_equal(got[same], e[same])
    # the three operations, element by element, on Python's doubles rounded back after each one
    i = rng.integers(0, p.size, 2000)
    f32 = np.float32
    one = [f32(f32(e[k]) + f32(f32(w) * f32(f32(p[k]) - f32(e[k])))) for k in i]
    assert np.array_equal(np.array(one, dtype=np.float32).view(np.uint32), got[i].view(np.uint32))
    d2, p2 = er.ema_stats(e, p)
    assert d2 > 0.0 and abs(p2 - float(np.sum(p.astype(np.float64) ** 2))) <= 1e-9 * p2


def test_refusals_come_from_the_argument_checks(built_lib, monkeypatch):
    lib = built_lib

    class NoCall(object):   # any call into the library from here on is a failure of the test
        def __getattr__(self, name):
            raise AssertionError('the library was called (%s) although an argument is bad' % name)

    monkeypatch.setattr(lib, '_lib', NoCall())
    e, p = torch.zeros(64), torch.ones(64)
    cases = [
        (dict(ema=e, params=p, w=0.5), 'must be on the GPU'),                                     # CPU tensors
        (dict(ema=e, params=torch.ones(63), w=0.5), 'params'),                                    # mismatched lengths
        (dict(ema=e.double(), params=p, w=0.5), 'ema'),                                           # float64
        (dict(ema=e, params=p.double(), w=0.5), 'params'),
        (dict(ema=e, params=e[:], w=0.5), 'may not overlap'),                                     # overlapping views
        (dict(ema=torch.zeros(100)[:64], params=p, w=-0.1), 'w must be'),
        (dict(ema=e, params=p, w=1.5), 'w must be'),
        (dict(ema=e, params=p, w=float('nan')), 'w must be'),
        (dict(ema=torch.zeros(8, 8), params=torch.ones(8, 8), w=0.5), 'ema'),                     # not flat
        (dict(ema=torch.zeros(128)[::2], params=p, w=0.5), 'ema'),                                # not contiguous
        (dict(ema=e, params=p, w=0.5, err_words=torch.zeros(2, dtype=torch.int64)), 'err_words'),
        (dict(ema=e, params=p, w=0.5, stats=torch.zeros(3)), 'stats'),
        (dict(ema=e, params=p, w=0.5, stats=torch.zeros(3, dtype=torch.float64), workspace=torch.zeros(8)), 'workspace'),
    ]
    big = torch.zeros(100)
    cases.append((dict(ema=big[:64], params=big[32:96], w=0.5), 'may not overlap'))
    for kw, said in cases:
        with pytest.raises(ValueError, match='param_ema: .*%s' % re.escape(said)):
            lib.param_ema(**kw)
    assert list(inspect.signature(lib.param_ema).parameters) == ['ema', 'params', 'w', 'err_words', 'stats', 'workspace']


def test_flags_and_defaults():
    from tacotron_amd import evaluate as ev, model, test as drv, train
    from tacotron_amd.config import Config
    assert Config.ema_decay == 0.0 and Config.use_ema is False
    c = Config()
    c.validate()
    for bad in (1.0, -0.5, float('nan')):
        c.ema_decay = bad
        with pytest.raises(ValueError, match='ema_decay'):
            c.validate()
    assert train.parse_args([]).ema is None and train.parse_args(['--ema', '0.999']).ema == 0.999
    for bad in ('0', '1', '1.5', '-0.1', 'nan'):
        with pytest.raises(SystemExit):
            train.parse_args(['--ema', bad])
    assert inspect.signature(train.train).parameters['ema'].default is None
    assert inspect.signature(model.Tacotron.step).parameters['ema_stats'].default is False
    assert inspect.signature(model.Tacotron.load_state_dict).parameters['use_ema'].default is False
    assert drv.parse_args([]).ema is False and drv.parse_args(['--ema', '--checkpoint', 'x']).ema is True
    with pytest.raises(SystemExit):
        drv.parse_args(['--ema'])
    assert ev.parse_args([]).ema is False and ev.parse_args(['--ema']).ema is True
    assert inspect.signature(ev.evaluate).parameters['ema'].default is False
    assert train.ema_line(0.999, 0, [4.0, 16.0, 1.0]) == 'ema decay 0.100000 lag 5.000e-01'
    assert train.ema_line(0.999, 10 ** 6, [1.0, 1e6, 1.0]) == 'ema decay 0.999000 lag 1.000e-03'
    assert 'skipped' in train.ema_line(0.999, 3, [-1.0, -1.0, 0.0])
    assert 'no collective' in ' '.join(__import__('tacotron_amd.dist', fromlist=['x']).__doc__.split())
