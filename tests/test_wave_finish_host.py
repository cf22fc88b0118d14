"""CPU checks of waveform finishing (taco_wave_finish): the C ABI declaration and its version, the exports and their ctypes
signature, the workspace query, the Python binding's argument checks, the driver's options, the rule that turns decoder steps into
samples, write_wav_pcm, and the fp64 restatement (tests/wave_ref.py) the GPU tests compare against."""
import ctypes as C
import inspect
import os
import re
import wave as wavefile

import numpy as np
import pytest
import torch

from tests import audio_ref, wave_ref as wr

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'taco_hip.h')


def _args(decl):
    return [' '.join(a.split()) for a in decl.replace('\n', ' ').split(',')]


def test_header_declares_both_entry_points():
    hdr = open(HDR).read()
    ws = re.search(r'int64_t taco_wave_finish_workspace_bytes\(([^)]*)\);', hdr)
    assert ws and _args(ws.group(1)) == ['int B', 'int L']
    fn = re.search(r'\bint taco_wave_finish\(([^)]*)\);', hdr)
    assert fn
    assert _args(fn.group(1)) == ['const float* wave', 'const int32_t* samples', 'float deemphasis', 'float trim_top_db', 'float* out',
                                  'int16_t* pcm', 'int32_t* bounds', 'float* peak', 'void* workspace', 'int B', 'int L', 'void* stream']
    assert int(re.search(r'#define\s+TACO_VERSION\s+(\d+)', hdr).group(1)) == 120
    assert 'detect them by the' in hdr and 'librosa.effects.trim' in hdr


def test_library_exports_them_at_version_120(built_lib):
    assert built_lib.version() == 120
    for name in ('taco_wave_finish_workspace_bytes', 'taco_wave_finish'):
        assert name in built_lib.EXPORTS
        assert hasattr(C.CDLL(built_lib.LIB_PATH), name)
    res, args = built_lib.EXPORTS['taco_wave_finish']
    P, I, F = C.c_void_p, C.c_int, C.c_float
    assert res is C.c_int and args == [P, P, F, F, P, P, P, P, P, I, I, P]
    assert built_lib.EXPORTS['taco_wave_finish_workspace_bytes'] == (C.c_int64, [I, I])


def test_workspace_query(built_lib):
    """room for the scanned signal at least, linear in B, and refusals for B <= 0 or L <= 0"""
    for B, L in ((1, 1), (1, 2047), (5, 107700), (32, 107700)):
        n = built_lib.wave_finish_workspace_floats(B, L)
        assert B * L <= n <= B * (L + 4 + 3 * (L // 512 + 2)) + 64
    assert (built_lib.wave_finish_workspace_floats(8, 107700) - built_lib.wave_finish_workspace_floats(4, 107700)
            == built_lib.wave_finish_workspace_floats(5, 107700) - built_lib.wave_finish_workspace_floats(1, 107700))
    raw = built_lib._lib.taco_wave_finish_workspace_bytes
    for B, L in ((0, 100), (-1, 100), (2, 0), (2, -7)):
        assert raw(B, L) == -1
        with pytest.raises(built_lib.TacoError):
            built_lib.wave_finish_workspace_floats(B, L)


def test_wrapper_refuses_bad_arguments_before_any_device_call(built_lib):
    """every refusal is raised on the host before the entry point is called (CPU tensors never reach it)"""
    B, L = 2, 600
    w = torch.zeros(B, L)
    sm = torch.tensor([600, 300], dtype=torch.int32)
    called = []
    real = built_lib._lib.taco_wave_finish
    bad = [
        dict(wave=torch.zeros(L)),                                         # no batch dimension
        dict(wave=torch.zeros(B, L, 1)),
        dict(wave=torch.zeros(B, 0)),                                      # no samples
        dict(wave=w.double()),                                             # not float32
        dict(wave=torch.zeros(L, B).t()),                                  # not contiguous
        dict(wave=w, samples=sm.long()),                                   # int64 counts
        dict(wave=w, samples=torch.tensor([1, 2, 3], dtype=torch.int32)),  # B + 1 counts
        dict(wave=w, samples=sm.view(B, 1)),
        dict(wave=w, deemphasis=-0.01),
        dict(wave=w, deemphasis=1.0),
        dict(wave=w, deemphasis=1.5),
        dict(wave=w, deemphasis=float('nan')),
        dict(wave=w, deemphasis=1.0 - 1e-12),                              # 1 once it is a float
        dict(wave=w, trim_top_db=-1.0),
        dict(wave=w, trim_top_db=float('nan')),
        dict(wave=w, want_out=False, want_pcm=False),                      # nothing to emit
        dict(wave=w, out=w),                                               # in place
        dict(wave=w, out=torch.zeros(B, L + 1)),
        dict(wave=w, out=torch.zeros(B, L, dtype=torch.float64)),
        dict(wave=w, pcm=torch.zeros(B, L, dtype=torch.int32)),
        dict(wave=w, pcm=torch.zeros(B * L, dtype=torch.int16)),
        dict(wave=w, bounds=torch.zeros(B, dtype=torch.int32)),
        dict(wave=w, bounds=torch.zeros(B, 2, dtype=torch.int64)),
        dict(wave=w, peak=torch.zeros(B, 1)),
        dict(wave=w, peak=torch.zeros(B, dtype=torch.float64)),
        dict(wave=w, work=torch.zeros(built_lib.wave_finish_workspace_floats(B, L) - 1)),
    ]
    try:
        built_lib._lib.taco_wave_finish = lambda *a: called.append(a) or 0
        for kw in bad:
            with pytest.raises(ValueError):
                built_lib.wave_finish(**kw)
    finally:
        built_lib._lib.taco_wave_finish = real
    assert not called
    sig = inspect.signature(built_lib.wave_finish).parameters
    assert [(k, sig[k].default) for k in list(sig)[1:]] == [
        ('samples', None), ('deemphasis', 0.97), ('trim_top_db', 0.0), ('want_out', True), ('want_pcm', True), ('out', None),
        ('pcm', None), ('bounds', None), ('peak', None), ('work', None)]


def test_driver_options(built_lib, capsys):
    from tacotron_amd import test as drv
    a = drv.parse_args([])
    assert a.deemphasis is None and a.trim_db is None
    assert drv.parse_args(['--deemphasis']).deemphasis == 0.97
    assert drv.parse_args(['--deemphasis', '0.9']).deemphasis == 0.9
    assert drv.parse_args(['--deemphasis', '0']).deemphasis == 0.0
    a = drv.parse_args(['--stop', '--vocode-lengths', '--gl-momentum', '0.99', '--gl-iters', '30', '--trim-db', '40', '--deemphasis'])
    assert a.deemphasis == 0.97 and a.trim_db == 40.0 and a.stop and a.vocode_lengths and a.gl_momentum == 0.99 and a.gl_iters == 30
    for argv in (['--deemphasis', '1'], ['--deemphasis', '-0.1'], ['--deemphasis', 'nan'], ['--deemphasis', 'x'], ['--trim-db'],
                 ['--trim-db', '0'], ['--trim-db', '-3'], ['--trim-db', 'nan'], ['--trim-db', 'x']):
        with pytest.raises(SystemExit) as e:
            drv.parse_args(argv)
        assert e.value.code == 2, argv
    capsys.readouterr()
    d = inspect.signature(drv.test).parameters
    assert d['deemphasis'].default is None and d['trim_db'].default is None
    for kw in (dict(deemphasis=1.0), dict(deemphasis=-0.5), dict(deemphasis=float('nan')), dict(trim_db=0.0), dict(trim_db=-1.0),
               dict(trim_db=float('nan'))):   # refused before anything is loaded or built
        with pytest.raises(ValueError):
            drv.test(None, [], **kw)


def test_samples_rule_of_finish_waveform(built_lib):
    """F = L / 300 + 1, F_b = min(F, lengths * r), n_b = F_b < 5 ? 0 : 300 (F_b - 1) -- on CPU tensors, against the table"""
    from tacotron_amd.griffinlim import finish_samples, finish_waveform
    F = 360
    L = 300 * (F - 1)
    table = {0: 0, 1: 0, 4: 0, 5: 1200, 6: 1500, 359: 107400, 360: 107700, 361: 107700, 10000: 107700}   # F_b (before the cap) -> n_b
    fb = sorted(table)
    got = finish_samples(torch.tensor(fb, dtype=torch.int32), 1, L)
    assert got.dtype == torch.int32 and got.tolist() == [table[k] for k in fb]
    for r in (2, 3, 5):
        lengths = torch.tensor([0, 1, 2, 3, 72, 100, 180, 1 << 28, -4], dtype=torch.int32)
        want = [0 if min(F, int(n) * r) < 5 else 300 * (min(F, int(n) * r) - 1) for n in lengths]
        assert finish_samples(lengths, r, L).tolist() == want
    # the wrapper hands exactly these to the binding
    seen = []
    real = built_lib.wave_finish
    try:
        built_lib.wave_finish = lambda wave, samples, **k: seen.append((samples, k)) or (None, None, None, None)
        w = torch.zeros(3, 300 * 23)
        finish_waveform(w, torch.tensor([12, 2, 40], dtype=torch.int32), 2, deemphasis=0.9, trim_top_db=25.0)
        finish_waveform(w)
        for bad in (dict(lengths=torch.tensor([1, 2, 3])), dict(lengths=torch.tensor([1, 2], dtype=torch.int32)),
                    dict(lengths=torch.tensor([1, 2, 3], dtype=torch.int32), r=0)):
            with pytest.raises(ValueError):
                finish_waveform(w, **bad)
    finally:
        built_lib.wave_finish = real
    assert len(seen) == 2
    assert seen[0][0].tolist() == [6900, 0, 6900] and seen[0][1]['deemphasis'] == 0.9 and seen[0][1]['trim_top_db'] == 25.0
    assert seen[1][0] is None and seen[1][1]['deemphasis'] == 0.97 and seen[1][1]['trim_top_db'] == 0.0
    p = inspect.signature(finish_waveform).parameters
    assert [(k, p[k].default) for k in list(p)[1:5]] == [('lengths', None), ('r', 1), ('deemphasis', 0.97), ('trim_top_db', 0.0)]


def test_write_wav_pcm_round_trips(built_lib, tmp_path):
    from tacotron_amd import test as drv
    rng = np.random.default_rng(2)
    x = rng.integers(-32768, 32768, size=4001).astype(np.int16)
    x[:4] = [-32768, 32767, 0, -1]
    for name, arr in (('a.wav', x), ('b.wav', x[::2]), ('empty.wav', x[:0])):   # (a strided view as well)
        path = str(tmp_path / name)
        drv.write_wav_pcm(path, arr)
        with wavefile.open(path) as f:
            assert (f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()) == (1, 2, 16000, len(arr))
            assert np.array_equal(np.frombuffer(f.readframes(len(arr)), dtype='<i2'), arr)
    for bad in (x.astype(np.float32), x.astype(np.int32), x.reshape(1, -1)):
        with pytest.raises(ValueError):
            drv.write_wav_pcm(str(tmp_path / 'bad.wav'), bad)


# ---- the restatement's own properties ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('a', [0.97, 0.5, 0.0])
def test_preemphasis_inverts_the_restatement(a):
    for f in wr.FAMILIES:
        x = wr.family(f, 20000).astype(np.float64)
        y = wr.deemphasis(x, a)
        assert np.abs(wr.preemphasis(y, a) - x).max() <= 1e-12
        assert y[0] == x[0]
    assert np.array_equal(wr.deemphasis(x, 0.0), x)
    assert len(wr.deemphasis(x[:0], a)) == 0 and len(wr.preemphasis(x[:0], a)) == 0


def test_error_bound_grows_with_the_signal():
    x = wr.family('bursts', 20000)
    E = wr.error_bound(x, 0.97)
    assert (E > 0).all() and np.isfinite(E).all()
    assert np.allclose(wr.error_bound(3.0 * x.astype(np.float64), 0.97), 3.0 * E, rtol=1e-12, atol=1e-29)
    bigger = x.copy()
    bigger[5000] += 1.0
    Eb = wr.error_bound(bigger, 0.97)
    assert (Eb >= E).all() and (Eb[5000:5100] > E[5000:5100]).all() and np.array_equal(Eb[:5000], E[:5000])
    assert (wr.error_bound(x, 0.97, const=8.0) < E).all()
    assert wr.error_bound(np.zeros(10, np.float32), 0.97).max() == 1e-30
    # S and T against their closed forms on an impulse: S[n] = a^n, T[n] = n a^n
    a = wr.coeff(0.97)
    imp = np.zeros(50)
    imp[0] = 1.0
    n = np.arange(50)
    assert np.allclose(wr.error_bound(imp, 0.97) - 1e-30, wr.U * (16 * a ** n + 2 * n * a ** n), rtol=1e-12)
    # a sequential fp32 evaluation sits well inside the bound; one with the wrong coefficient far outside
    x = wr.family('same_sign', 20000)
    y64 = wr.deemphasis(x, 0.97)
    E = wr.error_bound(x, 0.97)

    def seq32(c):
        acc, out = np.float32(0), np.zeros(len(x), np.float32)
        for i, v in enumerate(x):
            acc = np.float32(v + np.float32(np.float32(c) * acc))
            out[i] = acc
        return out
    assert (np.abs(seq32(0.97) - y64) / E).max() < 0.5
    assert (np.abs(seq32(0.9699) - y64) / E).max() > 100


def test_trim_restatement():
    """at 60 dB it is tests/audio_ref.py's trim; the GPU test's inputs keep every frame 1 dB from every threshold they use"""
    expect = {107700: {60.0: (19456, 71680), 40.0: (19456, 71168), 25.0: (19456, 71168)},
              59700: {60.0: (7168, 59700), 40.0: (7168, 59700), 25.0: (7168, 59700)},
              5000: {60.0: (512, 4608), 40.0: (512, 4608), 25.0: (512, 4608)}}
    for L, (s, e), floor, dbs in wr.TRIM_CASES:
        y = wr.deemphasis(wr.burst(L, s, e, floor), 0.97)
        assert wr.trim_bounds(y, 60.0) == audio_ref.trim_bounds(y)
        assert 4.0 < np.abs(y).max() < 7.0
        for db in dbs:
            assert wr.trim_margin(y, db) >= 1.0, (L, db)
            assert wr.trim_bounds(y, db) == expect[L][db], (L, db)
        assert wr.trim_bounds(y, 0.0) == (0, L)
    assert wr.trim_bounds(np.zeros(3000), 40.0) == (0, 3000)        # all 0 dB: not trimmed
    assert wr.trim_bounds(np.zeros(0), 40.0) == (0, 0)
    for n in (1, 511, 512, 2047):
        assert wr.trim_bounds(np.ones(n), 40.0) == (0, n)
        assert len(wr.frame_db(np.ones(n))) == 1 + n // 512
    assert wr.finish(np.zeros(0, np.float32), 0.97, 40.0)[1:] == ((0, 0), 0.0)


def test_pcm_restatements_agree_to_one_lsb():
    rng = np.random.default_rng(4)
    for scale in (0.2, 2.5):
        y = (scale * rng.standard_normal(5000)).astype(np.float32)
        peak = np.abs(y).max()
        q32, q64 = wr.pcm_fp32(y, peak), wr.pcm_write_wav(y)
        assert q32.dtype == np.int16 and np.abs(q32.astype(np.int32) - q64.astype(np.int32)).max() <= 1
        assert (peak > 1) == (scale > 1)
        assert (np.abs(q32.astype(np.int32)).max() == 32767) == (scale > 1)
    assert np.array_equal(wr.pcm_fp32(np.array([0.5, -0.5, 0.99999], np.float32), 0.99999), [16383, -16383, 32766])
