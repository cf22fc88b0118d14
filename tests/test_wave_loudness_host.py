"""CPU: the host side of taco_wave_loudness (include/taco_hip.h) -- taco_k_weighting against the standard's 48 kHz table and the
restatement's closed forms, the fp64 restatement (tests/loudness_ref.py) on the compliance signals it can be held to without a
listener (a full-scale 997 Hz sine, a gating case), its edge rows, the wrappers' argument checks and the driver's options."""
import inspect
import math

import numpy as np
import pytest
import torch

from tests import loudness_ref as lr


def test_k_weighting_is_the_table_of_the_standard(built_lib):
    got = built_lib.k_weighting(48000)
    assert len(got) == 10
    for g, w in zip(got, lr.TABLE_48K):
        assert abs(g - w) <= 1e-12, (g, w)


@pytest.mark.parametrize('sr', [16000, 22050, 24000])
def test_k_weighting_is_the_closed_form(built_lib, sr):
    got, want = built_lib.k_weighting(sr), lr.k_weighting(sr)
    for g, w in zip(got, want):
        assert abs(g - w) <= 1e-15 * max(1.0, abs(w)), (sr, g, w)
    assert got[5:8] == [1.0, -2.0, 1.0]


@pytest.mark.parametrize('sr', [7999, 16005, 48010, 7990, 0, -16000])
def test_k_weighting_refuses_other_rates(built_lib, sr):
    with pytest.raises(ValueError, match='k_weighting'):
        built_lib.k_weighting(sr)
    import ctypes as C
    fn = C.CDLL(built_lib.LIB_PATH).taco_k_weighting
    fn.restype, fn.argtypes = built_lib.EXPORTS['taco_k_weighting']
    coef = (C.c_double * 10)(*([7.0] * 10))
    assert fn(sr, coef) == -1 and list(coef) == [7.0] * 10
    assert 'k_weighting' in built_lib.last_error()
    with pytest.raises(built_lib.TacoError):
        built_lib.wave_loudness_workspace_floats(1, 100, sr)


def test_workspace_size_function(built_lib):
    assert built_lib.LOUD_CHUNK == 2048
    assert built_lib.wave_loudness_workspace_floats(1, 1, 8000) > 0
    big = built_lib.wave_loudness_workspace_floats(32, 107700, 16000)
    assert big >= 32 * 107700 and big < 34 * 107700
    for B, L in ((0, 100), (-1, 100), (2, 0), (2, -3)):
        with pytest.raises(built_lib.TacoError):
            built_lib.wave_loudness_workspace_floats(B, L, 16000)


def test_full_scale_sine_reads_minus_3_01():
    """a full-scale 997 Hz sine of 20 s reads -3.01 LUFS at 48 kHz; at 16 and 24 kHz it stays inside the +-0.1 LU of EBU Tech 3341"""
    at48 = lr.measure(lr.sine(48000, 20), 48000)['I']
    print('  48 kHz: %.4f LUFS' % at48)
    assert abs(at48 - (-3.0103)) <= 1e-4 and round(at48, 2) == -3.01
    for sr, found in ((16000, -2.9701), (24000, -2.9843)):
        r = lr.measure(lr.sine(sr, 20), sr)
        print('  %d Hz: %.4f LUFS, M %.4f' % (sr, r['I'], r['M']))
        assert abs(r['I'] - (-3.01)) <= 0.1 and abs(r['I'] - found) <= 1e-4
        assert r['blocks'] == (197, 197, 197) and abs(r['M'] - r['I']) < 0.011   # (a block holds ~400 periods: its edges weigh 1 / 400)


def test_gating_case():
    """10 s of 0.1 sin, 5 s of zeros, 5 s of 0.001 sin at 16 kHz: blocks (197, 151, 100), I = -23.036 against -22.970 for the tone"""
    r = lr.measure(lr.gating_case(), 16000)
    tone = lr.measure(lr.sine(16000, 10, 0.1), 16000)
    print('  blocks %s, I %.4f, tone alone %.4f, nearest block %.3f LU from a gate' % (r['blocks'], r['I'], tone['I'], r['margin']))
    assert r['blocks'] == (197, 151, 100)
    assert abs(r['I'] - (-23.036)) <= 5e-4 and abs(tone['I'] - (-22.970)) <= 5e-4
    assert r['margin'] >= 0.05


def test_restatement_edge_rows():
    sr, H = 16000, 1600
    x = 0.1 * np.random.default_rng(2).standard_normal(5 * H)
    for n, nb in ((0, 0), (1, 1), (H - 1, 1), (4 * H - 1, 1), (4 * H, 1), (4 * H + 1, 1), (5 * H, 2)):
        r = lr.level(x[:n], sr, -23.0, 1.0)
        assert r['blocks'][0] == nb, (n, r['blocks'])
        if n == 0:
            assert r['I'] == -math.inf and r['M'] == -math.inf and r['g'] == 1.0 and r['peak_out'] == 0.0 and r['out'].size == 0
        else:
            y = lr.k_filter(x[:n], sr)
            if n < 4 * H:   # one block over all samples
                assert r['z'][0] == np.sum(y * y) / n
            assert r['blocks'] == (nb, nb, nb) and r['I'] <= r['M'] + 1e-12
            assert abs(r['I'] + 20 * math.log10(r['g']) - (-23.0)) < 1e-9 and r['limited'] == 0
    # an all-zero row passes unchanged
    r = lr.level(np.zeros(3 * H), sr, -23.0, 0.5)
    assert r['blocks'] == (1, 0, 0) and r['I'] == -math.inf and r['M'] == -math.inf and r['g'] == 1.0 and r['limited'] == 0
    # the limited branch: one large sample holds the gain down
    spike = x.copy()
    spike[777] = 0.9
    free, held = lr.level(spike, sr, -16.0, 1.0), lr.level(spike, sr, -16.0, 0.5)
    assert held['limited'] == 1 and held['g'] == 0.5 / 0.9 and abs(held['peak_out'] - 0.5) < 1e-15
    assert held['I'] + 20 * math.log10(held['g']) < -16.0
    assert free['limited'] in (0, 1) and free['peak_out'] <= 1.0 + 1e-12
    # a block below the relative gate does not count: quiet tail
    assert lr.measure(lr.gating_case(), sr)['blocks'][2] < lr.measure(lr.gating_case(), sr)['blocks'][1]


def test_pcm_rule_of_the_restatement():
    out, pcm = lr.pcm_fp32(np.array([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -3.0, 1e-6], np.float32), 1.0)
    assert pcm.tolist() == [0, 16383, -16383, 32767, -32767, 32767, -32767, 0] and out.dtype == np.float32


def test_wrapper_checks_run_before_the_device(built_lib):
    """every refusal of lib.wave_loudness is a ValueError that names the wrapper, raised for CPU tensors as for any other"""
    lib = built_lib
    x = torch.zeros(2, 100)
    bad = [dict(wave=torch.zeros(100)), dict(wave=torch.zeros(2, 100, dtype=torch.float64)), dict(wave=torch.zeros(2, 0)),
           dict(samples=torch.zeros(2, dtype=torch.int64)), dict(samples=torch.zeros(3, dtype=torch.int32)),
           dict(sr=7999), dict(sr=16005), dict(sr=48010), dict(sr=16000.5),
           dict(target=-70.5), dict(target=0.1), dict(target=float('nan')),
           dict(target=-23.0, ceiling=0.0), dict(target=-23.0, ceiling=1.01), dict(target=-23.0, ceiling=float('nan')),
           dict(target=-23.0, want_out=False, want_pcm=False), dict(want_out=True), dict(pcm=torch.zeros(2, 100, dtype=torch.int16)),
           dict(target=-23.0, out=torch.zeros(2, 99)), dict(target=-23.0, pcm=torch.zeros(2, 100)),
           dict(loud=torch.zeros(2, 3)), dict(blocks=torch.zeros(2, 4)), dict(work=torch.zeros(4, 4))]
    for kw in bad:
        a = dict(wave=x)
        a.update(kw)
        with pytest.raises(ValueError, match='wave_loudness'):
            lib.wave_loudness(**a)
    with pytest.raises(ValueError, match='must be on the GPU'):
        lib.wave_loudness(x)
    with pytest.raises(ValueError, match='must be on the GPU'):
        lib.wave_loudness(x, target=-23.0, ceiling=0.5)
    assert list(inspect.signature(lib.wave_loudness).parameters) == ['wave', 'samples', 'sr', 'target', 'ceiling', 'want_out', 'want_pcm',
                                                                    'out', 'pcm', 'loud', 'blocks', 'work']


def test_level_waveform_checks(built_lib):
    from tacotron_amd.griffinlim import level_waveform
    x = torch.zeros(2, 100)
    b = torch.zeros(2, 2, dtype=torch.int32)
    t = torch.zeros(2, dtype=torch.int32)
    for kw in (dict(bounds=b, total=t), dict(bounds=t), dict(total=b), dict(bounds=b.long()), dict(ceiling_db=0.5),
               dict(ceiling_db=float('nan')), dict(ceiling_db=float('-inf')), dict(target=1.0)):
        with pytest.raises(ValueError, match='level_waveform|wave_loudness'):
            level_waveform(x, **kw)
    for kw in (dict(), dict(bounds=b), dict(total=t)):   # (good arguments reach the device check)
        with pytest.raises(ValueError, match='must be on the GPU'):
            level_waveform(x, **kw)
    p = inspect.signature(level_waveform).parameters
    assert p['target'].default == -23.0 and p['ceiling_db'].default == -1.0 and p['sr'].default == 16000


def test_driver_options(built_lib, capsys):
    from tacotron_amd import test as drv
    a = drv.parse_args([])
    assert a.loudness is None and a.peak_db is None
    a = drv.parse_args(['--loudness', '-23'])
    assert a.loudness == -23.0 and a.peak_db is None
    a = drv.parse_args(['--loudness', '-16', '--peak-db', '-2', '--stop', '--long', '--deemphasis', '--trim-db', '40', '--rate', '0.8'])
    assert a.loudness == -16.0 and a.peak_db == -2.0 and a.long is not None and a.deemphasis == 0.97
    assert drv.parse_args(['--loudness', '0', '--peak-db', '0']).peak_db == 0.0
    assert drv.parse_args(['--loudness', '-70']).loudness == -70.0
    for argv in (['--loudness', '0.5'], ['--loudness', '-70.5'], ['--loudness', 'nan'], ['--loudness'], ['--loudness', 'x'],
                 ['--loudness', '-23', '--peak-db', '0.1'], ['--loudness', '-23', '--peak-db', 'nan'],
                 ['--loudness', '-23', '--peak-db', '-inf'], ['--peak-db', '-1']):
        with pytest.raises(SystemExit) as e:
            drv.parse_args(argv)
        assert e.value.code == 2, argv
    capsys.readouterr()
    drv.check_options(loudness=-23.0)
    drv.check_options(loudness=-23.0, peak_db=-3.0)
    for kw in (dict(loudness=1.0), dict(loudness=-71.0), dict(loudness=float('nan')), dict(peak_db=-1.0), dict(loudness=-23.0, peak_db=1.0),
               dict(loudness=-23.0, vocode=False)):
        with pytest.raises(ValueError, match='loudness|peak_db'):
            drv.check_options(**kw)
    d = inspect.signature(drv.test).parameters
    assert d['loudness'].default is None and d['peak_db'].default is None
    row = drv.loud_row([-31.2, -28.0, 10 ** (8.2 / 20), 0.4], [50, 48, 40, 0])
    assert row.dtype == np.float64 and row.shape == (8,)
    assert drv.loud_line('prompt 3', row) == 'prompt 3: -31.2 LUFS -> -23.0 (gain +8.2 dB)'
    row = drv.loud_row([-31.2, -28.0, 10 ** (6.6 / 20), 0.891], [50, 48, 40, 1])
    assert drv.loud_line('prompt 3', row, -1.0) == 'prompt 3: -31.2 LUFS -> -24.6, limited by the -1 dB ceiling'
    assert 'level unchanged' in drv.loud_line('prompt 0', drv.loud_row([-math.inf, -math.inf, 1.0, 0.0], [1, 0, 0, 0]))
