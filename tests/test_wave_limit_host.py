"""CPU: the host side of taco_wave_limit -- the tables of lib.true_peak_taps / lib.limit_window against the restatement's own
(tests/limiter_ref.py), what the interpolator reads on tones (EBU Tech 3341: +0.2 / -0.4 dB), the properties of the float32
restatement that the GPU test holds the kernel to bit for bit, and every refusal of the wrapper, level_waveform(limit=...) and the
driver's --limit options, none of which needs a GPU."""
import inspect
import math

import numpy as np
import pytest
import torch

from tests import limiter_ref as mr

TWO_22 = 2.0 ** -22


def test_tables_are_the_restatements(built_lib):
    lib = built_lib
    for P, T, beta in ((4, 12, 6.0), (2, 12, 6.0), (8, 32, 6.0), (4, 2, 0.0), (3, 16, 8.5), (1, 12, 6.0)):
        a, b = lib.true_peak_taps(P, T, beta), mr.taps(P, T, beta)
        assert a.dtype == np.float32 and a.shape == (P - 1, T) and np.array_equal(a.view(np.uint32), b.view(np.uint32)), (P, T, beta)
        s = a.astype(np.float64).sum(axis=1)
        assert (np.abs(s - 1.0) <= 2.0 ** -23).all(), (P, T, s)   # every phase sums to 1 within 1 ulp
    assert np.array_equal(lib.true_peak_taps(), mr.taps(4, 12, 6.0))
    for W in (0, 1, 8, 24, 72, 512):
        a, b = lib.limit_window(W), mr.window(W)
        assert a.dtype == np.float32 and a.shape == (2 * W + 1,) and np.array_equal(a.view(np.uint32), b.view(np.uint32)), W
        assert np.array_equal(a, a[::-1]) and (a > 0).all(), W
        assert abs(a.astype(np.float64).sum() - 1.0) < 1e-6
    for bad in (dict(P=0), dict(P=9), dict(T=1), dict(T=13), dict(T=34), dict(beta=float('nan')), dict(beta=-1.0)):
        with pytest.raises(ValueError, match='true_peak_taps'):
            lib.true_peak_taps(**bad)
    for W in (-1, 513, 1.5):
        with pytest.raises(ValueError, match='limit_window'):
            lib.limit_window(W)
    assert (lib.LIMIT_P, lib.LIMIT_T, lib.LIMIT_BETA, lib.LIMIT_CHUNK, lib.LIMIT_MAX_W) == (4, 12, 6.0, 2048, 512)


@pytest.mark.parametrize('sr', [16000, 24000, 48000])
def test_meter_reads_tones_within_tech_3341(built_lib, sr):
    """0.5-amplitude tones at fs/8, fs/4 (0 and 45 degrees), fs/3 and 5 fs/12, and 7 kHz: the fp64 meter with the default taps reads
    each within +0.2 / -0.4 dB of -6.02 dBTP (EBU Tech 3341's tolerance of a true-peak meter)"""
    tp = built_lib.true_peak_taps()
    want = 20 * math.log10(0.5)
    tones = list(mr.TONES) + [('7 kHz', 7000.0 / sr, 0.0)]
    for name, f, ph in tones:
        x = mr.tone(4000, f, ph)
        got = 20 * math.log10(mr.true_peak64(x, tp, 100))   # (100 samples away from the row's ends)
        print('  sr %d %-14s %.3f dBTP' % (sr, name, got))
        assert want - 0.4 <= got <= want + 0.2, (sr, name, got)
        f32 = 20 * math.log10(float(mr.limit(x, tp=tp)['e'][100:-100].max()))
        assert abs(f32 - got) < 1e-4
    # the reason the meter exists: the samples of the fs/4 row at 45 degrees all sit 3 dB under its crests
    x = mr.tone(4000, 0.25, np.pi / 4)
    assert abs(20 * math.log10(float(np.abs(x).max())) - (-9.03)) < 0.005


def _cases():
    x, ns, gain, ceiling = mr.edge_rows()
    for b, n in enumerate(ns):
        yield 'edge n_b = %d' % n, x[b, :n], gain[b], ceiling, mr.CASE_W, mr.taps()
    x, gain = mr.shape_rows()
    for b, name in enumerate(mr.SHAPE_NAMES):
        yield name, x[b], gain[b], mr.SHAPE_CEILING, mr.CASE_W, mr.taps()
    yield 'fs/4 at 45 deg, P = 1', x[2], 1.0, mr.SHAPE_CEILING, mr.CASE_W, None
    for W in (0, 1, 512):
        yield 'W = %d' % W, x[4, :4100], 4.0, mr.SHAPE_CEILING, W, mr.taps()
    for P, T in ((1, 12), (2, 12), (8, 12), (4, 2), (4, 32)):
        yield 'P = %d, T = %d' % (P, T), x[4, :4100], 4.0, mr.SHAPE_CEILING, mr.CASE_W, mr.taps(P, T)


def test_properties_of_the_restatement():
    """on every case of the GPU comparison: s <= r; |out| <= ceiling (1 + 2^-22) -- |fl(G x)| <= ge, and fl(ge fl(ceiling / ge)) carries
    two roundings --; s == 1 exactly wherever no r < 1 lies within 2 W; s < 1 only within 2 W of such a sample"""
    seen_limited = seen_clean = 0
    for name, x, G, ceiling, W, tp in _cases():
        ref = mr.limit(x, G, ceiling, tp, mr.window(W))
        n = len(x)
        if n == 0:
            assert ref['peaks'].tolist() == [0.0, float(np.float32(G)), 1.0, 0.0] and ref['counts'].tolist() == [0, 0]
            continue
        r, s, out = ref['r'], ref['s'], ref['out'][:n]
        assert (s <= r).all(), name
        assert (np.abs(out.astype(np.float64)) <= float(np.float32(ceiling)) * (1 + TWO_22)).all(), (name, np.abs(out).max())
        need = np.flatnonzero(r < 1)
        near = np.zeros(n, bool)
        for i in need:
            near[max(0, i - 2 * W):i + 2 * W + 1] = True
        assert (s[~near] == 1.0).all(), name
        assert near[s < 1].all(), name
        assert ref['counts'][1] == (s < 1).sum() and ref['peaks'][2] == s.min() and ref['peaks'][3] == np.abs(out).max()
        seen_limited += len(need) > 0
        seen_clean += len(need) == 0
    assert seen_limited >= 20 and seen_clean >= 2
    # the named shapes do what they are there for
    x, gain = mr.shape_rows()
    W, win, tp = mr.CASE_W, mr.window(mr.CASE_W), mr.taps()
    s = mr.limit(x[0], 1.0, mr.SHAPE_CEILING, tp, win)['s']
    assert (s[1000:1000 + 2 * W] < 1).all() and (s[3000 + W + 1:3000 + 3 * W + 1] < 1).any() and s[3000 + 2 * W + 1] == s[3000 + 2 * W + 1]
    merged, apart = s[1000:1000 + 2 * W].max(), s[3000:3000 + 4 * W + 3].max()
    assert merged < apart   # between the near pair the gain does not recover as far as between the far pair
    plateau = mr.limit(x[1], 1.0, mr.SHAPE_CEILING, tp, win)
    assert (plateau['s'][2030:2030 + 4 * W + 9] <= plateau['r'][2030:2030 + 4 * W + 9]).all() and plateau['counts'][1] > 4 * W
    sine4, sine1 = mr.limit(x[2], 1.0, mr.SHAPE_CEILING, tp, win), mr.limit(x[2], 1.0, mr.SHAPE_CEILING, None, win)
    assert sine4['counts'][1] > 0 and sine1['counts'][1] == 0 and np.array_equal(sine1['out'], x[2])
    quiet = mr.limit(x[3], 2.0, mr.SHAPE_CEILING, tp, win)
    assert quiet['counts'][1] == 0 and np.array_equal(quiet['out'], np.float32(2.0) * x[3])


def test_pcm_rule_of_the_restatement():
    assert mr.pcm16(np.array([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -3.0, 1e-6], np.float32)).tolist() == [0, 16383, -16383, 32767, -32767, 32767, -32767, 0]


def test_wrapper_checks_run_before_the_device(built_lib):
    """every refusal of lib.wave_limit is a ValueError that names the wrapper, raised for CPU tensors as for any other"""
    lib = built_lib
    x = torch.zeros(2, 100)
    win = lib.limit_window(4)
    bad = [dict(wave=torch.zeros(100)), dict(wave=torch.zeros(2, 100, dtype=torch.float64)), dict(wave=torch.zeros(2, 0)),
           dict(samples=torch.zeros(2, dtype=torch.int64)), dict(samples=torch.zeros(3, dtype=torch.int32)),
           dict(gain=torch.zeros(2, dtype=torch.float64)), dict(gain=torch.zeros(3)), dict(gain=1.0),
           dict(taps=np.zeros((3, 11), np.float32)), dict(taps=np.zeros((8, 12), np.float32)), dict(taps=np.zeros((3, 34), np.float32)),
           dict(taps=np.zeros((3, 12))), dict(taps=np.zeros(12, np.float32)), dict(taps='x'),
           dict(window=np.zeros(4, np.float32)), dict(window=np.zeros(1027, np.float32)), dict(window=np.zeros((3, 3), np.float32)),
           dict(window=np.zeros(5)),
           dict(window=win, ceiling=0.0), dict(window=win, ceiling=1.01), dict(window=win, ceiling=float('nan')),
           dict(window=win, want_out=False, want_pcm=False), dict(want_out=True), dict(pcm=torch.zeros(2, 100, dtype=torch.int16)),
           dict(window=win, out=torch.zeros(2, 99)), dict(window=win, pcm=torch.zeros(2, 100)),
           dict(peaks=torch.zeros(2, 3)), dict(counts=torch.zeros(2, 2)), dict(work=torch.zeros(4, 4))]
    for kw in bad:
        a = dict(wave=x)
        a.update(kw)
        with pytest.raises(ValueError, match='wave_limit') as e:
            lib.wave_limit(**a)
        assert 'must be on the GPU' not in str(e.value), kw
    big = torch.zeros(2, 200)
    with pytest.raises(ValueError, match='may not overlap'):
        lib.wave_limit(big.view(-1)[:200].view(2, 100), window=win, out=big.view(-1)[50:250].view(2, 100))
    for kw in (dict(), dict(window=win, ceiling=0.5), dict(window=win, out=x), dict(taps=np.zeros((0, 12), np.float32)),
               dict(taps=lib.true_peak_taps(8, 32), window=lib.limit_window(512), gain=torch.ones(2))):
        with pytest.raises(ValueError, match='must be on the GPU'):
            lib.wave_limit(x, **kw)
    assert list(inspect.signature(lib.wave_limit).parameters) == ['wave', 'samples', 'gain', 'ceiling', 'taps', 'window', 'want_out',
                                                                 'want_pcm', 'out', 'pcm', 'peaks', 'counts', 'work']
    for B, L, W in ((0, 10, 0), (1, 0, 0), (1, 10, -1), (1, 10, 513)):
        with pytest.raises(lib.TacoError):
            lib.wave_limit_workspace_floats(B, L, W)
    assert lib.wave_limit_workspace_floats(1, 1, 0) > 0 and 'taco_wave_limit' in lib.EXPORTS


def test_level_waveform_limit_checks(built_lib):
    from tacotron_amd.griffinlim import level_waveform, limit_settings
    x = torch.zeros(2, 100)
    for kw in (dict(limit=1), dict(limit='yes'), dict(limit=True, lookahead_ms=-1.0), dict(limit=True, lookahead_ms=float('nan')),
               dict(limit=True, lookahead_ms=float('inf')), dict(limit=True, lookahead_ms='x'), dict(limit=True, oversample=0),
               dict(limit=True, oversample=9), dict(limit=True, oversample=2.5), dict(limit=True, passes=0), dict(limit=True, passes=9),
               dict(limit=True, target=None), dict(limit=True, target=1.0), dict(limit=True, ceiling_db=0.5),
               dict(limit=True, want_out=False)):
        with pytest.raises(ValueError, match='level_waveform'):
            level_waveform(x, **kw)
    for kw in (dict(limit=True), dict(limit=True, lookahead_ms=0.0, oversample=1, passes=1), dict(limit=False)):
        with pytest.raises(ValueError, match='must be on the GPU'):
            level_waveform(x, **kw)
    p = inspect.signature(level_waveform).parameters
    assert (p['limit'].default, p['lookahead_ms'].default, p['oversample'].default, p['passes'].default) == (False, 1.5, 4, 2)
    assert limit_settings('t') == (24, 4, 2) and limit_settings('t', 1.5, 4, 2, sr=48000) == (72, 4, 2)
    assert limit_settings('t', 1000.0)[0] == 512 and limit_settings('t', 0.0)[0] == 0   # clamped into 0 .. 512


def test_driver_options(built_lib, capsys):
    from tacotron_amd import test as drv
    a = drv.parse_args(['--loudness', '-16'])
    assert a.limit is False and a.limit_ms is None and a.true_peak is None and a.limit_passes is None
    a = drv.parse_args(['--loudness', '-16', '--limit'])
    assert a.limit is True and a.limit_ms is None
    a = drv.parse_args(['--loudness', '-16', '--limit', '--limit-ms', '3', '--true-peak', '2', '--limit-passes', '1', '--peak-db', '-2', '--stop', '--long'])
    assert (a.limit_ms, a.true_peak, a.limit_passes, a.peak_db) == (3.0, 2, 1, -2.0)
    for argv in (['--limit'], ['--limit', '--peak-db', '-1'], ['--loudness', '-16', '--limit-ms', '2'], ['--loudness', '-16', '--true-peak', '4'],
                 ['--loudness', '-16', '--limit-passes', '2'], ['--loudness', '-16', '--limit', '--limit-ms', '-1'],
                 ['--loudness', '-16', '--limit', '--limit-ms', 'nan'], ['--loudness', '-16', '--limit', '--true-peak', '0'],
                 ['--loudness', '-16', '--limit', '--true-peak', '9'], ['--loudness', '-16', '--limit', '--limit-passes', '0'],
                 ['--loudness', '-16', '--limit', '--true-peak', '2.5']):
        with pytest.raises(SystemExit) as e:
            drv.parse_args(argv)
        assert e.value.code == 2, argv
    capsys.readouterr()
    drv.check_options(loudness=-16.0, limit=True)
    drv.check_options(loudness=-16.0, limit=True, limit_ms=0.0, true_peak=1, limit_passes=8)
    for kw in (dict(limit=True), dict(limit=1, loudness=-16.0), dict(loudness=-16.0, limit_ms=1.5), dict(loudness=-16.0, true_peak=4),
               dict(loudness=-16.0, limit_passes=2), dict(loudness=-16.0, limit=True, limit_ms=-1.0),
               dict(loudness=-16.0, limit=True, true_peak=9), dict(loudness=-16.0, limit=True, limit_passes=0),
               dict(loudness=-16.0, limit=True, vocode=False)):
        with pytest.raises(ValueError, match='limit|loudness|true_peak'):
            drv.check_options(**kw)
    with pytest.raises(ValueError, match='limit'):   # test() validates in the same place, before anything is loaded
        drv.test(None, [], limit=True)
    with pytest.raises(ValueError, match='limit'):
        drv.test(None, [], loudness=-16.0, limit_ms=2.0)
    d = inspect.signature(drv.test).parameters
    assert d['limit'].default is False and all(d[k].default is None for k in ('limit_ms', 'true_peak', 'limit_passes'))
    assert drv.limit_options() == dict(limit=True, lookahead_ms=1.5, oversample=4, passes=2)
    row = drv.limit_row([0.31, 3.6, 10 ** (-4.2 / 20), 0.89], [32000, 992], -16.2, 10 ** (-1.0 / 20), -27.3)
    assert row.dtype == np.float64 and row.shape == (9,)
    assert drv.limit_line('prompt 3', row, -16.0) == ('prompt 3: -27.3 LUFS -> -16.2 (asked -16.0), true peak -1.0 dBTP, '
                                                       '3.1 % of samples limited, deepest -4.2 dB')
    assert 'level unchanged' in drv.limit_line('prompt 0', drv.limit_row([0, 1, 1, 0], [5, 0], -math.inf, 0.0, -math.inf), -16.0)


def test_the_option_names_exist_once(tmp_path):
    """The record of the options, check_options and test() name the same options with the same defaults (check_options: path_jump
    None), and a command line that sets every flag reaches test() whole: what option_keywords makes of the namespace are names
    test() accepts -- every option but `vocode`, which has no flag -- and the record's check passes on them."""
    import dataclasses
    from tacotron_amd import lib
    from tacotron_amd import test as drv
    fields = {f.name: f.default for f in dataclasses.fields(drv.Options)}
    checked = {k: p.default for k, p in inspect.signature(drv.check_options).parameters.items()}
    driven = {k: p.default for k, p in inspect.signature(drv.test).parameters.items()
              if k not in ('config', 'prompts', 'out_dir', 'checkpoint', 'speaker')}
    assert set(fields) == set(checked) == set(driven)
    assert fields == driven and dict(fields, path_jump=None) == checked
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in inspect.signature(drv.check_options).parameters.values())
    prosody = tmp_path / 'prosody.tsv'
    prosody.write_text('0\t0\t0.8\t-\n')
    common = ['--stop', '--end-offset', '2', '--hold', '3', '--min-steps', '5', '--vocode-lengths', '--gl-momentum', '0.99', '--gl-iters', '7',
              '--gl-init', 'estimate', '--deemphasis', '0.9', '--trim-db', '40', '--rate', '0.8', '--pitch', '2', '--lifter', '24',
              '--f0-range', '70,350', '--f0-smooth', '--f0-candidates', '3', '--align-scores', '--timings', '--path-jump', '2',
              '--loudness', '-16', '--peak-db', '-2', '--limit', '--limit-ms', '3', '--true-peak', '2', '--limit-passes', '1']
    seen = {}
    for argv in (common + ['--long', '--pause-ms', '200,100,10', '--fade-ms', '2'], common + ['--prosody', str(prosody)]):
        kw = drv.option_keywords(drv.parse_args(argv))
        assert set(kw) == set(driven) - {'vocode'}
        drv.Options(**kw).check()
        for k, v in kw.items():
            if v != fields[k]:
                seen[k] = v
        rule = kw['stop']
        assert isinstance(rule, lib.TacoStopRule) and (rule.end_offset, rule.hold, rule.min_steps) == (2, 3, 5)
        assert (kw['n_iter'], kw['gl_momentum'], kw['gl_init'], kw['deemphasis'], kw['trim_db']) == (7, 0.99, 'estimate', 0.9, 40.0)
        assert (kw['rate'], kw['pitch'], kw['lifter'], kw['f0'], kw['f0_smooth'], kw['path_jump']) == (0.8, 2.0, 24, (70.0, 350.0), 3, 2)
        assert (kw['loudness'], kw['peak_db'], kw['limit'], kw['limit_ms'], kw['true_peak'], kw['limit_passes']) == (-16.0, -2.0, True, 3.0, 2, 1)
        assert kw['vocode_lengths'] is True and kw['align_scores'] is True and kw['timings'] is True
    assert set(seen) == set(driven) - {'vocode'}            # between them the two command lines move every option off its default
    assert seen['long'] == dict(pause_ms=(200.0, 100.0, 10.0), fade_ms=2.0) and seen['prosody'] == [(0, 0, 0.8, None)]
    assert drv.option_keywords(drv.parse_args([]))['stop'] is None
