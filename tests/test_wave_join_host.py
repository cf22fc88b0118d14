"""CPU checks of joining long prompts (taco_wave_join): the C ABI declaration and its version, the exports and their ctypes signature,
the workspace query, the Python binding's argument checks, the host splitter (data.split_prompt), the driver's --long options, and the
NumPy restatement (tests/join_ref.py) the GPU tests compare against, on numbers worked by hand."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import join_ref as jr

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'taco_hip.h')


def _args(decl):
    return [' '.join(a.split()) for a in decl.replace('\n', ' ').split(',')]


def test_header_declares_both_entry_points():
    hdr = open(HDR).read()
    ws = re.search(r'int64_t taco_wave_join_workspace_bytes\(([^)]*)\);', hdr)
    assert ws and _args(ws.group(1)) == ['int N', 'int P', 'int Lj']
    fn = re.search(r'\bint taco_wave_join\(([^)]*)\);', hdr)
    assert fn
    assert _args(fn.group(1)) == ['const float* pieces', 'int64_t pitch', 'const int32_t* bounds', 'const int32_t* first',
                                  'const int32_t* gap', 'int fade', 'float* out', 'int16_t* pcm', 'int32_t* offsets', 'int32_t* total',
                                  'float* peak', 'void* workspace', 'int N', 'int P', 'int L', 'int Lj', 'void* stream']
    at = [hdr.index(d) for d in ('int taco_wave_finish(', 'int64_t taco_wave_join_workspace_bytes(', 'int64_t taco_audio_features_workspace_bytes(')]
    assert at == sorted(at)
    assert int(re.search(r'#define\s+TACO_VERSION\s+(\d+)', hdr).group(1)) == 120


def test_library_exports_them_at_version_120(built_lib):
    assert built_lib.version() == 120
    for name in ('taco_wave_join_workspace_bytes', 'taco_wave_join'):
        assert name in built_lib.EXPORTS
        assert hasattr(C.CDLL(built_lib.LIB_PATH), name)
    res, args = built_lib.EXPORTS['taco_wave_join']
    P, I, H = C.c_void_p, C.c_int, C.POINTER(C.c_int32)
    assert res is C.c_int and args == [P, C.c_int64, P, H, H, I, P, P, P, P, P, P, I, I, I, I, P]
    assert built_lib.EXPORTS['taco_wave_join_workspace_bytes'] == (C.c_int64, [I, I, I])


def test_workspace_query(built_lib):
    """room for the fp32 rows a pcm-only call needs and for the copies of first and gap; refusals for non-positive arguments"""
    for N, P, Lj in ((1, 1, 1), (5, 3, 4001), (32, 8, 4 * 107700 + 1000), (300, 2, 999)):
        n = built_lib.wave_join_workspace_bytes(N, P, Lj)
        assert 4 * (P * Lj + P + 1 + N) <= n <= 4 * (P * (Lj + 3 + Lj // 1024 + 2) + P + 1 + N) + 64
    raw = built_lib._lib.taco_wave_join_workspace_bytes
    for N, P, Lj in ((0, 1, 100), (-1, 1, 100), (2, 0, 100), (2, -1, 100), (2, 1, 0), (2, 1, -7)):
        assert raw(N, P, Lj) == -1
        with pytest.raises(built_lib.TacoError):
            built_lib.wave_join_workspace_bytes(N, P, Lj)


def test_wrapper_refuses_bad_arguments_before_any_device_call(built_lib):
    """every refusal is raised on the host before the entry point is called (CPU tensors never reach it)"""
    N, L = 4, 50
    x = torch.zeros(N, L)
    b = torch.zeros(N, 2, dtype=torch.int32)
    first, gap = [0, 3, 4], [1, 2, 3, 4]
    good = dict(pieces=x, bounds=b, first=first, gap=gap)
    called = []
    real = built_lib._lib.taco_wave_join
    bad = [
        dict(first=[0, 3, 2, 4]),                                           # not monotone
        dict(first=[1, 3, 4]),                                              # does not start at 0
        dict(first=[0, 3, 5]),                                              # first[P] != N
        dict(first=[0, 3, 3]),
        dict(first=[0]),                                                    # no prompt
        dict(first=[0.0, 3.5, 4.0]),                                        # not integers
        dict(first=torch.tensor([0.0, 3.0, 4.0])),                          # a float tensor
        dict(gap=[1, 2, -1, 4]),                                            # negative gap
        dict(gap=[1, 2, 3]),                                                # N - 1 gaps
        dict(gap=[1, 2, 3, 1 << 31]),                                       # does not fit int32
        dict(gap=[1, 2, 3, 0.5]),
        dict(fade=-1),
        dict(fade=2.5),
        dict(want_out=False, want_pcm=False),                               # nothing to emit
        dict(pieces=x.double()),                                            # wrong dtypes
        dict(pieces=x.half()),
        dict(bounds=b.long()),
        dict(bounds=torch.zeros(N, 2)),
        dict(pieces=torch.zeros(L)),                                        # wrong shapes
        dict(pieces=torch.zeros(N, 0)),
        dict(bounds=torch.zeros(N, dtype=torch.int32)),
        dict(bounds=torch.zeros(N + 1, 2, dtype=torch.int32)),
        dict(pieces=torch.zeros(1, L).expand(N, L)),                        # pitch 0 < L
        dict(pieces=torch.zeros(N * L).as_strided((N, L), (L - 1, 1))),     # pitch L - 1 < L
        dict(pieces=torch.zeros(L, N).t()),                                 # samples not contiguous
        dict(Lj=0),
        dict(Lj=-8),
        dict(Lj=10.5),
        dict(Lj=100, out=torch.zeros(2, 101)),
        dict(Lj=100, out=torch.zeros(2, 100, dtype=torch.float64)),
        dict(Lj=100, pcm=torch.zeros(2, 100, dtype=torch.int32)),
        dict(Lj=100, pcm=torch.zeros(3, 100, dtype=torch.int16)),
        dict(offsets=torch.zeros(N, dtype=torch.int64)),
        dict(offsets=torch.zeros(N + 1, dtype=torch.int32)),
        dict(total=torch.zeros(3, dtype=torch.int32)),
        dict(total=torch.zeros(2)),
        dict(peak=torch.zeros(2, 1)),
        dict(peak=torch.zeros(2, dtype=torch.float64)),
        dict(Lj=100, work=torch.zeros(built_lib.wave_join_workspace_bytes(N, 2, 100) - 1, dtype=torch.uint8)),
        dict(Lj=100, work=torch.zeros(built_lib.wave_join_workspace_bytes(N, 2, 100))),
        dict(),                                                             # everything right, but on the CPU
    ]
    big = torch.zeros(N * L + 2 * 60)
    bad.append(dict(pieces=big[:N * L].view(N, L), Lj=60, out=big[N * L - 60:N * L + 60].view(2, 60)))   # out overlaps pieces
    try:
        built_lib._lib.taco_wave_join = lambda *a: called.append(a) or 0
        for kw in bad:
            with pytest.raises(ValueError):
                built_lib.wave_join(**dict(good, **kw))
    finally:
        built_lib._lib.taco_wave_join = real
    assert not called
    sig = inspect.signature(built_lib.wave_join).parameters
    assert [(k, sig[k].default) for k in list(sig)[4:]] == [
        ('fade', 0), ('Lj', None), ('want_out', True), ('want_pcm', True), ('out', None), ('pcm', None), ('offsets', None),
        ('total', None), ('peak', None), ('work', None)]


def test_join_waveform_turns_kinds_and_milliseconds_into_samples(built_lib):
    from tacotron_amd import data, griffinlim as gl
    kinds = [data.SENTENCE, data.CLAUSE, data.WORD, data.HARD, data.END]
    assert gl.join_gaps(kinds) == [4800, 2400, 0, 0, 0]
    assert gl.join_gaps(kinds, (100, 50.5, 1)) == [1600, 808, 16, 0, 0]
    assert gl.join_samples(5.0) == 80 and gl.join_samples(0) == 0
    for bad in (-1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            gl.join_samples(bad)
        with pytest.raises(ValueError):
            gl.join_gaps(kinds, (bad, 0, 0))
    with pytest.raises(ValueError):
        gl.join_gaps(kinds, (1, 2))
    seen = []
    real = built_lib.wave_join
    try:
        built_lib.wave_join = lambda *a, **k: seen.append((a, k)) or None
        gl.join_waveform('pieces', 'bounds', [0, 2, 5], kinds, want_out=False)
        gl.join_waveform('pieces', 'bounds', [0, 5], kinds, pause_ms=(10, 20, 30), fade_ms=1.0, Lj=64)
    finally:
        built_lib.wave_join = real
    assert seen[0] == (('pieces', 'bounds', [0, 2, 5], [4800, 2400, 0, 0, 0]), dict(fade=80, want_out=False))
    assert seen[1] == (('pieces', 'bounds', [0, 5], [160, 320, 480, 0, 0]), dict(fade=16, Lj=64))


# ---- the splitter ------------------------------------------------------------------------------------------------------------------
def _squash(s):
    return s.replace(' ', '').replace('\n', '')


def test_split_prompt_properties_over_random_lines():
    from tacotron_amd.data import END, HARD, split_prompt
    rng = np.random.default_rng(17)
    alphabet = np.array(list('abcdefghij' + ' ' * 3 + '.,;:?!'))
    longest = 0
    for trial in range(2000):
        n = int(rng.integers(0, 701))
        line = ''.join(rng.choice(alphabet, size=n))
        if trial % 3 == 0:
            line += '\n'
        if trial % 7 == 0:   # a run without spaces, longer than a piece
            line = line[:n // 2] + 'x' * int(rng.integers(100, 300)) + line[n // 2:]
        pieces = split_prompt(line)
        if len(line.strip()) <= 140:
            assert pieces == [(line, END)]
            continue
        longest = max(longest, len(pieces))
        assert len(pieces) >= 2 and pieces[-1][1] == END and all(k != END for _, k in pieces[:-1])
        for text, kind in pieces:
            assert 1 <= len(text) - 1 <= 140 and text.endswith('\n') and '\n' not in text[:-1]
            assert text[:-1] == text[:-1].strip(' ')
            assert kind != HARD or ' ' not in text
        assert _squash(''.join(t for t, _ in pieces)) == _squash(line)
    assert longest >= 5


def test_split_prompt_hand_cases():
    from tacotron_amd.data import CLAUSE, END, HARD, SENTENCE, WORD, split_prompt
    from tacotron_amd.config import MAX_TEXT_LEN
    assert (END, SENTENCE, CLAUSE, WORD, HARD) == (0, 1, 2, 3, 4) and MAX_TEXT_LEN == 140
    # short lines come back verbatim: the raw line, not its stripped text
    for line in ('', '\n', 'hello world.\n', '  padded  \n', 'a' * 140, 'a' * 140 + '\n', ' ' + 'a' * 140 + ' \n'):
        assert split_prompt(line) == [(line, END)]
    # a sentence end wins over a later comma, which wins over a later word boundary
    a, b, c = 'w' * 50 + '.', 'x' * 40 + ',', 'y' * 30
    line = ' '.join([a, b, c, 'z' * 60]) + '\n'
    assert len(line.strip()) > 140
    assert split_prompt(line) == [(a + '\n', SENTENCE), (' '.join([b, c, 'z' * 60]) + '\n', END)]
    # no sentence end inside the first 140: the last comma
    line = ' '.join(['w' * 50, b, c, 'z' * 60])
    assert split_prompt(line) == [('w' * 50 + ' ' + b + '\n', CLAUSE), (c + ' ' + 'z' * 60 + '\n', END)]
    # neither: the last word boundary at or below 140 characters
    line = ' '.join(['w' * 50, 'x' * 40, 'y' * 48, 'z' * 60])   # 50 + 1 + 40 + 1 + 48 = 140, then a space
    assert split_prompt(line) == [(' '.join(['w' * 50, 'x' * 40, 'y' * 48]) + '\n', WORD), ('z' * 60 + '\n', END)]
    line = ' '.join(['w' * 50, 'x' * 40, 'y' * 49, 'z' * 60])   # one more: that boundary is at 141
    assert split_prompt(line) == [(' '.join(['w' * 50, 'x' * 40]) + '\n', WORD), ('y' * 49 + ' ' + 'z' * 60 + '\n', END)]
    # a punctuation mark that is not followed by a space is no cut; several spaces are skipped
    line = 'w' * 60 + '.x' + 'w' * 60 + '   ' + 'v' * 100
    assert split_prompt(line) == [('w' * 60 + '.x' + 'w' * 60 + '\n', WORD), ('v' * 100 + '\n', END)]
    # a word of 141 characters is cut inside
    assert split_prompt('q' * 141) == [('q' * 140 + '\n', HARD), ('q\n', END)]
    assert split_prompt('q' * 141 + '\n') == [('q' * 140 + '\n', HARD), ('q\n', END)]
    assert [k for _, k in split_prompt('q' * 300 + ' end. ' + 'r' * 150)] == [HARD, HARD, SENTENCE, HARD, END]
    # three pieces, and another limit
    line = ('one. ' * 40).strip()
    got = split_prompt(line)
    assert [k for _, k in got] == [SENTENCE, END] and got[0][0] == ('one. ' * 28).strip() + '\n'
    assert split_prompt('ab cd, ef gh', max_chars=7) == [('ab cd,\n', CLAUSE), ('ef gh\n', END)]
    with pytest.raises(ValueError):
        split_prompt('abc', max_chars=0)


def test_load_prompts_still_refuses_a_long_line():
    from tacotron_amd.data import load_prompts
    ivocab = {i + 1: ch for i, ch in enumerate("abcdefghijklmnopqrstuvwxyz '.,?!-")}
    ivocab[0] = '<pad>'
    with pytest.raises(ValueError):
        list(load_prompts(['a' * 141 + '\n'], ivocab))
    got = list(load_prompts(['a' * 140 + '\n'], ivocab))
    assert got[0]['text'].shape == (1, 140) and got[0]['text_length'].tolist() == [140]


def test_driver_options(built_lib, capsys):
    from tacotron_amd import test as drv
    a = drv.parse_args([])
    assert a.long is None and a.pause_ms == (300.0, 150.0, 0.0) and a.fade_ms == 5.0
    a = drv.parse_args(['--stop', '--long'])
    assert a.long == dict(pause_ms=(300.0, 150.0, 0.0), fade_ms=5.0)
    a = drv.parse_args(['--stop', '--long', '--pause-ms', '200,100,20', '--fade-ms', '0', '--deemphasis', '--trim-db', '40'])
    assert a.long == dict(pause_ms=(200.0, 100.0, 20.0), fade_ms=0.0) and a.deemphasis == 0.97 and a.trim_db == 40.0
    on = ['--stop', '--long']
    for argv in (['--long'], ['--long', '--deemphasis'], on + ['--pause-ms', '1,2'], on + ['--pause-ms', 'x,1,2'],
                 on + ['--pause-ms', '-1,0,0'], on + ['--fade-ms', '-2'], on + ['--fade-ms', 'nan']):
        with pytest.raises(SystemExit) as e:
            drv.parse_args(argv)
        assert e.value.code == 2, argv
    capsys.readouterr()
    with pytest.raises(SystemExit):   # the help text says that the defaults are untuned
        drv.parse_args(['--help'])
    text = ' '.join(capsys.readouterr().out.split())
    assert '--long' in text and '--pause-ms' in text and '--fade-ms' in text and text.count('not tuned by ear') >= 2
    d = inspect.signature(drv.test).parameters
    assert d['long'].default is None
    assert inspect.signature(drv.check_options).parameters['long'].default is None
    with pytest.raises(ValueError):
        drv.check_options(long=True)
    with pytest.raises(ValueError):
        drv.check_options(stop=None, long=dict(fade_ms=1.0))
    drv.check_options(stop=True, long=True)
    drv.check_options(stop=True, long=dict(pause_ms=(1, 2, 3)))
    drv.check_options(long=None)
    drv.check_options(long=False)
    for kw in (dict(long=True), dict(long=True, deemphasis=0.5), dict(long=dict(fade_ms=-1.0), stop=True),
               dict(long=dict(pause_ms=(1, 2)), stop=True), dict(long=dict(pauses=(1, 2, 3)), stop=True)):
        with pytest.raises(ValueError):   # refused before anything is loaded or built
            drv.test(None, [], **kw)


# ---- the restatement on numbers worked by hand -------------------------------------------------------------------------------------
def test_restatement_on_the_small_case():
    c = jr.CORE
    x, bounds = jr.core_pieces()
    assert jr.piece_lengths(bounds, c['L']) == c['lens']
    out, pcm, offsets, total, peak = jr.join(x, bounds, c['first'], c['gap'], c['fade'], c['Lj'])
    assert offsets.tolist() == [0, 2600, 2600, 0, 34] and total.tolist() == [2607, 0, 1334]
    assert out.dtype == np.float32 and pcm.dtype == np.int16 and out.shape == pcm.shape == (3, 4001)
    assert np.isfinite(out).all()                                   # the NaN behind every len_i is never read
    # prompt 0: piece 0 whole apart from its last 16 samples, 100 zeros, nothing of piece 1, piece 2 with f = 3 at its front only
    assert np.array_equal(out[0, :2484], x[0, :2484])
    w16 = (np.arange(16, dtype=np.float32) + np.float32(0.5)) / np.float32(16)
    assert np.array_equal(out[0, 2484:2500], x[0, 2484:2500] * w16[::-1])
    assert not out[0, 2500:2600].any() and not out[0, 2607:].any()
    w3 = np.array([0.5 / 3, 1.5 / 3, 2.5 / 3])
    assert np.allclose(out[0, 2600:2603], x[2, :3] * w3, rtol=1e-6) and np.array_equal(out[0, 2603:2607], x[2, 3:7])
    # prompt 1 has no pieces; prompt 2: a one-sample piece untouched, 33 zeros, the last piece ramped at its front only
    assert not out[1].any() and peak[1] == 0 and not pcm[1].any()
    assert out[2, 0] == x[3, 0] and not out[2, 1:34].any()
    assert np.array_equal(out[2, 34:50], x[4, :16] * w16) and np.array_equal(out[2, 50:1334], x[4, 16:1300])
    assert not out[2, 1334:].any()
    for p in range(3):
        assert peak[p] == np.abs(out[p]).max()
    # a truncating Lj, a zero fade, and clamped bounds
    _, _, off2, tot2, _ = jr.join(x, bounds, c['first'], c['gap'], c['fade'], 2550)
    assert off2.tolist() == [0, 2550, 2550, 0, 34] and tot2.tolist() == [2550, 0, 1334]
    o0 = jr.join(x, bounds, c['first'], c['gap'], 0, c['Lj'])[0]
    assert np.array_equal(o0[0, :2500], x[0]) and np.array_equal(o0[2, 34:1334], x[4, :1300])
    assert jr.piece_lengths([[5, 3], [0, 9000], [7, 7]], 2500) == [0, 2500, 0]
    # the ramp weights: (k + 0.5) / f, symmetric, never 0 and never 1
    for f in (1, 3, 16, 80):
        w = jr.ramp(f)
        assert w.dtype == np.float32 and (w > 0).all() and (w < 1).all() and np.allclose(w + w[::-1], 1.0, atol=1e-7)
