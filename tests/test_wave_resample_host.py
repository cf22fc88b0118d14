"""CPU checks of the device resampling path (taco_wave_resample): the C ABI declaration, the exports and their ctypes signature, the
polyphase table of audio.resample_filter against the literal fp64 loop (tests/resample_ref.py), the oracle against an ideal tone,
the length rule, read_wav_raw, the binding's argument checks and the CLI option."""
import ctypes as C
import inspect
import os
import re
import wave as wavefile

import numpy as np
import pytest
import torch

from tests import resample_ref as rr

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'taco_hip.h')

PAIRS = [(48000, 24000), (44100, 16000), (16000, 24000), (22050, 16000)]
# (Q, taps) per rate pair: the most taps one output sums, left + right, measured with an fp64 prototype of resampy's loop before the
# table existed.  (The table may be one column wider: at 44.1 -> 16 kHz the longest left wing, 177 taps, and the longest right wing,
# 177, belong to different phases; no phase has more than 353.)
TAPS = {(48000, 24000): (1, 255), (44100, 16000): (160, 353), (16000, 24000): (3, 127), (22050, 16000): (320, 175), (48000, 16000): (1, 383)}


def _args(decl):
    return [' '.join(a.split()) for a in decl.replace('\n', ' ').split(',')]


def apply_table(x, P, Q, n_left, n_right, table, n_calc):
    """the product form in fp64: y[t] = sum of table row (t P) % Q over x around nn = (t P) // Q, x = 0 outside the signal"""
    x = np.asarray(x, dtype=np.float64)
    pad = np.concatenate([np.zeros(n_left), x, np.zeros(n_right + 1)])
    y = np.zeros(n_calc)
    for t in range(n_calc):
        nn, p = divmod(t * P, Q)
        left = pad[n_left + nn - np.arange(n_left)]
        right = pad[n_left + nn + 1 + np.arange(n_right)]
        y[t] = table[p, :n_left] @ left + table[p, n_left:] @ right
    return y


def test_header_declares_the_entry_point():
    hdr = open(HDR).read()
    fn = re.search(r'\bint taco_wave_resample\(([^)]*)\);', hdr)
    assert fn
    assert _args(fn.group(1)) == ['const uint8_t* pcm', 'int64_t row_bytes', 'int width', 'int channels', 'const int32_t* rows',
                                  'const float* taps', 'int P', 'int Q', 'int n_left', 'int n_right', 'float* wave', 'int B', 'int L',
                                  'void* stream']
    assert int(re.search(r'#define\s+TACO_VERSION\s+(\d+)', hdr).group(1)) == 120
    assert 'detect it by the symbol' in hdr and 'kaiser_best' in hdr
    assert 'taco_wave_resample_workspace_bytes' not in hdr   # no workspace


def test_library_exports_it_at_version_120(built_lib):
    assert built_lib.version() == 120
    assert 'taco_wave_resample' in built_lib.EXPORTS
    assert hasattr(C.CDLL(built_lib.LIB_PATH), 'taco_wave_resample')
    res, args = built_lib.EXPORTS['taco_wave_resample']
    P, I, L = C.c_void_p, C.c_int, C.c_int64
    assert res is C.c_int and args == [P, L, I, I, P, P, I, I, I, I, P, I, I, P]
    tile = int(re.search(r'#define\s+TACO_WAVE_RESAMPLE_TILE\s+(\d+)', open(HDR).read()).group(1))
    assert built_lib.WAVE_RESAMPLE_TILE == tile == 1024


@pytest.mark.parametrize('sr_orig,sr_new', PAIRS, ids=['%d_%d' % p for p in PAIRS])
def test_polyphase_table_equals_the_literal_loop(sr_orig, sr_new):
    """random 1500-sample signal: the table applied at integer phases equals resampy's floating time register within
    1e-12 max|y| -- the polyphase derivation, the phases at exact-integer times and the clipping at both ends included"""
    from tacotron_amd import audio
    x = np.random.default_rng(sr_orig + sr_new).standard_normal(1500)
    y, S, K = rr.resample(x, sr_orig, sr_new)
    n_calc, n_len = audio.resample_lengths(len(x), sr_orig, sr_new)
    assert (n_calc, n_len) == rr.lengths(len(x), sr_orig, sr_new) and len(y) == n_len
    P, Q, n_left, n_right, table = audio.resample_filter(sr_orig, sr_new)
    assert table.dtype == np.float64 and table.shape == (Q, n_left + n_right)
    g = np.gcd(sr_orig, sr_new)
    assert (P, Q) == (sr_orig // g, sr_new // g)
    got = apply_table(x, P, Q, n_left, n_right, table, n_calc)
    err = np.abs(got - y[:n_calc]).max()
    print('  %d -> %d: max |table - loop| = %.3e, max |y| = %.3f, taps %d..%d' % (sr_orig, sr_new, err, np.abs(y).max(), K.min(), K.max()))
    assert err <= 1e-12 * np.abs(y).max()
    assert K.max() == TAPS[(sr_orig, sr_new)][1] <= n_left + n_right and (y[n_calc:] == 0).all()
    # the zero padding of shorter phases carries no weight, and every row has weight somewhere
    assert (np.abs(table).sum(axis=1) > 0.5 * min(1.0, sr_new / sr_orig)).all()


def test_tap_counts():
    from tacotron_amd import audio
    for (sr_orig, sr_new), (Q, taps) in TAPS.items():
        _, q, n_left, n_right, table = audio.resample_filter(sr_orig, sr_new)
        per_phase = np.count_nonzero(table, axis=1)
        assert q == Q and per_phase.max() == taps, (sr_orig, sr_new, q, n_left, n_right, per_phase.max())
        assert taps <= n_left + n_right <= taps + 1 and n_left >= 1 and n_right >= 1
        if Q == 1:
            assert n_left + n_right == taps
    assert audio.resample_filter(48000, 24000)[:4] == (2, 1, 128, 127)
    with pytest.raises(ValueError):
        audio.resample_filter(0, 16000)


def test_oracle_resamples_a_tone():
    """1 kHz from 48 to 24 kHz: the fp64 loop gives the ideal tone within 1e-7 over the middle half (7.1e-9 measured in fp64)"""
    n = 4000
    x = np.sin(2 * np.pi * 1000.0 * np.arange(n) / 48000.0)
    y, _, _ = rr.resample(x, 48000, 24000)
    ideal = np.sin(2 * np.pi * 1000.0 * np.arange(len(y)) / 24000.0)
    mid = slice(len(y) // 4, 3 * len(y) // 4)
    err = np.abs(y[mid] - ideal[mid]).max()
    print('  tone 48 -> 24 kHz: max error over the middle half %.3e' % err)
    assert err <= 1e-7


def test_resample_lengths():
    from tacotron_amd import audio
    assert audio.resample_lengths(1, 48000, 24000) == (0, 1)
    assert audio.resample_lengths(2, 48000, 24000) == (1, 1)
    assert audio.resample_lengths(0, 48000, 24000) == (0, 0)
    for sr_orig, sr_new in PAIRS + [(48000, 16000), (16000, 16000)]:
        ratio = float(sr_new) / sr_orig
        for n in list(range(1, 70)) + [441, 1499, 1500, 2500, 107999, 192000, 480001]:
            n_calc, n_len = audio.resample_lengths(n, sr_orig, sr_new)
            assert n_calc == int(n * ratio) and n_len == int(np.ceil(n * ratio)), (sr_orig, sr_new, n)
            assert 0 <= n_len - n_calc <= 1 and n_len >= 1
            assert isinstance(n_calc, int) and isinstance(n_len, int)


def _write_wav(path, frames, channels, width, rate):
    with wavefile.open(str(path), 'wb') as f:
        f.setnchannels(channels)
        f.setsampwidth(width)
        f.setframerate(rate)
        f.writeframes(frames)


@pytest.mark.parametrize('channels', [1, 2])
@pytest.mark.parametrize('width', [1, 2, 3, 4])
def test_read_wav_raw_round_trips(tmp_path, width, channels):
    from tacotron_amd import audio
    n = 301
    data = np.random.default_rng(10 * width + channels).integers(0, 256, size=n * width * channels, dtype=np.uint8)
    path = tmp_path / 'x.wav'
    _write_wav(path, data.tobytes(), channels, width, 44100)
    raw, ch, w, rate, frames = audio.read_wav_raw(path)
    assert (ch, w, rate, frames) == (channels, width, 44100, n)
    assert raw.dtype == np.uint8 and np.array_equal(raw, data)
    _write_wav(path, b'', channels, width, 8000)
    raw, ch, w, rate, frames = audio.read_wav_raw(str(path))
    assert len(raw) == 0 and frames == 0 and rate == 8000


def test_wrapper_refuses_bad_arguments_before_any_device_call(built_lib):
    """every refusal is raised on the host before the entry point is called (CPU tensors never reach it)"""
    B, L = 2, 50
    pcm = torch.zeros(B, 240, dtype=torch.uint8)          # 60 stereo PCM16 frames per row
    rows = torch.tensor([[60, 30], [10, 5]], dtype=torch.int32)
    taps = torch.zeros(1, 255)
    good = dict(pcm=pcm, rows=rows, taps=taps, width=2, channels=2, P=2, Q=1, n_left=128, n_right=127, L=L)
    called = []
    real = built_lib._lib.taco_wave_resample
    bad = [
        dict(pcm=torch.zeros(240, dtype=torch.uint8)),                   # no batch dimension
        dict(pcm=torch.zeros(B, 240, 1, dtype=torch.uint8)),
        dict(pcm=torch.zeros(B, 0, dtype=torch.uint8)),                  # no bytes
        dict(pcm=torch.zeros(B, 240, dtype=torch.int16)),                # not bytes
        dict(pcm=torch.zeros(240, B, dtype=torch.uint8).t()),            # not contiguous
        dict(pcm=torch.zeros(B, 242, dtype=torch.uint8)),                # half a frame
        dict(width=0), dict(width=5), dict(width=2.5), dict(channels=0), dict(channels=9),
        dict(width=3, channels=3),                                       # 240 bytes are no multiple of 9
        dict(P=0), dict(Q=0), dict(P=-2), dict(n_left=0), dict(n_right=0), dict(n_right=-1),
        dict(rows=rows.long()), dict(rows=rows[:1]), dict(rows=rows.view(4)), dict(rows=torch.zeros(B, 3, dtype=torch.int32)),
        dict(taps=None),                                                 # P != Q needs the table
        dict(taps=torch.zeros(1, 254)), dict(taps=torch.zeros(2, 255)), dict(taps=torch.zeros(255)),
        dict(taps=torch.zeros(1, 255, dtype=torch.float64)),
        dict(Q=3, taps=torch.zeros(1, 255)),                             # Q rows
        dict(P=64, taps=torch.zeros(1, 255)),                            # a tile's span does not fit the LDS
        dict(L=None), dict(L=0), dict(L=-3), dict(L=2.5),
        dict(L=None, out=torch.zeros(B + 1, L)), dict(L=None, out=torch.zeros(B, L, dtype=torch.float64)),
        dict(L=None, out=torch.zeros(B * L)), dict(L=None, out=torch.zeros(L, B).t()),
        dict(out=torch.zeros(B, L)),                                     # both L and out
        {},                                                              # good arguments, but on the CPU: no fallback
    ]
    try:
        built_lib._lib.taco_wave_resample = lambda *a: called.append(a) or 0
        for kw in bad:
            with pytest.raises(ValueError):
                built_lib.wave_resample(**dict(good, **kw))
    finally:
        built_lib._lib.taco_wave_resample = real
    assert not called
    sig = inspect.signature(built_lib.wave_resample).parameters
    assert list(sig) == ['pcm', 'rows', 'taps', 'width', 'channels', 'P', 'Q', 'n_left', 'n_right', 'L', 'out']
    assert sig['L'].default is None and sig['out'].default is None


def test_resample_option_parses_and_defaults_to_host(capsys):
    from tacotron_amd import preprocess
    assert preprocess.parse_args(['vctk']).resample == 'host'
    assert preprocess.parse_args(['vctk', '--resample', 'device']).resample == 'device'
    assert preprocess.parse_args(['nancy', '--resample', 'host', '--r', '3']).resample == 'host'
    with pytest.raises(SystemExit) as e:
        preprocess.parse_args(['vctk', '--resample', 'scipy'])
    assert e.value.code == 2
    capsys.readouterr()
    p = inspect.signature(preprocess.preprocess).parameters
    assert p['resample'].default == 'host'
    with pytest.raises(ValueError):   # refused before anything is read or written
        preprocess.preprocess({'prompts': [], 'audio_files': []}, os.devnull, resample='scipy')
