"""GPU: taco_wave_resample (include/taco_hip.h) -- the resampled rows against the fp64 restatement of resampy's loop
(tests/resample_ref.py) within the derived bound (K + 4) 2^-24 S per output, decode-only bit for bit against audio.load_wav, the
tile edges, poisoned outputs between guard bands, unused input bytes, the per-row contract, determinism, graph replay, every
TACO_EINVAL case through the raw C ABI, and preprocess(..., resample='device').

Signals are a few thousand samples; the oracle of each (rate pair, channels) is computed once and shared."""
import ctypes as C
import functools
import pickle
import wave as wavefile

import numpy as np
import pytest
import torch

from tests import resample_ref as rr
from tests.poison import Guarded

pytestmark = pytest.mark.gpu

PAIRS = [(48000, 24000), (44100, 16000), (16000, 24000), (48000, 16000)]
FRAMES = [1, 40, 2500]     # one frame (n_calc = 0 at ratio 0.5); shorter than every n_left (both wings clipped by the row's ends); long


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[x.dtype.itemsize])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def decode16(q, channels):
    """int16 (frames * channels) interleaved -> the fp32 mono samples audio.load_wav gives"""
    x = q.astype(np.float32) * np.float32(2.0 ** -15)
    return x.reshape(-1, channels).mean(axis=1, dtype=np.float32) if channels > 1 else x


def pcm_rows(frames, channels, seed):
    """a list of int16 arrays, frames[b] * channels samples each: band-limited-ish noise plus a tone, different per channel"""
    rng = np.random.default_rng(seed)
    out = []
    for n in frames:
        t = np.arange(n)[:, None]
        x = 0.25 * rng.standard_normal((n, channels)) + 0.3 * np.sin(0.05 * t * (1 + np.arange(channels)) + rng.uniform(0, 6, channels))
        out.append(np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16).reshape(-1))
    return out


def pack(rows_bytes, pad_seed=0, pad=0):
    """(B, row_bytes) uint8: row b's bytes, then garbage (seeded noise, so that unused input is never zeros)"""
    width = max(len(r) for r in rows_bytes) + pad
    host = np.random.default_rng(1000 + pad_seed).integers(0, 256, size=(len(rows_bytes), max(width, 1)), dtype=np.uint8)
    for b, r in enumerate(rows_bytes):
        host[b, :len(r)] = r
    return host


def run(lib, host, width, channels, frames, sr_orig, sr_new, L=None, fill='qnan', n_calc=None, taps=True):
    """lib.wave_resample into a poisoned (B, L) buffer between guard bands; every element must have been written.
    -> (wave as a NumPy array, [(n_calc, n_len)])"""
    from tacotron_amd import audio
    P, Q, n_left, n_right, table = audio.resample_filter(sr_orig, sr_new)
    counts = [audio.resample_lengths(n, sr_orig, sr_new) for n in frames]
    calc = [c[0] for c in counts] if n_calc is None else list(n_calc)
    L = max(1, max(c[1] for c in counts)) if L is None else L
    B = len(frames)
    G = Guarded({'wave': ((B, L), torch.float32, fill)})
    pcm = torch.from_numpy(np.ascontiguousarray(host)).cuda()
    rows = torch.tensor([[n, c] for n, c in zip(frames, calc)], dtype=torch.int32, device='cuda')
    t = torch.from_numpy(table.astype(np.float32)).cuda() if taps else None
    r = lib.wave_resample(pcm, rows, t, width, channels, P, Q, n_left, n_right, out=G['wave'])
    torch.cuda.synchronize()
    assert r is G['wave']
    G.check(*(['wave'] if fill != 'zeros' else []))
    return r.cpu().numpy(), counts


@functools.lru_cache(maxsize=None)
def case(sr_orig, sr_new, channels):
    """the shared B = 3 ragged batch of a rate pair: PCM16 rows, their decoded samples and the oracle's (y, S, K) per row"""
    q = pcm_rows(FRAMES, channels, seed=sr_orig // 100 + sr_new // 1000 + channels)
    x = [decode16(r, channels) for r in q]
    ref = [rr.resample(v, sr_orig, sr_new) for v in x]
    for v in ref:
        for a in v:
            a.setflags(write=False)
    return q, x, ref


def check_rows(wave, counts, ref, what):
    worst = 0.0
    for b, ((n_calc, n_len), (y, S, K)) in enumerate(zip(counts, ref)):
        assert len(y) == n_len and len(S) == n_calc
        got = wave[b].astype(np.float64)
        err = np.abs(got[:n_calc] - y[:n_calc])
        E = rr.bound(S, K)
        ratio = float((err / np.maximum(E, 1e-300)).max()) if n_calc else 0.0
        worst = max(worst, ratio)
        print('  %s row %d: n_calc %d, taps %s, worst |gpu - oracle| / bound = %.4f, max |y| %.3f'
              % (what, b, n_calc, (int(K.min()), int(K.max())) if n_calc else '-', ratio, np.abs(y).max() if n_len else 0.0))
        assert (err <= E).all(), (what, b, ratio, int((err / np.maximum(E, 1e-300)).argmax()))
        assert not bits(wave[b, n_calc:]).any(), (what, b)          # exact (positive) zeros behind n_calc
    return worst


# ---- parity with the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('channels', [1, 2])
@pytest.mark.parametrize('sr_orig,sr_new', PAIRS, ids=['%d_%d' % p for p in PAIRS])
def test_resampled_rows_within_the_derived_bound(built_lib, sr_orig, sr_new, channels):
    q, x, ref = case(sr_orig, sr_new, channels)
    wave, counts = run(built_lib, pack([r.view(np.uint8) for r in q]), 2, channels, FRAMES, sr_orig, sr_new)
    if sr_new * 2 == sr_orig:
        assert counts[0] == (0, 1)
    assert wave.shape == (3, max(c[1] for c in counts))
    check_rows(wave, counts, ref, '%d -> %d, %d ch' % (sr_orig, sr_new, channels))


def test_tile_edges(built_lib):
    """48 -> 24 kHz, n_calc in {T - 1, T, T + 1, 2 T + 1} as the four rows of one call, L = 2 T + 6: the last tile is partial"""
    T = built_lib.WAVE_RESAMPLE_TILE
    want = [T - 1, T, T + 1, 2 * T + 1]
    frames = [2 * n for n in want]
    q = pcm_rows(frames, 1, seed=77)
    ref = [rr.resample(decode16(r, 1), 48000, 24000) for r in q]
    wave, counts = run(built_lib, pack([r.view(np.uint8) for r in q]), 2, 1, frames, 48000, 24000, L=2 * T + 6)
    assert [c[0] for c in counts] == want
    check_rows(wave, counts, ref, 'tile edges')


# ---- decode-only ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('channels', [1, 2, 3])
@pytest.mark.parametrize('width', [1, 2, 3, 4])
def test_decode_only_is_load_wav_bit_for_bit(built_lib, tmp_path, width, channels):
    """P == Q: random bytes (every bit pattern of every width, full-scale values included) -> the bits of audio.load_wav, through the
    binding (taps None) and through load_batch_device; exact zeros behind each row"""
    from tacotron_amd import audio
    T = built_lib.WAVE_RESAMPLE_TILE
    frames = [T + 3, 1, 517]
    rng = np.random.default_rng(100 * width + channels)
    raws, paths = [], []
    for i, n in enumerate(frames):
        data = rng.integers(0, 256, size=n * width * channels, dtype=np.uint8)
        if width > 1:   # the extreme values of the format (the one-sample row takes the most negative alone)
            ends = np.frombuffer(b'\x00' * (width - 1) + b'\x80' + b'\xff' * (width - 1) + b'\x7f', dtype=np.uint8)
            data[:2 * width] = ends[:len(data)]
        path = str(tmp_path / ('f%d.wav' % i))
        with wavefile.open(path, 'wb') as f:
            f.setnchannels(channels)
            f.setsampwidth(width)
            f.setframerate(16000)
            f.writeframes(data.tobytes())
        raws.append(data)
        paths.append(path)
    want = [audio.load_wav(p, 16000) for p in paths]
    wave, counts = run(built_lib, pack(raws), width, channels, frames, 16000, 16000, L=T + 9, taps=False)
    assert counts == [(n, n) for n in frames]
    for b, n in enumerate(frames):
        assert same_bits(wave[b, :n], want[b]), (width, channels, b)
        assert not bits(wave[b, n:]).any()
    waves, lengths = audio.load_batch_device(paths, 16000)
    assert lengths == frames and tuple(waves.shape) == (3, T + 3) and waves.dtype == torch.float32
    assert same_bits(waves.cpu().numpy(), wave[:, :T + 3])


def test_load_batch_device_groups_formats(built_lib, tmp_path):
    """files of two rates and two formats in one batch: each row equals its own single-file call, bit for bit, in the caller's order"""
    from tacotron_amd import audio
    specs = [(48000, 2, 1, 1500), (24000, 2, 2, 700), (48000, 2, 1, 333), (24000, 3, 1, 1), (48000, 2, 1, 0)]
    paths = []
    for i, (rate, width, channels, n) in enumerate(specs):
        path = str(tmp_path / ('g%d.wav' % i))
        with wavefile.open(path, 'wb') as f:
            f.setnchannels(channels)
            f.setsampwidth(width)
            f.setframerate(rate)
            f.writeframes(np.random.default_rng(i).integers(0, 256, size=n * width * channels, dtype=np.uint8).tobytes())
        paths.append(path)
    waves, lengths = audio.load_batch_device(paths, 24000)
    assert lengths == [750, 700, 167, 1, 0] and tuple(waves.shape) == (5, 750)
    waves = waves.cpu().numpy()
    for b, p in enumerate(paths[:4]):
        one, n1 = audio.load_batch_device([audio.read_wav_raw(p)], 24000)
        assert n1 == [lengths[b]]
        assert same_bits(waves[b, :lengths[b]], one.cpu().numpy()[0]), b
        assert not bits(waves[b, lengths[b]:]).any()
    assert not bits(waves[4]).any()
    for b in (1, 3):   # the files already at 24 kHz are load_wav's samples
        assert same_bits(waves[b, :lengths[b]], audio.load_wav(paths[b], 24000))


# ---- written range, unused input, rows, determinism -------------------------------------------------------------------------------
@pytest.mark.parametrize('sr_orig,sr_new', [(48000, 24000), (44100, 16000)], ids=['uniform', 'phases'])
def test_every_element_is_written_whatever_the_buffer_held(built_lib, sr_orig, sr_new):
    """L two tiles past the longest row: whole tiles of zeros.  NaN / all-ones / noise fills give the bits of the zero-filled call,
    nothing still holds its poison, exact zeros from n_calc to L, guard bands intact (run() checks them)"""
    q, x, ref = case(sr_orig, sr_new, 1)
    host = pack([r.view(np.uint8) for r in q])
    L = rr.lengths(FRAMES[-1], sr_orig, sr_new)[1] + 2 * built_lib.WAVE_RESAMPLE_TILE + 5
    base, counts = run(built_lib, host, 2, 1, FRAMES, sr_orig, sr_new, L=L, fill='zeros')
    check_rows(base, counts, ref, 'L = %d' % L)
    for fill in ('qnan', 'ones', 'noise'):
        got, _ = run(built_lib, host, 2, 1, FRAMES, sr_orig, sr_new, L=L, fill=fill)
        assert same_bits(got, base), fill


@pytest.mark.parametrize('sr_orig,sr_new,channels', [(48000, 24000, 2), (16000, 24000, 1)])
def test_bytes_behind_n_orig_have_no_influence(built_lib, sr_orig, sr_new, channels):
    q, _, _ = case(sr_orig, sr_new, channels)
    rows_bytes = [r.view(np.uint8) for r in q]
    a, _ = run(built_lib, pack(rows_bytes, pad_seed=1), 2, channels, FRAMES, sr_orig, sr_new)
    b, _ = run(built_lib, pack(rows_bytes, pad_seed=2, pad=4 * channels * 7), 2, channels, FRAMES, sr_orig, sr_new)
    ff = pack(rows_bytes)
    for i, r in enumerate(rows_bytes):
        ff[i, len(r):] = 0xff
    c, _ = run(built_lib, ff, 2, channels, FRAMES, sr_orig, sr_new)
    assert same_bits(a, b) and same_bits(a, c)


@pytest.mark.parametrize('sr_orig,sr_new', PAIRS[:3], ids=['%d_%d' % p for p in PAIRS[:3]])
def test_rows_are_the_call_on_each_row_alone_and_calls_repeat(built_lib, sr_orig, sr_new):
    q, _, _ = case(sr_orig, sr_new, 2)
    rows_bytes = [r.view(np.uint8) for r in q]
    host = pack(rows_bytes)
    wave, counts = run(built_lib, host, 2, 2, FRAMES, sr_orig, sr_new)
    again, _ = run(built_lib, host, 2, 2, FRAMES, sr_orig, sr_new, fill='ones')
    assert same_bits(wave, again)
    for b, n in enumerate(FRAMES):
        one, c1 = run(built_lib, rows_bytes[b][None], 2, 2, [n], sr_orig, sr_new)
        assert c1 == [counts[b]] and one.shape == (1, max(1, counts[b][1]))
        assert same_bits(wave[b, :one.shape[1]], one[0]), b


def test_graph_replay_follows_the_device_rows(built_lib):
    """one capture on a side stream; the replay reads `rows` at replay time"""
    from tacotron_amd import audio
    q, _, _ = case(48000, 24000, 1)
    host = pack([r.view(np.uint8) for r in q])
    P, Q, n_left, n_right, table = audio.resample_filter(48000, 24000)
    taps = torch.from_numpy(table.astype(np.float32)).cuda()
    pcm = torch.from_numpy(host).cuda()
    first = [[n, n // 2] for n in FRAMES]
    second = [[FRAMES[2], 1000], [0, 0], [300, 150]]
    rows = torch.tensor(first, dtype=torch.int32, device='cuda')
    L = 1300
    G = Guarded({'wave': ((3, L), torch.float32, 'qnan')})
    call = lambda: built_lib.wave_resample(pcm, rows, taps, 2, 1, P, Q, n_left, n_right, out=G['wave'])   # noqa: E731
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            call()
    torch.cuda.synchronize()
    for rw in (first, second, first):
        rows.copy_(torch.tensor(rw, dtype=torch.int32))
        G.refill('wave')
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        G.check('wave')
        want, _ = run(built_lib, host, 2, 1, [r[0] for r in rw], 48000, 24000, L=L, n_calc=[r[1] for r in rw])
        assert same_bits(G['wave'].cpu().numpy(), want), rw


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_enqueue_nothing(built_lib):
    """every TACO_EINVAL case returns before a launch: the output keeps its sentinel; the error string is set"""
    from tacotron_amd import audio
    lib = built_lib
    B, L = 2, 700
    P, Q, n_left, n_right, table = audio.resample_filter(48000, 24000)
    taps = torch.from_numpy(table.astype(np.float32)).cuda()
    pcm = torch.from_numpy(pack([r.view(np.uint8) for r in pcm_rows([600, 1400], 2, seed=5)])).cuda()
    rows = torch.tensor([[600, 300], [1400, 700]], dtype=torch.int32, device='cuda')
    G = Guarded({'wave': ((B, L), torch.float32, 7.0)})
    fn = C.CDLL(lib.LIB_PATH).taco_wave_resample
    fn.restype, fn.argtypes = lib.EXPORTS['taco_wave_resample']
    good = dict(pcm=lib.ptr(pcm), row_bytes=pcm.shape[1], width=2, channels=2, rows=lib.ptr(rows), taps=lib.ptr(taps), P=P, Q=Q,
                n_left=n_left, n_right=n_right, wave=lib.ptr(G['wave']), B=B, L=L)
    order = ('pcm', 'row_bytes', 'width', 'channels', 'rows', 'taps', 'P', 'Q', 'n_left', 'n_right', 'wave', 'B', 'L')
    cases = [{'pcm': None}, {'rows': None}, {'wave': None}, {'taps': None}, {'width': 0}, {'width': 5}, {'width': -1}, {'channels': 0},
             {'channels': 9}, {'P': 0}, {'Q': 0}, {'P': -2}, {'Q': -1}, {'n_left': 0}, {'n_right': 0}, {'n_left': -3}, {'B': 0}, {'B': -1},
             {'B': 65536}, {'L': 0}, {'L': -5}, {'row_bytes': 0}, {'row_bytes': -4}, {'row_bytes': pcm.shape[1] - 1},
             {'width': 3}, {'P': 64}]   # (5600 bytes are no multiple of 6; 64 frames per output do not fit the LDS)
    assert pcm.shape[1] % 6 != 0
    everything = torch.ones(B, L, dtype=torch.bool, device='cuda')
    for change in cases:
        a = dict(good)
        a.update(change)
        lib.audio_features_workspace_bytes(1, 1)   # (a successful call in between: the string below is this refusal's)
        rc = fn(*[a[k] for k in order], lib.stream_ptr())
        torch.cuda.synchronize()
        msg = lib.last_error()
        print('  %r: rc %d, %s' % (change, rc, msg))
        assert rc == -1, (change, rc)
        assert 'wave_resample' in msg
        assert G.margin_intact('wave', everything), 'wave was written although %r is refused' % (change,)
    G.check()
    # and the good arguments do run; decode-only with taps NULL as well
    for change in ({}, {'P': 1, 'Q': 1, 'taps': None}, {'P': 3, 'Q': 3}):
        a = dict(good)
        a.update(change)
        G.refill('wave')
        assert fn(*[a[k] for k in order], lib.stream_ptr()) == 0, change
        torch.cuda.synchronize()
        G.check()
        w = G['wave'].cpu().numpy()
        assert np.isfinite(w).all() and w[0, :300].any() and not bits(w[0, 300:]).any()


# ---- the pipeline ---------------------------------------------------------------------------------------------------------------
def test_preprocess_on_the_device_path(built_lib, tmp_path):
    """four 0.3 s 48 kHz PCM16 files -> preprocess(sr=24000, max_len=6000, resample='device'): mels / stfts are process_audio on
    load_batch_device's own waves bit for bit; texts, text_lens, speech_lens and meta.pkl are those of resample='host'.  (The features
    of the two paths are not compared: the filters differ, on purpose.)"""
    from tacotron_amd import audio, preprocess
    n = 14400
    t = np.arange(n) / 48000.0
    rng = np.random.default_rng(11)
    files, prompts = [], ['first prompt.', 'the second one', 'third!', 'and a fourth, longer prompt']
    spans = [(2400, 9600), (1000, 8000), (0, n), (4800, 12000)]   # the third is loud throughout: 7200 samples at 24 kHz > max_len, dropped
    for i, (lo, hi) in enumerate(spans):
        x = np.zeros(n)
        x[lo:hi] = 0.4 * np.sin(2 * np.pi * (300.0 + 170.0 * i) * t[lo:hi]) + 0.05 * rng.standard_normal(hi - lo)
        path = str(tmp_path / ('u%d.wav' % i))
        with wavefile.open(path, 'wb') as f:
            f.setnchannels(1)
            f.setsampwidth(2)
            f.setframerate(48000)
            f.writeframes(np.round(x * 32767.0).astype('<i2').tobytes())
        files.append(path)
    data = {'prompts': prompts, 'audio_files': files}
    dev_dir, host_dir = tmp_path / 'device', tmp_path / 'host'
    kept_n = preprocess.preprocess(data, str(dev_dir), sr=24000, max_len=6000, batch=3, verbose=False, resample='device')
    assert kept_n == 3
    waves, lengths = audio.load_batch_device(files, 24000)
    assert lengths == [7200] * 4 and tuple(waves.shape) == (4, 7200)
    mel, stft, kept, _ = audio.process_audio(waves, lengths, 2, 6000, torch.float16)
    keep = np.flatnonzero(kept.cpu().numpy())
    assert keep.tolist() == [0, 1, 3]
    assert same_bits(np.load(dev_dir / 'mels.npy'), mel.cpu().numpy()[keep])
    assert same_bits(np.load(dev_dir / 'stfts.npy'), stft.cpu().numpy()[keep])
    assert preprocess.preprocess(data, str(host_dir), sr=24000, max_len=6000, batch=3, verbose=False) == 3
    for name in ('texts', 'text_lens', 'speech_lens'):
        assert open(dev_dir / (name + '.npy'), 'rb').read() == open(host_dir / (name + '.npy'), 'rb').read(), name
    with open(dev_dir / 'meta.pkl', 'rb') as a, open(host_dir / 'meta.pkl', 'rb') as b:
        ma, mb = pickle.load(a), pickle.load(b)
    assert ma == mb and ma['sr'] == 24000 and ma['r'] == 2
    assert np.load(dev_dir / 'mels.npy').shape == np.load(host_dir / 'mels.npy').shape == (3, 8, 160)
