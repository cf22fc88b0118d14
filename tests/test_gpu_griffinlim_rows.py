"""GPU: Griffin-Lim per utterance (include/taco_hip.h taco_griffinlim_rows) -- device frame counts and seeded device phases.

Row b of a batch is vocoded over its own first F_b = min(F, frames[b] * frames_per_unit) frames.  The yardsticks:
  - taco_griffinlim of that row alone (B = 1, F = F_b, the first F_b columns copied contiguous): the samples below 300 (F_b - 1)
    are the same BITS, everything behind them is exactly 0;
  - the fp64 NumPy restatement of the librosa algorithm (oracle/griffinlim_numpy.py) on those columns, at the tolerances
    tests/test_gpu_vocoder.py uses: rel-L2 < 2e-5 for n_iter <= 1, < 1e-3 after 3 rounds (and 1e-3 for the model pipeline, the
    bound of its test_output_to_waveform_pipeline);
  - the device phases against the oracle fed the angles of the integer restatement of the hash (tests/phase_ref.py).
Waveform and workspace are the tests' own buffers between guard bands, filled with NaN before every call (tests/poison.py)."""
import ctypes as C
import os
import wave

import numpy as np
import pytest
import torch

from oracle import griffinlim_numpy as gl
from tests.phase_ref import phase_angles
from tests.poison import Guarded
from tests.util import rel_l2

pytestmark = pytest.mark.gpu

B5, F41 = 5, 41
FRAMES5 = [41, 24, 8, 3, 50]


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def row_frames(frames, F, per_unit=1):
    """F_b of every row, and the frames that are vocoded (0 for a row below 5 frames)"""
    fb = [min(F, int(f) * per_unit) for f in frames]
    return fb, [f if f >= 5 else 0 for f in fb]


def _case(F, seed):
    """as tests/test_gpu_vocoder.py: a magnitude matrix that IS the STFT of a signal, plus noise-floor bins; random phases"""
    rng = np.random.default_rng(seed)
    y = np.cumsum(rng.standard_normal(300 * (F - 1))) * 0.01 + np.sin(np.arange(300 * (F - 1)) * 0.05)
    mag = np.abs(gl.stft(y)) + 1e-3
    ph = 2 * np.pi * rng.random(mag.shape)
    return mag, ph


def _batch(B=B5, F=F41, seed=3):
    mags, phs = zip(*[_case(F, seed + b) for b in range(B)])
    mag = np.stack(mags).astype(np.float32) * np.array([1.0, 0.5, 2.0, 1.0, 0.25], dtype=np.float32)[:B, None, None]
    return mag, np.stack(phs).astype(np.float32)


def dev(x, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(x), dtype=dtype, device='cuda')


def _griffinlim(lib, m, p, n_iter):
    """lib.griffinlim into a poisoned waveform buffer with a poisoned workspace, between guard bands"""
    B, _, F = m.shape
    G = Guarded({'wave': ((B, 300 * (F - 1)), torch.float32, 'qnan'),
                 'work': ((lib.griffinlim_workspace_floats(B, F),), torch.float32, 'qnan')})
    w = lib.griffinlim(m, p, n_iter, out=G['wave'], work=G['work'])
    torch.cuda.synchronize()
    G.check('wave')
    return w.cpu().numpy()


def _rows(lib, m, frames, p=None, seed=0, n_iter=0, per_unit=1):
    """lib.griffinlim_rows the same way; every sample of every row must have been written"""
    B, _, F = m.shape
    G = Guarded({'wave': ((B, 300 * (F - 1)), torch.float32, 'qnan'),
                 'work': ((lib.griffinlim_rows_workspace_floats(B, F),), torch.float32, 'qnan')})
    fr = frames if torch.is_tensor(frames) else dev(frames, torch.int32)
    w = lib.griffinlim_rows(m, fr, phase0=p, seed=seed, n_iter=n_iter, frames_per_unit=per_unit, out=G['wave'], work=G['work'])
    assert w is G['wave']
    torch.cuda.synchronize()
    G.check('wave')
    assert bool(torch.isfinite(w).all())
    return w.cpu().numpy()


def _check_tails(w, frames, F, per_unit=1):
    _, act = row_frames(frames, F, per_unit)
    for b, fa in enumerate(act):
        n = 300 * (fa - 1) if fa else 0
        assert not bits(w[b, n:]).any(), 'row %d is not exactly 0 from sample %d on' % (b, n)
        if fa:
            assert w[b, :n].any(), 'row %d is silent' % b


@pytest.mark.parametrize('n_iter', [0, 1, 3])
def test_rows_equal_griffinlim_of_each_row_alone(built_lib, n_iter):
    """(1) per-row identity with taco_griffinlim, (2) the oracle, (3) the columns from F_b on are never read"""
    mag, ph = _batch()
    m, p = dev(mag), dev(ph)
    w = _rows(built_lib, m, FRAMES5, p, n_iter=n_iter)
    fb, act = row_frames(FRAMES5, F41)
    assert fb == [41, 24, 8, 3, 41] and act == [41, 24, 8, 0, 41]      # row 3 is below 5 frames, row 4 clamps to F
    _check_tails(w, FRAMES5, F41)
    assert not bits(w[3]).any()
    for b, fa in enumerate(act):
        if not fa:
            continue
        n = 300 * (fa - 1)
        alone = _griffinlim(built_lib, m[b:b + 1, :, :fa].contiguous(), p[b:b + 1, :, :fa].contiguous(), n_iter)
        assert alone.shape == (1, n)
        assert same_bits(w[b, :n], alone[0]), 'row %d (%d frames) is not taco_griffinlim of that row alone' % (b, fa)
        ref = gl.griffinlim(mag[b][:, :fa].astype(np.float64), ph[b][:, :fa].astype(np.float64), n_iter)
        e = rel_l2(w[b, :n], ref)
        print('  n_iter=%d row %d F_b=%d: waveform rel-L2 %.2e' % (n_iter, b, fa, e))
        assert ref.shape == (n,) and e < (2e-5 if n_iter <= 1 else 1e-3)
    # the tail is not read: NaN in every column t >= F_b of the magnitudes and of the phases
    mn, pn = m.clone(), p.clone()
    for b, f in enumerate(fb):
        mn[b, :, f:] = float('nan')
        pn[b, :, f:] = float('nan')
    assert bool(torch.isnan(mn[1, :, 24:]).all()) and bool(torch.isfinite(mn[4]).all())
    assert same_bits(_rows(built_lib, mn, FRAMES5, pn, n_iter=n_iter), w)


def test_frames_per_unit(built_lib):
    mag, ph = _batch(B=2, F=24)
    m, p = dev(mag), dev(ph)
    a = _rows(built_lib, m, [8, 4], p, n_iter=2, per_unit=2)
    b = _rows(built_lib, m, [16, 8], p, n_iter=2, per_unit=1)
    _check_tails(a, [8, 4], 24, 2)
    assert same_bits(a, b)
    assert not same_bits(a, _rows(built_lib, m, [8, 4], p, n_iter=2, per_unit=1))
    # a product past int32 clamps to F instead of wrapping
    big = _rows(built_lib, m, [2 ** 31 - 1, 8], p, n_iter=2, per_unit=2 ** 31 - 1)
    full = _rows(built_lib, m, [24, 24], p, n_iter=2)
    assert same_bits(big, full)
    neg = _rows(built_lib, m, [-(2 ** 31), 0], p, n_iter=2, per_unit=2 ** 31 - 1)
    assert not bits(neg).any()


@pytest.mark.parametrize('n_iter', [0, 1])
def test_device_phases(built_lib, n_iter):
    """phase0 = None: the phases are the counter hash of (seed, element index), restated in integers on the host"""
    mag, _ = _batch()
    m = dev(mag)
    w = _rows(built_lib, m, FRAMES5, None, seed=5, n_iter=n_iter)
    _check_tails(w, FRAMES5, F41)
    ang = phase_angles(5, B5, F41)                      # (B, 1025, F): the element index runs over the pitch F, not F_b
    _, act = row_frames(FRAMES5, F41)
    for b, fa in enumerate(act):
        if not fa:
            continue
        n = 300 * (fa - 1)
        ref = gl.griffinlim(mag[b][:, :fa].astype(np.float64), ang[b][:, :fa], n_iter)
        e = rel_l2(w[b, :n], ref)
        print('  device phases n_iter=%d row %d F_b=%d: waveform rel-L2 %.2e' % (n_iter, b, fa, e))
        assert e < 2e-5
    # the same seed again: the same bits; another seed: another waveform in every row that has one
    assert same_bits(_rows(built_lib, m, FRAMES5, None, seed=5, n_iter=n_iter), w)
    w6 = _rows(built_lib, m, FRAMES5, None, seed=6, n_iter=n_iter)
    for b, fa in enumerate(act):
        if fa:
            n = 300 * (fa - 1)
            assert rel_l2(w6[b, :n], w[b, :n]) > 0.1, 'row %d: seeds 5 and 6 give the same waveform' % b
    # seeds use all 64 bits
    assert not same_bits(_rows(built_lib, m, FRAMES5, None, seed=5 + 2 ** 32, n_iter=n_iter), w)
    # a row's samples do not depend on the other rows' lengths
    other = [10, 24, 41, 30, 6]
    w2 = _rows(built_lib, m, other, None, seed=5, n_iter=n_iter)
    assert same_bits(w2[1], w[1])
    w3 = _rows(built_lib, m, [41, 5, 5, 5, 5], None, seed=5, n_iter=n_iter)
    assert same_bits(w3[0], w[0])


def test_graph_replay_follows_the_device_lengths(built_lib):
    """One capture on a side stream; the replay reads `frames` from the device at replay time."""
    mag, ph = _batch(B=3, F=24)
    m, p = dev(mag), dev(ph)
    n_iter = 2
    first, second = [24, 12, 6], [9, 24, 3]
    frames = dev(first, torch.int32)
    G = Guarded({'wave': ((3, 300 * 23), torch.float32, 'qnan'),
                 'work': ((built_lib.griffinlim_rows_workspace_floats(3, 24),), torch.float32, 'qnan')})
    call = lambda: built_lib.griffinlim_rows(m, frames, phase0=p, n_iter=n_iter, out=G['wave'], work=G['work'])   # noqa: E731
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            call()
    torch.cuda.synchronize()
    for fr in (first, second, first):
        frames.copy_(dev(fr, torch.int32))
        G.refill('wave', 'work')
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        G.check('wave')
        got = G['wave'].cpu().numpy()
        want = _rows(built_lib, m, fr, p, n_iter=n_iter)
        assert same_bits(got, want), 'replay with frames %s differs from the eager call' % (fr,)
        _check_tails(got, fr, 24)


RULE = dict(end_offset=200, hold=1, min_steps=5)   # target 0: every row stops after step 4 -> len_b = 8


def _model(Td=16, B=3, Tt=24, seed=3):
    from tacotron_amd.config import Config
    from tacotron_amd.data import synthetic_batch
    from tacotron_amd.model import Tacotron
    c = Config()
    c.r, c.vocab_size, c.max_decode_iter = 2, 30, Td
    return Tacotron(c, synthetic_batch(B, Tt, Td, 2, 30, seed=seed, min_len=8), train=False, seed=5)


@pytest.mark.parametrize('lengths', ['model', [8, 16, 4]])
def test_model_output_to_waveform_per_row(built_lib, lengths):
    """Tacotron.run(stop=rule) -> invert_spectrogram(..., lengths=...): every row is the Griffin-Lim of its own len_b r frames --
    and not the cut of today's full-length waveform, which the frames behind len_b leak into."""
    from tacotron_amd.audio import denormalize, reshape_frames
    from tacotron_amd.griffinlim import invert_spectrogram
    B, Td, r = 3, 16, 2
    F = (Td // 4) * 4 * r
    m = _model(Td, B)
    out, _ = m.run(stop=built_lib.TacoStopRule(**RULE))
    m.check()
    torch.cuda.synchronize()
    assert m.lengths.dtype == torch.int32 and m.lengths.tolist() == [8, 8, 8]
    ln = m.lengths if lengths == 'model' else dev(lengths, torch.int32)
    rng = np.random.default_rng(5)
    mean = rng.standard_normal(1025 * r).astype(np.float32) * 0.1 - 2.0
    std = (0.5 + rng.random(1025 * r)).astype(np.float32)
    ph = (2 * np.pi * rng.random((B, 1025, F))).astype(np.float32)
    G = Guarded({'mag_t': ((B, 1025, F), torch.float32, 'qnan'), 'wave': ((B, 300 * (F - 1)), torch.float32, 'qnan'),
                 'work': ((built_lib.griffinlim_rows_workspace_floats(B, F),), torch.float32, 'qnan')})
    w = invert_spectrogram(out, mean, std, r, n_iter=2, lengths=ln, phase0=dev(ph), mag_t=G['mag_t'], wave=G['wave'], work=G['work'])
    torch.cuda.synchronize()
    G.check('mag_t', 'wave')
    w = w.cpu().numpy()
    today = invert_spectrogram(out, mean, std, r, n_iter=2, phase0=dev(ph)).cpu().numpy()   # full length, cut afterwards
    assert today.shape == w.shape == (B, 300 * (F - 1))
    out_h = out.cpu().numpy()
    lens = ln.cpu().numpy().tolist()
    _check_tails(w, lens, F, r)
    for b, L in enumerate(lens):
        fa = L * r
        n = 300 * (fa - 1)
        spec = reshape_frames(denormalize(out_h[b].astype(np.float64), mean.astype(np.float64), std.astype(np.float64)), r, forward=False)
        assert spec.shape == (F, 1025)
        ref = gl.griffinlim(np.exp(spec[:fa].T), ph[b][:, :fa].astype(np.float64), 2)
        e, d = rel_l2(w[b, :n], ref), rel_l2(today[b, :n], w[b, :n])
        print('  lengths %s row %d len_b=%d: vs oracle rel-L2 %.2e; cut full-length waveform vs this one %.2e' % (lens, b, L, e, d))
        assert e < 1e-3
        if L == Td:
            assert same_bits(w[b], today[b])   # a row that runs to the end is the row of today's path
        if L < Td:
            # were the two closer than twice the oracle bound, the cut waveform would pass the check above as well
            assert d > 2e-3, 'row %d: the per-row waveform does not differ from the cut full-length one' % b


def test_driver_vocodes_with_the_lengths(built_lib, tmp_path):
    """tacotron_amd.test.test(..., stop=rule, vocode_lengths=True): files of the same sizes and the same spectrogram / alignment /
    length files as without the option; the samples are those of invert_spectrogram with model.lengths and device phases."""
    from tacotron_amd import test as drv
    from tacotron_amd.config import Config
    from tacotron_amd.data import load_prompts
    from tacotron_amd.griffinlim import invert_spectrogram
    from tacotron_amd.model import Tacotron
    from tacotron_amd.params import ParamBuffer
    prompts = ['hello world.\n', 'a somewhat longer prompt, with punctuation!\n', 'short\n']

    def cfg():
        c = Config()
        c.data_path = str(tmp_path / 'no_data') + '/'
        c.max_decode_iter = 16
        return c

    rule = built_lib.TacoStopRule(**RULE)
    with pytest.raises(ValueError):
        drv.test(cfg(), prompts, out_dir=str(tmp_path / 'bad'), n_iter=2, vocode_lengths=True)
    assert not (tmp_path / 'bad').exists()
    cut, rows, ref = tmp_path / 'cut', tmp_path / 'rows', tmp_path / 'ref'
    assert drv.test(cfg(), prompts, out_dir=str(cut), n_iter=2, stop=rule) == 3
    assert drv.test(cfg(), prompts, out_dir=str(rows), n_iter=2, stop=rule, vocode_lengths=True) == 3
    # the driver's path with the option, restated
    c = cfg()
    ivocab = {i + 1: ch for i, ch in enumerate("abcdefghijklmnopqrstuvwxyz '.,?!-")}
    ivocab[0] = '<pad>'
    c.vocab_size = len(ivocab)
    os.makedirs(ref)
    batch = next(load_prompts(prompts, ivocab))
    shape = built_lib.make_shape(3, batch['text'].shape[1], c.max_decode_iter, c.r, c.vocab_size, c.num_speakers)
    m = Tacotron(c, batch, train=False, params=ParamBuffer(shape, 'cuda').init_(0))
    out, _ = m.run(stop=rule)
    nb = c.fft_size * c.r
    wav = invert_spectrogram(out, torch.zeros(nb).cuda(), torch.ones(nb).cuda(), c.r, n_iter=2, seed=0, lengths=m.lengths).cpu().numpy()
    n = 300 * (8 * c.r - 1)
    assert not bits(wav[:, n:]).any()
    for i in range(3):
        assert int(np.load(rows / ('prompt_%03d_len.npy' % i))) == 8
        for kind in ('len', 'spec', 'align'):
            name = 'prompt_%03d_%s.npy' % (i, kind)
            assert open(rows / name, 'rb').read() == open(cut / name, 'rb').read(), name
        with wave.open(str(rows / ('prompt_%03d.wav' % i))) as f:
            assert f.getnframes() == n
        drv.write_wav(str(ref / ('prompt_%03d.wav' % i)), wav[i, :n])
        got = open(rows / ('prompt_%03d.wav' % i), 'rb').read()
        assert got == open(ref / ('prompt_%03d.wav' % i), 'rb').read()
        assert got != open(cut / ('prompt_%03d.wav' % i), 'rb').read()


def test_bad_arguments_enqueue_nothing(built_lib):
    """every TACO_EINVAL case of the C ABI returns before a launch: the poisoned waveform and workspace keep their fill"""
    lib = built_lib
    B, F = 2, 8
    mag, ph = _batch(B=B, F=F)
    m, p, fr = dev(mag), dev(ph), dev([8, 6], torch.int32)
    G = Guarded({'wave': ((B, 300 * (F - 1)), torch.float32, 'qnan'),
                 'work': ((lib.griffinlim_rows_workspace_floats(B, F),), torch.float32, 'qnan')})
    fn = C.CDLL(lib.LIB_PATH).taco_griffinlim_rows
    fn.restype, fn.argtypes = lib.EXPORTS['taco_griffinlim_rows']
    good = dict(mag_t=lib.ptr(m), phase0=lib.ptr(p), seed=1, frames=lib.ptr(fr), per_unit=1, wave=lib.ptr(G['wave']),
                work=lib.ptr(G['work']), B=B, F=F, n_iter=1)
    order = ('mag_t', 'phase0', 'seed', 'frames', 'per_unit', 'wave', 'work', 'B', 'F', 'n_iter')
    cases = [('mag_t', None), ('frames', None), ('wave', None), ('work', None), ('B', 0), ('B', -1), ('F', 4), ('F', 0),
             ('n_iter', -1), ('per_unit', 0), ('per_unit', -2)]
    everything = torch.ones(G['wave'].shape, dtype=torch.bool, device='cuda')
    for key, val in cases:
        a = dict(good)
        a[key] = val
        torch.cuda.synchronize()
        rc = fn(*[a[k] for k in order], lib.stream_ptr())
        torch.cuda.synchronize()
        print('  %s = %r: rc %d, %s' % (key, val, rc, lib.last_error()))
        assert rc == -1, (key, val, rc)
        assert G.margin_intact('wave', everything), 'wave was written although %s = %r is refused' % (key, val)
        assert bool(torch.isnan(G['work']).all())
    for Bx, Fx in ((0, 8), (2, 4)):
        with pytest.raises(lib.TacoError):
            lib.griffinlim_rows_workspace_floats(Bx, Fx)
    # and the good arguments do run (phase0 NULL as well)
    for ph0 in (good['phase0'], None):
        a = dict(good)
        a['phase0'] = ph0
        G.refill('wave', 'work')
        assert fn(*[a[k] for k in order], lib.stream_ptr()) == 0
        torch.cuda.synchronize()
        G.check('wave')
        assert bool(torch.isfinite(G['wave']).all())
