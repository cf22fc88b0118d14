"""GPU: fast Griffin-Lim (include/taco_hip.h taco_griffinlim_fast) -- momentum rounds and the per-round convergence readout.

The yardsticks:
  - the two older entry points, bit for bit: momentum 0 IS taco_griffinlim_rows / taco_griffinlim; a first round has no
    predecessor, so n_iter <= 1 does not depend on the momentum; the readout changes no sample; a row of a batch is the B = 1 call
    on that row alone, samples and readout;
  - the fp64 restatement tests/fgl_ref.py on inputs rounded to fp32: waveform rel-L2 < 1e-3 after 2 and 3 momentum rounds (the bar
    tests/test_gpu_vocoder.py sets for 3 plain rounds); conv[:, 0] and conv[:, n_iter] within 4e-5 absolute of the restatement's
    first value and of oracle spectral_convergence(device waveform) (twice the 2e-5 rel-L2 bar of one synthesis + analysis pass:
    the device's pass and the fp32 waveform the host analyses again); the rounds in between within 2 % + 1e-3, the project's bar
    for a many-round result;
  - the claim itself, on the device: momentum 0.99 / 30 rounds ends below the restatement's plain 50 rounds on the four inputs of
    DESIGN.md 4b, next to a device plain 50-round call that agrees with that value.
Waveform, readout and workspace are the tests' own buffers between guard bands, filled with NaN before every call."""
import ctypes as C
import wave as wavefile

import numpy as np
import pytest
import torch

from oracle import griffinlim_numpy as gl
from tests import fgl_ref
from tests.poison import Guarded
from tests.util import rel_l2

pytestmark = pytest.mark.gpu

MANY = lambda ref: 0.02 * ref + 1e-3   # noqa: E731  (the bar for a many-round figure)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def dev(x, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(x), dtype=dtype, device='cuda')


def _batch(F, seeds, scale=(1.0, 0.5, 2.0, 0.25)):
    mags, phs = zip(*[fgl_ref.case(F, s) for s in seeds])
    mag = np.stack(mags).astype(np.float32) * np.array(scale, dtype=np.float32)[:len(seeds), None, None]
    return mag, np.stack(phs).astype(np.float32)


def _fast(lib, m, frames=None, p=None, seed=0, n_iter=0, momentum=0.99, conv=True, per_unit=1):
    """lib.griffinlim_fast into NaN-filled buffers between guard bands; every element of the outputs must have been written"""
    B, _, F = m.shape
    spec = {'wave': ((B, 300 * (F - 1)), torch.float32, 'qnan'),
            'work': ((lib.griffinlim_fast_workspace_floats(B, F),), torch.float32, 'qnan')}
    if conv:
        spec['conv'] = ((B, n_iter + 1), torch.float32, 'qnan')
    G = Guarded(spec)
    fr = frames if frames is None or torch.is_tensor(frames) else dev(frames, torch.int32)
    r = lib.griffinlim_fast(m, fr, phase0=p, seed=seed, n_iter=n_iter, momentum=momentum, frames_per_unit=per_unit,
                            out=G['wave'], conv=G['conv'] if conv else None, work=G['work'])
    torch.cuda.synchronize()
    w = r[0] if conv else r
    assert w is G['wave'] and (not conv or r[1] is G['conv'])
    G.check(*(('wave', 'conv') if conv else ('wave',)))
    assert bool(torch.isfinite(w).all())
    if not conv:
        return w.cpu().numpy(), None
    assert bool(torch.isfinite(G['conv']).all())
    return w.cpu().numpy(), G['conv'].cpu().numpy()


def _rows(lib, m, frames, p, seed, n_iter):
    B, _, F = m.shape
    G = Guarded({'wave': ((B, 300 * (F - 1)), torch.float32, 'qnan'),
                 'work': ((lib.griffinlim_rows_workspace_floats(B, F),), torch.float32, 'qnan')})
    w = lib.griffinlim_rows(m, dev(frames, torch.int32), phase0=p, seed=seed, n_iter=n_iter, out=G['wave'], work=G['work'])
    torch.cuda.synchronize()
    G.check('wave')
    return w.cpu().numpy()


def _plain(lib, m, p, n_iter):
    B, _, F = m.shape
    G = Guarded({'wave': ((B, 300 * (F - 1)), torch.float32, 'qnan'),
                 'work': ((lib.griffinlim_workspace_floats(B, F),), torch.float32, 'qnan')})
    w = lib.griffinlim(m, p, n_iter, out=G['wave'], work=G['work'])
    torch.cuda.synchronize()
    G.check('wave')
    return w.cpu().numpy()


FR4 = [41, 24, 3, 0]


@pytest.mark.parametrize('n_iter', [0, 1, 3])
def test_momentum_0_is_the_plain_algorithm_bit_for_bit(built_lib, n_iter):
    """guarantee 1: taco_griffinlim_rows (frames given, phases given and drawn) and taco_griffinlim (frames NULL)"""
    mag, ph = _batch(41, (3, 4, 5, 6))
    m, p = dev(mag), dev(ph)
    for want_conv in (False, True):
        w, _ = _fast(built_lib, m, FR4, p, n_iter=n_iter, momentum=0.0, conv=want_conv)
        assert same_bits(w, _rows(built_lib, m, FR4, p, 0, n_iter)), 'frames + phase0, conv %s' % want_conv
        w, _ = _fast(built_lib, m, FR4, None, seed=7, n_iter=n_iter, momentum=0.0, conv=want_conv)
        assert same_bits(w, _rows(built_lib, m, FR4, None, 7, n_iter)), 'frames + device phases, conv %s' % want_conv
        w, _ = _fast(built_lib, m, None, p, n_iter=n_iter, momentum=0.0, conv=want_conv)
        assert same_bits(w, _plain(built_lib, m, p, n_iter)), 'frames NULL, conv %s' % want_conv


@pytest.mark.parametrize('n_iter', [0, 1])
def test_first_round_does_not_depend_on_the_momentum(built_lib, n_iter):
    """guarantee 2 -- and two rounds do depend on it"""
    mag, ph = _batch(24, (3, 4))
    m, p = dev(mag), dev(ph)
    for frames in (None, [24, 9]):
        w0, c0 = _fast(built_lib, m, frames, p, n_iter=n_iter, momentum=0.0)
        for a in (0.5, 0.99):
            w, c = _fast(built_lib, m, frames, p, n_iter=n_iter, momentum=a)
            assert same_bits(w, w0) and same_bits(c, c0), 'momentum %g, frames %s' % (a, frames)
            assert same_bits(_fast(built_lib, m, frames, p, n_iter=n_iter, momentum=a, conv=False)[0], w0)
    w2, _ = _fast(built_lib, m, None, p, n_iter=2, momentum=0.0)
    assert rel_l2(_fast(built_lib, m, None, p, n_iter=2, momentum=0.99)[0], w2) > 1e-3


@pytest.mark.parametrize('momentum', [0.0, 0.5, 0.99])
def test_readout_changes_no_sample_and_calls_repeat(built_lib, momentum):
    """guarantees 3 and 5"""
    mag, ph = _batch(24, (3, 4, 5))
    m, p = dev(mag), dev(ph)
    for frames, p0 in ((None, p), (None, None), ([24, 11, 6], p), ([24, 11, 6], None)):
        w, c = _fast(built_lib, m, frames, p0, seed=3, n_iter=4, momentum=momentum, conv=True)
        w_no, _ = _fast(built_lib, m, frames, p0, seed=3, n_iter=4, momentum=momentum, conv=False)
        assert same_bits(w, w_no), 'the waveform depends on conv (frames %s, phase0 %s)' % (frames, p0 is not None)
        w2, c2 = _fast(built_lib, m, frames, p0, seed=3, n_iter=4, momentum=momentum, conv=True)
        assert same_bits(w, w2) and same_bits(c, c2)
        assert (c > 0).all() and (c[:, 1:] < c[:, :1]).all()


@pytest.mark.parametrize('momentum', [0.0, 0.99])
def test_rows_are_the_call_on_each_row_alone(built_lib, momentum):
    """guarantee 4: samples and readout of row b = the B = 1, F = F_b call; zeros behind; nothing read past F_b"""
    F, frames, n_iter = 96, [96, 40, 3, 0], 4
    mag, ph = _batch(F, (3, 4, 5, 6))
    m, p = dev(mag), dev(ph)
    for p0 in (p, None):
        w, c = _fast(built_lib, m, frames, p0, seed=9, n_iter=n_iter, momentum=momentum)
        for b, fb in enumerate(frames):
            n = 300 * (fb - 1) if fb >= 5 else 0
            assert not bits(w[b, n:]).any(), 'row %d is not exactly 0 from sample %d on' % (b, n)
            if fb < 5:
                assert not bits(c[b]).any(), 'row %d has no frames and a readout' % b
                continue
            assert w[b, :n].any()
            if p0 is None:
                continue   # (the hash runs over the pitch F: a contiguous copy of the row draws other phases)
            wa, ca = _fast(built_lib, m[b:b + 1, :, :fb].contiguous(), None, p[b:b + 1, :, :fb].contiguous(), n_iter=n_iter,
                           momentum=momentum)
            assert same_bits(w[b, :n], wa[0]), 'row %d (%d frames): samples differ from the row alone' % (b, fb)
            assert same_bits(c[b], ca[0]), 'row %d (%d frames): readout differs from the row alone' % (b, fb)
        # NaN in every column t >= F_b
        mn, pn = m.clone(), p.clone()
        for b, fb in enumerate(frames):
            mn[b, :, fb:] = float('nan')
            pn[b, :, fb:] = float('nan')
        wn, cn = _fast(built_lib, mn, frames, None if p0 is None else pn, seed=9, n_iter=n_iter, momentum=momentum)
        assert same_bits(wn, w) and same_bits(cn, c)
        # a row's results do not depend on the other rows' lengths
        wo, co = _fast(built_lib, m, [7, 40, 96, 50], p0, seed=9, n_iter=n_iter, momentum=momentum)
        assert same_bits(wo[1], w[1]) and same_bits(co[1], c[1])
    # frames_per_unit multiplies
    a = _fast(built_lib, m, [48, 20, 2, 0], p, n_iter=2, momentum=momentum, per_unit=2)
    b2 = _fast(built_lib, m, [96, 40, 4, 0], p, n_iter=2, momentum=momentum)
    assert same_bits(a[0], b2[0]) and same_bits(a[1], b2[1])


@pytest.mark.parametrize('F,seed', [(8, 3), (41, 3)])
@pytest.mark.parametrize('n_iter', [2, 3])
def test_against_the_fp64_restatement(built_lib, F, seed, n_iter):
    mag, ph = fgl_ref.fp32_inputs(fgl_ref.case, F, seed)
    w, c = _fast(built_lib, dev(mag[None]), None, dev(ph[None]), n_iter=n_iter, momentum=0.99)
    mag64 = mag.astype(np.float64)
    ref_w, ref_c = fgl_ref.griffinlim_fast(mag64, ph.astype(np.float64), n_iter, 0.99)
    e = rel_l2(w[0], ref_w)
    d0 = abs(float(c[0, 0]) - ref_c[0])
    sc = gl.spectral_convergence(w[0].astype(np.float64), mag64)
    dn = abs(float(c[0, n_iter]) - sc)
    print('  case(%d, %d) momentum 0.99 n_iter=%d: waveform rel-L2 %.2e; conv[0] %.6f vs %.6f (|d| %.1e); conv[n] %.6f vs host %.6f '
          '(|d| %.1e), restatement %.6f; in between %s vs %s'
          % (F, seed, n_iter, e, c[0, 0], ref_c[0], d0, c[0, n_iter], sc, dn, ref_c[-1], c[0, 1:n_iter], ref_c[1:n_iter]))
    assert ref_w.shape == w[0].shape and e < 1e-3
    assert d0 <= 4e-5 and dn <= 4e-5
    assert (np.abs(c[0, 1:n_iter] - ref_c[1:n_iter]) <= MANY(ref_c[1:n_iter])).all()


@pytest.mark.parametrize('name,fn,F,seed', fgl_ref.CASES, ids=[c[0] for c in fgl_ref.CASES])
def test_30_momentum_rounds_end_below_50_plain_ones(built_lib, name, fn, F, seed):
    mag, ph = fgl_ref.fp32_inputs(fn, F, seed)
    m, p = dev(mag[None]), dev(ph[None])
    mag64, ph64 = mag.astype(np.float64), ph.astype(np.float64)
    _, ref_fast = fgl_ref.griffinlim_fast(mag64, ph64, 30, 0.99)
    _, ref_plain = fgl_ref.griffinlim_fast(mag64, ph64, 50, 0.0)
    w, c = _fast(built_lib, m, None, p, n_iter=30, momentum=0.99)
    wp, cp = _fast(built_lib, m, None, p, n_iter=50, momentum=0.0)
    sc = gl.spectral_convergence(w[0].astype(np.float64), mag64)
    worst = float(np.max(np.abs(c[0, 1:30] - ref_fast[1:30]) / MANY(ref_fast[1:30])))
    print('  %s: device momentum 0.99 / 30 rounds %.5f (restatement %.5f, host readout of the device waveform %.5f); plain 50 rounds '
          'device %.5f restatement %.5f; conv[0] device %.6f restatement %.6f; rounds 1..29 worst |d| / bar %.3f'
          % (name, c[0, 30], ref_fast[30], sc, cp[0, 50], ref_plain[50], c[0, 0], ref_fast[0], worst))
    assert abs(float(c[0, 0]) - ref_fast[0]) <= 4e-5 and abs(float(c[0, 30]) - sc) <= 4e-5
    assert same_bits(c[:, :1], cp[:, :1])
    assert (np.abs(c[0, 1:30] - ref_fast[1:30]) <= MANY(ref_fast[1:30])).all()
    assert abs(float(c[0, 30]) - ref_fast[30]) <= MANY(ref_fast[30])
    assert abs(float(cp[0, 50]) - ref_plain[50]) <= MANY(ref_plain[50])
    assert float(c[0, 30]) < ref_plain[50]


def test_bad_arguments_enqueue_nothing(built_lib):
    """every TACO_EINVAL case returns before a launch: waveform, readout and workspace keep their fill; the error string is set"""
    lib = built_lib
    B, F, n_iter = 2, 8, 2
    mag, ph = _batch(F, (3, 4))
    m, p, fr = dev(mag), dev(ph), dev([8, 6], torch.int32)
    G = Guarded({'wave': ((B, 300 * (F - 1)), torch.float32, 'qnan'), 'conv': ((B, n_iter + 1), torch.float32, 'qnan'),
                 'work': ((lib.griffinlim_fast_workspace_floats(B, F),), torch.float32, 'qnan')})
    fn = C.CDLL(lib.LIB_PATH).taco_griffinlim_fast
    fn.restype, fn.argtypes = lib.EXPORTS['taco_griffinlim_fast']
    good = dict(mag_t=lib.ptr(m), phase0=lib.ptr(p), seed=1, frames=lib.ptr(fr), per_unit=1, momentum=0.99, wave=lib.ptr(G['wave']),
                conv=lib.ptr(G['conv']), work=lib.ptr(G['work']), B=B, F=F, n_iter=n_iter)
    order = ('mag_t', 'phase0', 'seed', 'frames', 'per_unit', 'momentum', 'wave', 'conv', 'work', 'B', 'F', 'n_iter')
    cases = [('mag_t', None), ('wave', None), ('work', None), ('B', 0), ('B', -1), ('F', 4), ('F', 0), ('n_iter', -1),
             ('per_unit', 0), ('per_unit', -2), ('momentum', -0.01), ('momentum', 1.0), ('momentum', 2.0),
             ('momentum', float('nan')), ('momentum', float('inf'))]
    for key, val in cases:
        for frames in (good['frames'], None):
            a = dict(good, frames=frames)
            a[key] = val
            lib.griffinlim_fast_workspace_floats(B, F)   # (a successful call in between: the string below is this refusal's)
            torch.cuda.synchronize()
            rc = fn(*[a[k] for k in order], lib.stream_ptr())
            torch.cuda.synchronize()
            msg = lib.last_error()
            print('  %s = %r, frames %s: rc %d, %s' % (key, val, 'given' if frames else 'NULL', rc, msg))
            assert rc == -1, (key, val, rc)
            assert 'griffinlim_fast' in msg
            for name in ('wave', 'conv', 'work'):
                assert G.margin_intact(name, torch.ones(G[name].shape, dtype=torch.bool, device='cuda')), \
                    '%s was written although %s = %r is refused' % (name, key, val)
    G.check()
    for Bx, Fx in ((0, 8), (2, 4)):
        with pytest.raises(lib.TacoError):
            lib.griffinlim_fast_workspace_floats(Bx, Fx)
    # and the good arguments do run, with every nullable argument NULL in turn
    for null in ((), ('phase0',), ('frames',), ('conv',), ('phase0', 'frames', 'conv')):
        a = dict(good)
        for k in null:
            a[k] = None
        G.refill('wave', 'conv', 'work')
        assert fn(*[a[k] for k in order], lib.stream_ptr()) == 0, null
        torch.cuda.synchronize()
        G.check(*(('wave',) if 'conv' in null else ('wave', 'conv')))
        assert bool(torch.isfinite(G['wave']).all())
        if 'conv' in null:
            assert G.margin_intact('conv', torch.ones(G['conv'].shape, dtype=torch.bool, device='cuda'))


def test_graph_replay_follows_the_device_lengths(built_lib):
    """one capture on a side stream, momentum 0.99 with the readout; the replay reads `frames` at replay time"""
    mag, ph = _batch(24, (3, 4, 5))
    m, p = dev(mag), dev(ph)
    n_iter = 3
    first, second = [24, 12, 6], [9, 24, 3]
    frames = dev(first, torch.int32)
    G = Guarded({'wave': ((3, 300 * 23), torch.float32, 'qnan'), 'conv': ((3, n_iter + 1), torch.float32, 'qnan'),
                 'work': ((built_lib.griffinlim_fast_workspace_floats(3, 24),), torch.float32, 'qnan')})
    call = lambda: built_lib.griffinlim_fast(m, frames, phase0=p, n_iter=n_iter, momentum=0.99, out=G['wave'], conv=G['conv'],  # noqa: E731
                                             work=G['work'])
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
        G.refill('wave', 'conv', 'work')
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        G.check('wave', 'conv')
        got_w, got_c = G['wave'].cpu().numpy(), G['conv'].cpu().numpy()
        want_w, want_c = _fast(built_lib, m, fr, p, n_iter=n_iter, momentum=0.99)
        assert same_bits(got_w, want_w) and same_bits(got_c, want_c), 'replay with frames %s differs from the eager call' % (fr,)


RULE = dict(end_offset=200, hold=1, min_steps=5)   # target 0: every row stops after step 4 -> len_b = 8


def _raises(*a, **k):
    raise AssertionError('lib.griffinlim_fast reached without a momentum')


def test_invert_spectrogram_with_momentum(built_lib, monkeypatch):
    from tacotron_amd.config import Config
    from tacotron_amd.data import synthetic_batch
    from tacotron_amd.griffinlim import invert_spectrogram
    from tacotron_amd.model import Tacotron
    B, Td, r = 3, 16, 2
    F = (Td // 4) * 4 * r
    c = Config()
    c.r, c.vocab_size, c.max_decode_iter = r, 30, Td
    model = Tacotron(c, synthetic_batch(B, 24, Td, r, 30, seed=3, min_len=8), train=False, seed=5)
    out, _ = model.run(stop=built_lib.TacoStopRule(**RULE))
    model.check()
    torch.cuda.synchronize()
    rng = np.random.default_rng(5)
    mean = rng.standard_normal(1025 * r).astype(np.float32) * 0.1 - 2.0
    std = (0.5 + rng.random(1025 * r)).astype(np.float32)
    lengths = dev([8, 16, 4], torch.int32)
    G = Guarded({'wave': ((B, 300 * (F - 1)), torch.float32, 'qnan'),
                 'work': ((built_lib.griffinlim_fast_workspace_floats(B, F),), torch.float32, 'qnan')})
    w, conv = invert_spectrogram(out, mean, std, r, n_iter=5, seed=2, lengths=lengths, momentum=0.99, want_conv=True, wave=G['wave'],
                                 work=G['work'])
    torch.cuda.synchronize()
    G.check('wave')
    assert w is G['wave'] and conv.shape == (B, 6) and bool(torch.isfinite(conv).all()) and bool((conv > 0).all())
    w = w.cpu().numpy()
    for b, L in enumerate([8, 16, 4]):
        n = 300 * (L * r - 1)
        assert w[b, :n].any() and not bits(w[b, n:]).any()
    # the same through the binding; without lengths: device phases as well, every row over F frames
    mag_t = built_lib.denorm_unframe(out.contiguous(), dev(mean), dev(std), r, want_spec=False, want_mag_t=True)
    w2, c2 = built_lib.griffinlim_fast(mag_t, lengths, seed=2, n_iter=5, momentum=0.99, frames_per_unit=r, want_conv=True)
    assert same_bits(w2.cpu().numpy(), w) and same_bits(c2.cpu().numpy(), conv.cpu().numpy())
    w3 = invert_spectrogram(out, mean, std, r, n_iter=5, seed=2, momentum=0.99)
    assert torch.is_tensor(w3) and same_bits(w3.cpu().numpy(), built_lib.griffinlim_fast(mag_t, None, seed=2, n_iter=5).cpu().numpy())
    # momentum=None: today's two paths, which never reach the new entry point
    before = [invert_spectrogram(out, mean, std, r, n_iter=2, seed=2).cpu().numpy(),
              invert_spectrogram(out, mean, std, r, n_iter=2, seed=2, lengths=lengths).cpu().numpy()]
    monkeypatch.setattr(built_lib, 'griffinlim_fast', _raises)
    after = [invert_spectrogram(out, mean, std, r, n_iter=2, seed=2).cpu().numpy(),
             invert_spectrogram(out, mean, std, r, n_iter=2, seed=2, lengths=lengths).cpu().numpy()]
    assert same_bits(before[0], after[0]) and same_bits(before[1], after[1])
    with pytest.raises(AssertionError):
        invert_spectrogram(out, mean, std, r, n_iter=2, momentum=0.5)


def test_driver_with_momentum(built_lib, tmp_path, monkeypatch, capsys):
    """--stop --vocode-lengths --gl-momentum 0.99 --gl-iters 30 on fresh weights; without the options the files are today's"""
    from tacotron_amd import test as drv
    from tacotron_amd.config import Config
    prompts = ['hello world.\n', 'a somewhat longer prompt, with punctuation!\n', 'short\n']

    def cfg():
        c = Config()
        c.data_path = str(tmp_path / 'no_data') + '/'
        c.max_decode_iter = 16
        return c

    a = drv.parse_args(['--stop', '--vocode-lengths', '--gl-momentum', '0.99', '--gl-iters', '30'])
    rule = built_lib.TacoStopRule(**RULE)
    fast, rows, rows2 = tmp_path / 'fast', tmp_path / 'rows', tmp_path / 'rows2'
    assert drv.test(cfg(), prompts, out_dir=str(fast), n_iter=a.gl_iters, stop=rule, vocode_lengths=a.vocode_lengths,
                    gl_momentum=a.gl_momentum) == 3
    assert 'worst final spectral convergence' in capsys.readouterr().out
    assert drv.test(cfg(), prompts, out_dir=str(rows), n_iter=2, stop=rule, vocode_lengths=True) == 3
    n = 300 * (8 * cfg().r - 1)
    for i in range(3):
        conv = np.load(fast / ('prompt_%03d_conv.npy' % i))
        assert conv.shape == (31,) and conv.dtype == np.float32 and np.isfinite(conv).all() and (conv > 0).all()
        assert conv[30] < conv[0]
        for kind in ('len', 'spec', 'align'):
            name = 'prompt_%03d_%s.npy' % (i, kind)
            assert open(fast / name, 'rb').read() == open(rows / name, 'rb').read(), name
        with wavefile.open(str(fast / ('prompt_%03d.wav' % i))) as f:
            assert f.getnframes() == n
        assert not (rows / ('prompt_%03d_conv.npy' % i)).exists()
    # without the new options the driver never reaches the new entry point and writes what it wrote
    monkeypatch.setattr(built_lib, 'griffinlim_fast', _raises)
    assert drv.test(cfg(), prompts, out_dir=str(rows2), n_iter=2, stop=rule, vocode_lengths=True) == 3
    assert sorted(f.name for f in rows.iterdir()) == sorted(f.name for f in rows2.iterdir())
    for f in rows.iterdir():
        assert open(f, 'rb').read() == open(rows2 / f.name, 'rb').read(), f.name
    assert drv.test(cfg(), prompts, out_dir=str(tmp_path / 'plain'), n_iter=2) == 3
    assert not list((tmp_path / 'plain').glob('*_conv.npy'))
    with pytest.raises(AssertionError):
        drv.test(cfg(), prompts, out_dir=str(tmp_path / 'x'), n_iter=2, gl_momentum=0.5)
