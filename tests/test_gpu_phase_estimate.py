"""taco_phase_estimate on the GPU (include/taco_hip.h): initial phases read off the magnitudes, against the NumPy restatement
(tests/phase_estimate_ref.py).  Every op-level comparison is exact -- phase0 equal in its bits, compared as int32: the rules are integers
and single rounded fp32 operations, so there is no tolerance to choose.  Outputs and workspace are carved from one guarded arena
(tests/poison.py) and start as poison.  Behind the kernel: Griffin-Lim from the estimate against the fp64 restatement
(tests/fgl_ref.py) with the bars of tests/test_gpu_griffinlim_fast.py, invert_spectrogram(phase_init=...) on its three paths, and the
driver.  Magnitudes are normal fp32 numbers; no test feeds non-finite values inside a row's first F_b columns."""
import contextlib
import ctypes as C
import io
import os
import wave as wavefile

import numpy as np
import pytest
import torch

from tests import fgl_ref
from tests import phase_estimate_ref as pr
from tests.poison import Guarded

pytestmark = pytest.mark.gpu

K = pr.K
MANY = lambda ref: 0.02 * ref + 1e-3   # noqa: E731  (tests/test_gpu_griffinlim_fast.py: the bar for a many-round figure)


def ibits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(ibits(a), ibits(b))


def dev(x, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(x), dtype=dtype, device='cuda')


_CASE = {}


def case_mag(F, seed):
    """|STFT| of fgl_ref.case as fp32 (K, F), computed once per (F, seed) and never changed"""
    if (F, seed) not in _CASE:
        m = fgl_ref.case(F, seed)[0].astype(np.float32)
        m.setflags(write=False)
        _CASE[F, seed] = m
    return _CASE[F, seed]


def run(lib, mag, frames=None, per_unit=1, ws_fill='ones'):
    """one guarded call -> phase0 as a host array"""
    mag = np.array(mag, dtype=np.float32, order='C')   # (a writable copy: the shared inputs are read-only)
    B, _, F = mag.shape
    specs = {'mag': ((B, K, F), torch.float32, 'zeros'), 'phase0': ((B, K, F), torch.float32, 'qnan'),
             'ws': ((lib.phase_estimate_workspace_bytes(B, F),), torch.uint8, ws_fill)}
    if frames is not None:
        specs['frames'] = ((B,), torch.int32, 'zeros')
    G = Guarded(specs)
    G['mag'].copy_(torch.from_numpy(mag))
    if frames is not None:
        G['frames'].copy_(torch.as_tensor(np.asarray(frames, dtype=np.int32)))
    out = lib.phase_estimate(G['mag'], G['frames'] if frames is not None else None, per_unit, out=G['phase0'], workspace=G['ws'])
    torch.cuda.synchronize()
    assert out is G['phase0']
    G.check('phase0')
    assert np.array_equal(G['mag'].cpu().numpy().view(np.int32), mag.view(np.int32)), 'mag_t was written'
    if frames is not None:
        assert np.array_equal(G['frames'].cpu().numpy(), np.asarray(frames, dtype=np.int32))
    return out.cpu().numpy()


def check(lib, mag, frames=None, per_unit=1, label=''):
    with np.errstate(invalid='ignore'):
        want = pr.phase_estimate(mag, frames, per_unit)
    got = run(lib, mag, frames, per_unit)
    bad = np.argwhere(ibits(got) != ibits(want))
    assert bad.size == 0, '%s: %d of %d elements differ from the restatement, first at (b, bin, frame) = %s: %r against %r' % (
        label, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])
    return got


# F walks 1, the edges of the 16-frame tile of both launches (15, 16, 17, 31, 32, 33, 48, 64, 65), the four frames a thread of the
# chain keeps in flight (3, 4, 5) and a last tile that is neither full nor a single frame (96 = 6 tiles, 41).
@pytest.mark.parametrize('F', [1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 48, 64, 65, 96])
def test_frames_one_row(built_lib, F):
    mag = case_mag(96, 3)[None, :, :F]
    check(built_lib, mag, None, label='F=%d' % F)


@pytest.mark.parametrize('per_unit,frames', [(1, [41, 7, 0]), (2, [20, 4, 0]), (2, [21, 3, -5]), (1, [2 ** 30, 16, 17])])
def test_rows_with_their_own_lengths(built_lib, per_unit, frames):
    """frames inside, at 0, below 0 and beyond F; NaN behind every row's F_b; and the per-row contract"""
    lib = built_lib
    F = 41
    mag = np.stack([case_mag(F, s) for s in (3, 4, 5)]) * np.array([1.0, 0.5, 2.0], dtype=np.float32)[:, None, None]
    Fb = [max(0, min(F, f * per_unit)) for f in frames]
    dirty = mag.copy()
    for b in range(3):
        dirty[b, :, Fb[b]:] = np.nan
    got = check(lib, dirty, frames, per_unit, label='frames %s x %d' % (frames, per_unit))
    for b in range(3):
        assert np.array_equal(ibits(got[b, :, Fb[b]:]), np.zeros((K, F - Fb[b]), dtype=np.int32)), 'row %d: not +0 behind F_b' % b
        if Fb[b] > 0:
            alone = run(lib, np.ascontiguousarray(mag[b:b + 1, :, :Fb[b]]))
            assert same_bits(alone[0], got[b, :, :Fb[b]]), 'row %d differs from the B = 1, F = F_b call on its own columns' % b


def test_frames_null_is_all_frames(built_lib):
    mag = np.stack([case_mag(41, 3), case_mag(41, 4)])
    got = check(built_lib, mag, None, label='frames NULL')
    assert same_bits(got, run(built_lib, mag, [41, 41]))


def test_edge_frames(built_lib):
    """the edge frames of tests/phase_estimate_ref.py spliced into ordinary rows, every one between voiced frames"""
    edges = pr.edge_frames()
    names = sorted(edges)
    F = 3 * len(names) + 2
    rows = [pr.splice(case_mag(96, 3)[:, :F], {2 + 3 * i: edges[n] for i, n in enumerate(names)}),
            pr.splice(case_mag(96, 3)[:, :F], {1 + 2 * i: edges[n] for i, n in enumerate(reversed(names))}),
            np.stack([edges[n] for n in names] * 2, axis=1)[:, :F]]   # ... and back to back, the first frame of the row an edge
    rows[2] = np.concatenate([rows[2], np.tile(edges['all_zero'][:, None], (1, F - rows[2].shape[1]))], axis=1)
    mag = np.stack(rows).astype(np.float32)
    assert np.isfinite(mag).all() and ((mag == 0) | (np.abs(mag) >= np.finfo(np.float32).tiny)).all()
    got = check(built_lib, mag, None, label='edge frames')
    # what the edges are there for, read off the device's result
    rising = run(built_lib, np.stack([edges['falling'], edges['rising'], edges['all_zero']], axis=1)[None])[0]
    assert same_bits(rising[:, 1], rising[:, 0]) and same_bits(rising[:, 2], rising[:, 0]), 'a frame without owners moved a phase'
    assert np.array_equal(ibits(rising[:, 0]), ibits(pr.phase_of(np.zeros(K, dtype=np.uint32))))
    assert got.shape == mag.shape


@pytest.mark.parametrize('fill', ['ones', 'qnan', 'noise', 'zeros'])
def test_result_does_not_depend_on_the_workspace(built_lib, fill):
    mag = np.stack([case_mag(41, 3), case_mag(41, 4)])
    frames = [41, 18]
    want = pr.phase_estimate(mag, frames)
    assert same_bits(run(built_lib, mag, frames, ws_fill=fill), want)


def test_two_calls_give_the_same_bits(built_lib):
    mag = np.stack([case_mag(96, 3), case_mag(96, 4)])
    m = dev(mag)
    a, b = built_lib.phase_estimate(m), built_lib.phase_estimate(m)
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert float(a.min()) >= 0.0 and float(a.max()) < 2.0 * np.pi + 1e-6


def test_bad_arguments_enqueue_nothing(built_lib):
    """every TACO_EINVAL case returns before a launch: phase0 and workspace keep their fill; the error string is set"""
    lib = built_lib
    B, F = 2, 8
    m, fr = dev(np.stack([case_mag(41, 3)[:, :F]] * B)), dev([8, 6], torch.int32)
    G = Guarded({'phase0': ((B, K, F), torch.float32, 'qnan'), 'ws': ((lib.phase_estimate_workspace_bytes(B, F),), torch.uint8, 'ones')})
    fn = C.CDLL(lib.LIB_PATH).taco_phase_estimate
    fn.restype, fn.argtypes = lib.EXPORTS['taco_phase_estimate']
    good = dict(mag_t=lib.ptr(m), frames=lib.ptr(fr), per_unit=1, phase0=lib.ptr(G['phase0']), ws=lib.ptr(G['ws']), B=B, F=F)
    order = ('mag_t', 'frames', 'per_unit', 'phase0', 'ws', 'B', 'F')
    cases = [('mag_t', None), ('phase0', None), ('ws', None), ('B', 0), ('B', -1), ('F', 0), ('F', -3), ('per_unit', 0), ('per_unit', -2),
             ('mag_t', good['phase0'])]
    for key, val in cases:
        for frames in (good['frames'], None):
            a = dict(good, frames=frames)
            a[key] = val
            lib.phase_estimate_workspace_bytes(B, F)
            torch.cuda.synchronize()
            rc = fn(*[a[k] for k in order], lib.stream_ptr())
            torch.cuda.synchronize()
            msg = lib.last_error()
            assert rc == -1, (key, val, rc)
            assert 'phase_estimate' in msg
            for name in ('phase0', 'ws'):
                assert G.margin_intact(name, torch.ones(G[name].shape, dtype=torch.bool, device='cuda')), \
                    '%s was written although %s = %r is refused' % (name, key, val)
    G.check()
    for Bx, Fx in ((0, 8), (2, 0), (-1, 8)):
        assert C.CDLL(lib.LIB_PATH).taco_phase_estimate_workspace_bytes(Bx, Fx) < 0
        with pytest.raises(ValueError):
            lib.phase_estimate_workspace_bytes(Bx, Fx)
    with pytest.raises(ValueError):
        lib.phase_estimate(m, out=m)
    with pytest.raises(ValueError):
        lib.phase_estimate(m, fr, 0)
    with pytest.raises(ValueError):
        lib.phase_estimate(m, fr.to(torch.int64))
    with pytest.raises(ValueError):
        lib.phase_estimate(m[:, :1000].contiguous())
    with pytest.raises(ValueError):
        lib.phase_estimate(m, workspace=torch.empty(16, dtype=torch.uint8, device='cuda'))
    assert fn(*[good[k] for k in order], lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    G.check('phase0')


def test_graph_replay_follows_the_device_lengths(built_lib):
    """one capture on one side stream, no parallel branches; the replay reads `frames` at replay time"""
    lib = built_lib
    mag = np.stack([case_mag(41, s) for s in (3, 4, 5)])
    m = dev(mag)
    first, second = [41, 12, 6], [9, 41, 0]
    frames = dev(first, torch.int32)
    G = Guarded({'phase0': ((3, K, 41), torch.float32, 'qnan'), 'ws': ((lib.phase_estimate_workspace_bytes(3, 41),), torch.uint8, 'ones')})
    call = lambda: lib.phase_estimate(m, frames, out=G['phase0'], workspace=G['ws'])   # noqa: E731
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
        G.refill('phase0', 'ws')
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        G.check('phase0')
        assert same_bits(G['phase0'].cpu().numpy(), pr.phase_estimate(mag, fr)), 'replay with frames %s' % (fr,)


def test_griffinlim_from_the_estimate(built_lib):
    """lib.griffinlim_fast from lib.phase_estimate, 10 rounds at momentum 0.99, B = 3: the readout against the fp64 restatement fed
    the restatement's phases (the bars of tests/test_gpu_griffinlim_fast.py), and against the same call from device seed phases"""
    lib = built_lib
    F = 96
    inputs = [fgl_ref.fp32_inputs(fgl_ref.speechy, 96, 1)[0], fgl_ref.fp32_inputs(fgl_ref.speechy, 96, 2)[0],
              fgl_ref.fp32_inputs(fgl_ref.case, 41, 3)[0]]
    frames = [96, 96, 41]
    mag = np.full((3, K, F), np.nan, dtype=np.float32)
    for b, x in enumerate(inputs):
        mag[b, :, :x.shape[1]] = x
    m, fr = dev(mag), dev(frames, torch.int32)
    est = lib.phase_estimate(m, fr)
    _, conv = lib.griffinlim_fast(m, fr, phase0=est, n_iter=10, momentum=0.99, want_conv=True)
    _, seeded = lib.griffinlim_fast(m, fr, phase0=None, seed=5, n_iter=10, momentum=0.99, want_conv=True)
    torch.cuda.synchronize()
    conv, seeded, est = conv.cpu().numpy(), seeded.cpu().numpy(), est.cpu().numpy()
    for b, x in enumerate(inputs):
        ph = pr.phase_estimate_row(x)
        assert same_bits(est[b, :, :frames[b]], ph)
        _, ref = fgl_ref.griffinlim_fast(x.astype(np.float64), ph.astype(np.float64), 10, 0.99)
        print('  row %d: conv[0] device %.6f restatement %.6f, seeded %.6f; conv[10] device %.6f restatement %.6f, seeded %.6f; rounds '
              '1..9 worst |d| / bar %.3f' % (b, conv[b, 0], ref[0], seeded[b, 0], conv[b, 10], ref[10], seeded[b, 10],
                                             float(np.max(np.abs(conv[b, 1:10] - ref[1:10]) / MANY(ref[1:10])))))
        assert abs(float(conv[b, 0]) - ref[0]) <= 4e-5
        assert (np.abs(conv[b, 1:10] - ref[1:10]) <= MANY(ref[1:10])).all()
        assert abs(float(conv[b, 10]) - ref[10]) <= MANY(ref[10])
        assert conv[b, 0] <= 0.5 * seeded[b, 0]
        assert conv[b, 10] < seeded[b, 10]


# ---- invert_spectrogram ---------------------------------------------------------------------------------------------------------------
def _model_output(B=2, Td=8, r=2, seed=0):
    """(out (B, Td, 1025 r) normalised log-magnitudes on the device, mean, std): smooth enough to have lobes, not a trained model's"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, Td, K * r)).astype(np.float32)
    x = (x + np.roll(x, 1, axis=2) + np.roll(x, 2, axis=2)) * 0.5
    return dev(x), np.zeros(K * r, dtype=np.float32), np.ones(K * r, dtype=np.float32)


@pytest.mark.parametrize('path', ['plain', 'lengths', 'rate', 'momentum', 'rate+momentum'])
def test_invert_spectrogram_estimate_is_phase0_handed_in(built_lib, monkeypatch, path):
    from tacotron_amd import griffinlim as glm
    lib = built_lib
    out, mean, std = _model_output()
    lengths = dev([8, 3], torch.int32)
    kw = dict(n_iter=2, seed=4)
    if path in ('lengths', 'rate', 'rate+momentum'):
        kw['lengths'] = lengths
    if 'rate' in path:
        kw['rate'] = [0.8, 1.25]
    if 'momentum' in path:
        kw.update(momentum=0.99, want_conv=True)
    seen = []
    real = lib.phase_estimate

    def spy(mag_t, frames=None, frames_per_unit=1, **more):
        ph = real(mag_t, frames, frames_per_unit, **more)
        seen.append((mag_t.cpu().numpy(), None if frames is None else frames.cpu().numpy(), frames_per_unit, ph))
        return ph

    monkeypatch.setattr(lib, 'phase_estimate', spy)
    got = glm.invert_spectrogram(out, mean, std, 2, phase_init='estimate', **kw)
    torch.cuda.synchronize()
    assert len(seen) == 1
    mag, frames, per_unit, ph = seen[0]
    assert (frames is None) == (path in ('plain', 'momentum')) and per_unit == (2 if path == 'lengths' else 1)
    with np.errstate(invalid='ignore'):
        assert same_bits(ph.cpu().numpy(), pr.phase_estimate(mag, frames, per_unit)), 'not the estimate of the magnitudes the vocoder got'
    want = glm.invert_spectrogram(out, mean, std, 2, phase0=ph, **kw)
    torch.cuda.synchronize()
    assert len(seen) == 1, 'phase0 given: nothing is estimated'
    got, want = (got if isinstance(got, tuple) else (got,)), (want if isinstance(want, tuple) else (want,))
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.dtype == w.dtype and torch.equal(g.view(torch.int32), w.view(torch.int32))
    rand = glm.invert_spectrogram(out, mean, std, 2, **kw)
    rand = rand if isinstance(rand, tuple) else (rand,)
    assert [tuple(t.shape) for t in rand] == [tuple(t.shape) for t in got], 'return shapes changed'
    assert not torch.equal(rand[0], got[0])
    with pytest.raises(ValueError):
        glm.invert_spectrogram(out, mean, std, 2, phase_init='estimate', phase0=ph, **kw)


@pytest.mark.parametrize('path', ['plain', 'lengths', 'rate', 'momentum'])
def test_invert_spectrogram_random_is_unchanged(built_lib, monkeypatch, path):
    """None and 'random' are the call without the keyword, bit for bit, and never reach the estimate"""
    from tacotron_amd import griffinlim as glm
    out, mean, std = _model_output(seed=1)
    kw = dict(n_iter=2, seed=9)
    if path in ('lengths', 'rate'):
        kw['lengths'] = dev([8, 3], torch.int32)
    if path == 'rate':
        kw['rate'] = 0.8
    if path == 'momentum':
        kw['momentum'] = 0.99

    def never(*a, **k):
        raise AssertionError('lib.phase_estimate reached without phase_init=\'estimate\'')

    monkeypatch.setattr(built_lib, 'phase_estimate', never)
    base = glm.invert_spectrogram(out, mean, std, 2, **kw)
    for init in (None, 'random'):
        got = glm.invert_spectrogram(out, mean, std, 2, phase_init=init, **kw)
        for g, w in zip(got if isinstance(got, tuple) else (got,), base if isinstance(base, tuple) else (base,)):
            assert torch.equal(g.view(torch.int32), w.view(torch.int32)), 'phase_init=%r changed the %s path' % (init, path)


# ---- the driver -----------------------------------------------------------------------------------------------------------------------
PROMPTS = ['hello world.\n', 'a somewhat longer prompt, with punctuation!\n']


def _cfg(tmp_path):
    from tacotron_amd.config import Config
    c = Config()
    c.data_path = str(tmp_path / 'no_data') + '/'
    c.max_decode_iter = 16
    return c


def _wav(path):
    with wavefile.open(str(path), 'rb') as f:
        assert f.getframerate() == 16000 and f.getnchannels() == 1 and f.getsampwidth() == 2
        return np.frombuffer(f.readframes(f.getnframes()), dtype='<i2')


def test_driver_draft_voice_and_unchanged_default(built_lib, tmp_path, monkeypatch):
    """test(gl_init='estimate', n_iter=0) writes wav files of the expected lengths; the default call hands phase_init=None on and its
    files are those of invert_spectrogram without the keyword at the same seed"""
    from tacotron_amd import griffinlim as glm
    from tacotron_amd import test as drv
    calls = []
    real = drv.vocode

    def spy(*a, **k):
        res = real(*a, **k)
        calls.append((a, dict(k), res.waveform))
        return res

    monkeypatch.setattr(drv, 'vocode', spy)
    with contextlib.redirect_stdout(io.StringIO()):
        assert drv.test(_cfg(tmp_path), PROMPTS, out_dir=str(tmp_path / 'plain'), n_iter=2) == 2
        assert drv.test(_cfg(tmp_path), PROMPTS, out_dir=str(tmp_path / 'random'), n_iter=2, gl_init='random') == 2
        assert drv.test(_cfg(tmp_path), PROMPTS, out_dir=str(tmp_path / 'draft'), n_iter=0, gl_init='estimate') == 2
    assert [k['phase_init'] for _, k, _ in calls] == [None, None, 'estimate']
    assert _cfg(tmp_path).r == 2
    samples = 300 * (16 * 2 - 1)
    a, k, res = calls[0]
    k = {name: v for name, v in k.items() if name != 'phase_init'}
    before = glm.invert_spectrogram(*a, **k)   # (the call as it was written before there was a phase_init)
    torch.cuda.synchronize()
    assert torch.equal(before.view(torch.int32), res.view(torch.int32))
    for i in range(2):
        drv.write_wav(str(tmp_path / 'expect.wav'), before[i].cpu().numpy())
        want = open(tmp_path / 'expect.wav', 'rb').read()
        for sub in ('plain', 'random'):
            assert open(tmp_path / sub / ('prompt_%03d.wav' % i), 'rb').read() == want, '%s prompt %d' % (sub, i)
        draft = _wav(tmp_path / 'draft' / ('prompt_%03d.wav' % i))
        assert draft.shape == (samples,) and _wav(tmp_path / 'plain' / ('prompt_%03d.wav' % i)).shape == (samples,)
        assert np.abs(draft.astype(np.int32)).max() > 0
    names = sorted(os.listdir(tmp_path / 'plain'))
    assert sorted(os.listdir(tmp_path / 'draft')) == names
    for name in names:
        if not name.endswith('.wav'):
            assert open(tmp_path / 'draft' / name, 'rb').read() == open(tmp_path / 'plain' / name, 'rb').read(), name


def test_driver_estimate_with_lengths_and_momentum(built_lib, tmp_path, capsys):
    """--stop --vocode-lengths --gl-init estimate --gl-momentum 0.99 --gl-iters 10: the convergence line is printed as it is"""
    from tacotron_amd import test as drv
    lib = built_lib
    rule = lib.TacoStopRule(end_offset=200, hold=1, min_steps=5)   # target 0: every row stops after step 4 -> len_b = 8
    assert drv.test(_cfg(tmp_path), PROMPTS, out_dir=str(tmp_path / 'fast'), n_iter=10, stop=rule, vocode_lengths=True, gl_momentum=0.99,
                    gl_init='estimate') == 2
    out = capsys.readouterr().out
    assert 'Griffin-Lim momentum 0.99, 10 rounds: worst final spectral convergence of the batch' in out
    for i in range(2):
        assert _wav(tmp_path / 'fast' / ('prompt_%03d.wav' % i)).shape == (300 * (8 * 2 - 1),)
        assert np.load(tmp_path / 'fast' / ('prompt_%03d_conv.npy' % i)).shape == (11,)
