"""GPU: taco_wave_finish (include/taco_hip.h) through the C ABI -- de-emphasis against its derived first-order bound, the energy
trim against the fp64 restatement (tests/wave_ref.py) on inputs whose decision margin the test asserts first, the exact peak, PCM16
bit for bit against the entry point's fp32 rule and within 1 LSB of write_wav's float64 rule, the per-row contract, determinism,
poisoned buffers between guard bands, every TACO_EINVAL case, and the driver's --deemphasis / --trim-db.
"""
import ctypes as C
import wave as wavefile

import numpy as np
import pytest
import torch

from tests import audio_ref, wave_ref as wr
from tests.poison import Guarded

pytestmark = pytest.mark.gpu

L_FULL = wr.L_FULL


def dev(x, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(x), dtype=dtype, device='cuda')


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({2: np.uint16, 4: np.uint32}[x.dtype.itemsize])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def _finish(lib, x, samples=None, a=0.97, db=0.0, want_out=True, want_pcm=True, fill='qnan'):
    """lib.wave_finish into poisoned buffers between guard bands (the workspace poisoned as well); every element of every output
    must have been written.  -> (out, pcm, bounds, peak) as NumPy arrays (None for an output not asked for)"""
    xt = x if torch.is_tensor(x) else dev(x)
    B, L = xt.shape
    spec = {'bounds': ((B, 2), torch.int32, fill), 'peak': ((B,), torch.float32, fill),
            'work': ((lib.wave_finish_workspace_floats(B, L),), torch.float32, fill)}
    if want_out:
        spec['out'] = ((B, L), torch.float32, fill)
    if want_pcm:
        spec['pcm'] = ((B, L), torch.int16, fill)
    G = Guarded(spec)
    st = samples if samples is None or torch.is_tensor(samples) else dev(samples, torch.int32)
    r = lib.wave_finish(xt, st, deemphasis=a, trim_top_db=db, want_out=want_out, want_pcm=want_pcm, out=G['out'] if want_out else None,
                        pcm=G['pcm'] if want_pcm else None, bounds=G['bounds'], peak=G['peak'], work=G['work'])
    torch.cuda.synchronize()
    assert r[2] is G['bounds'] and r[3] is G['peak'] and (r[0] is None) == (not want_out) and (r[1] is None) == (not want_pcm)
    # (0 is a legal sample and the fill of the clean run; every int16 value is a legal PCM sample, so that `pcm` is written
    # everywhere is shown by test_same_arguments_same_bits_and_poison_changes_nothing: all-zero and all-ones fills end in the same bits)
    G.check(*[k for k in ('out', 'bounds', 'peak') if k in spec and fill != 'zeros'])
    return tuple(None if t is None else t.cpu().numpy() for t in r)


# ---- de-emphasis -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('a', [0.97, 0.5, 0.999])
def test_deemphasis_within_the_derived_bound(built_lib, a):
    """|y32 - y64| <= E = 2^-24 (16 S + 2 T) + 1e-30 per sample on the four families, and the front end's pre-emphasis of `out`
    returns x within E[n] + a E[n-1] + 4 * 2^-24 (|y[n]| + |y[n-1]|)"""
    x = np.stack([wr.family(f) for f in wr.FAMILIES])
    out, _, bounds, peak = _finish(built_lib, x, a=a, want_pcm=False)
    a32 = wr.coeff(a)
    worst = 0.0
    for i, f in enumerate(wr.FAMILIES):
        y64 = wr.deemphasis(x[i], a)
        E = wr.error_bound(x[i], a)
        err = np.abs(out[i].astype(np.float64) - y64)
        ratio = float((err / E).max())
        back = np.abs(wr.preemphasis(out[i], a) - x[i].astype(np.float64))
        ay = np.abs(y64)
        Eb = E + a32 * np.append(0.0, E[:-1]) + 4 * wr.U * (ay + np.append(0.0, ay[:-1]))
        rb = float((back / Eb).max())
        print('  a = %g, %-9s: worst err / E = %.4f at sample %d (|y| max %.3g); round trip / its bound = %.4f'
              % (a, f, ratio, int((err / E).argmax()), ay.max(), rb))
        worst = max(worst, ratio)
        assert (err <= E).all(), (f, ratio)
        assert (back <= Eb).all(), (f, rb)
        assert tuple(bounds[i]) == (0, L_FULL) and peak[i] == np.abs(out[i]).max()
    print('  a = %g: worst err / E of the four families %.4f' % (a, worst))


def test_deemphasis_0_is_the_input_bit_for_bit(built_lib):
    rng = np.random.default_rng(3)
    L = 10000
    x = rng.standard_normal((3, L)).astype(np.float32)
    x[0, :8] = [-0.0, 0.0, -0.0, 1e-40, -1e-40, 3e38, -3e38, -0.0]   # signed zeros, denormals, large values
    n = [L, 4097, 0]
    xin = x.copy()
    for b in range(3):
        xin[b, n[b]:] = np.nan
    out, pcm, bounds, peak = _finish(built_lib, xin, n, a=0.0)
    for b in range(3):
        assert same_bits(out[b, :n[b]], x[b, :n[b]]), b
        assert not bits(out[b, n[b]:]).any() and not pcm[b, n[b]:].any()
        assert tuple(bounds[b]) == (0, n[b])
        assert peak[b] == (np.abs(x[b, :n[b]]).max() if n[b] else 0.0)


# ---- trim -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('L,where,floor,dbs', wr.TRIM_CASES, ids=['L%d' % c[0] for c in wr.TRIM_CASES])
def test_trim_bounds_equal_the_fp64_restatement(built_lib, L, where, floor, dbs):
    """precondition, asserted: no frame of the restatement lies within 1 dB of the threshold; then the bounds are EQUAL"""
    x = wr.burst(L, where[0], where[1], floor)
    y64 = wr.deemphasis(x, 0.97)
    assert wr.trim_bounds(y64, 60.0) == audio_ref.trim_bounds(y64)   # the restatement at 60 dB is the front end's trim
    for db in dbs:
        margin = wr.trim_margin(y64, db)
        s, e = wr.trim_bounds(y64, db)
        assert margin >= 1.0, 'the input does not satisfy the precondition: a frame lies %.2f dB from -%g dB' % (margin, db)
        out, pcm, bounds, peak = _finish(built_lib, x[None], a=0.97, db=db)
        print('  L = %d, top_db %g: margin %.1f dB, fp64 bounds (%d, %d), device %s, peak %.4f' % (L, db, margin, s, e, tuple(int(v) for v in bounds[0]), peak[0]))
        assert tuple(bounds[0]) == (s, e)
        assert 0 < s and e - s < L and peak[0] > 1.0                   # (it does trim, and the row takes the peak > 1 branch)
        assert peak[0] == np.abs(out[0]).max()                         # exact
        assert abs(peak[0] - np.abs(y64[s:e]).max()) <= wr.error_bound(x, 0.97).max()
        assert (np.abs(out[0, :e - s] - y64[s:e]) <= wr.error_bound(x, 0.97)[s:e]).all()
        assert not bits(out[0, e - s:]).any() and not pcm[0, e - s:].any()
        assert same_bits(pcm[0], wr.pcm_fp32(out[0], peak[0]))


def test_trim_edge_rows(built_lib):
    """no trim at top_db 0; an all-zero row is not trimmed; n_b in {0, 1, 511, 512, 2047} against the restatement"""
    rng = np.random.default_rng(5)
    L = 2047
    ns = [0, 1, 511, 512, 2047, 2047]
    x = (0.1 * rng.standard_normal((len(ns), L))).astype(np.float32)
    x[5] = 0.0   # the all-zero row
    xin = x.copy()
    for b, n in enumerate(ns):
        xin[b, n:] = np.nan
    for db in (0.0, 40.0):
        out, pcm, bounds, peak = _finish(built_lib, xin, ns, a=0.97, db=db)
        for b, n in enumerate(ns):
            y64, (s, e), pk = wr.finish(x[b, :n], 0.97, db)
            if db > 0 and n > 0 and x[b, :n].any():
                assert wr.trim_margin(y64, db) >= 1.0
            assert tuple(bounds[b]) == (s, e) == (0, n), (db, b, tuple(bounds[b]), (s, e))
            assert peak[b] == (np.abs(out[b, :n]).max() if n else 0.0)
            assert abs(peak[b] - pk) <= 1e-5
            assert (np.abs(out[b, :n] - y64) <= wr.error_bound(x[b, :n], 0.97)).all()
            assert not bits(out[b, n:]).any() and not pcm[b, n:].any()
    # a burst with the trim switched off keeps every sample
    Lc, where, floor, _ = wr.TRIM_CASES[2]
    xb = wr.burst(Lc, where[0], where[1], floor)
    _, _, bounds, _ = _finish(built_lib, xb[None], a=0.97, db=0.0)
    assert tuple(bounds[0]) == (0, Lc)


def test_front_end_and_finishing_cut_the_same_samples(built_lib):
    """the -60 dB bounds of taco_audio_features equal the bounds of taco_wave_finish at trim_top_db 60 on the same rows, exactly:
    both kernels state csrc/stft.h's trim rule.  Three rows of different lengths, 1e-5 noise around a 0.5-amplitude tone whose
    edges lie at least 64 samples from every trim frame's edge (no frame is near the threshold: -16 dB or above against -91 dB)"""
    from tacotron_amd import audio
    L, lengths, body = 6000, [6000, 4097, 1537], [(2200, 4300), (1600, 2300), (1200, 1400)]
    rng = np.random.default_rng(17)
    x = np.zeros((3, L), np.float32)
    for b, (n, (s, e)) in enumerate(zip(lengths, body)):
        x[b, :n] = 1e-5 * rng.standard_normal(n)
        x[b, s:e] += 0.5 * np.sin(2 * np.pi * 180 * np.arange(s, e) / 16000.0)
    wave = dev(x)
    front = built_lib.audio_features(wave, lengths, dev(audio.mel_basis()), 1, max_len=L)[3]
    finish = built_lib.wave_finish(wave, samples=dev(lengths, torch.int32), deemphasis=0.0, trim_top_db=60.0)[2]
    torch.cuda.synchronize()
    front, finish = front.cpu().numpy(), finish.cpu().numpy()
    print('  front end %s, finishing %s' % (front.tolist(), finish.tolist()))
    assert np.array_equal(front, finish)
    # the bounds by hand: frame t covers [512 t - 1024, 512 t + 1024) of the reflect-padded row and passes when it holds tone
    assert finish.tolist() == [[1536, 5632], [1024, 3584], [512, 1537]]


# ---- rows, determinism, poison ------------------------------------------------------------------------------------------------
ROWS_N = [L_FULL, 0, 1, 59700, 12345]


def _rows_input():
    L = L_FULL
    x = np.stack([wr.burst(L, 20011, 70003, 1e-5), wr.family('noise'), wr.family('bursts'), wr.burst(L, 8000, 59700, 3e-6),
                  wr.family('same_sign')])
    xin = x.copy()
    for b, n in enumerate(ROWS_N):
        xin[b, n:] = np.nan
    return x, xin


@pytest.mark.parametrize('db', [0.0, 40.0])
def test_rows_are_the_call_on_each_row_alone(built_lib, db):
    """B = 5, L = 107,700, samples = [L, 0, 1, 59700, 12345], NaN behind each n_b: row b is bit-identical to its own B = 1,
    L = n_b call on a contiguous copy, for out, pcm, bounds and peak"""
    x, xin = _rows_input()
    out, pcm, bounds, peak = _finish(built_lib, xin, ROWS_N, a=0.97, db=db)
    assert np.isfinite(out).all() and np.isfinite(peak).all()
    for b, n in enumerate(ROWS_N):
        if n == 0:
            assert tuple(bounds[b]) == (0, 0) and peak[b] == 0 and not bits(out[b]).any() and not pcm[b].any()
            continue
        o1, p1, b1, k1 = _finish(built_lib, np.ascontiguousarray(x[b:b + 1, :n]), None, a=0.97, db=db)
        assert tuple(bounds[b]) == tuple(b1[0]), (b, bounds[b], b1[0])
        assert same_bits(peak[b:b + 1], k1)
        assert same_bits(out[b, :n], o1[0]) and same_bits(pcm[b, :n], p1[0]), b
        assert not bits(out[b, n:]).any() and not pcm[b, n:].any()
        assert peak[b] == np.abs(out[b]).max()


def test_same_arguments_same_bits_and_poison_changes_nothing(built_lib):
    """two calls give the same bits; a NaN / all-ones / noise workspace and output fill give the bits of the zero-filled call"""
    x, xin = _rows_input()
    ref = _finish(built_lib, xin, ROWS_N, a=0.97, db=40.0, fill='zeros')
    for fill in ('zeros', 'qnan', 'ones', 'noise'):
        got = _finish(built_lib, xin, ROWS_N, a=0.97, db=40.0, fill=fill)
        for name, r, g in zip(('out', 'pcm', 'bounds', 'peak'), ref, got):
            assert r.dtype == g.dtype and np.array_equal(r.view(np.uint8), g.view(np.uint8)), (fill, name)
    # one output at a time
    o_only = _finish(built_lib, xin, ROWS_N, a=0.97, db=40.0, want_pcm=False)
    p_only = _finish(built_lib, xin, ROWS_N, a=0.97, db=40.0, want_out=False)
    assert same_bits(o_only[0], ref[0]) and same_bits(p_only[1], ref[1])
    for r in (o_only, p_only):
        assert np.array_equal(r[2], ref[2]) and same_bits(r[3], ref[3])


# ---- PCM ------------------------------------------------------------------------------------------------------------------------
def test_pcm_rule(built_lib):
    """bit-exact against the NumPy-fp32 restatement of step 4 on the device's own out and peak; within 1 LSB of write_wav's float64
    rule on the same samples; one row unscaled (peak <= 1), one scaled (peak > 1)"""
    L = 30000
    quiet = (0.02 * np.random.default_rng(9).standard_normal(L)).astype(np.float32)
    loud = wr.burst(L, 3000, 25000, 1e-5)
    x = np.stack([quiet, loud])
    out, pcm, bounds, peak = _finish(built_lib, x, a=0.97, db=0.0)
    assert peak[0] <= 1.0 < peak[1], peak
    for b in range(2):
        assert peak[b] == np.abs(out[b]).max()
        assert same_bits(pcm[b], wr.pcm_fp32(out[b], peak[b])), b
        d = np.abs(pcm[b].astype(np.int32) - wr.pcm_write_wav(out[b]).astype(np.int32))
        print('  row %d: peak %.4f, PCM16 differs from write_wav\'s float64 rule in %d of %d samples, by at most %d' % (b, peak[b], int((d > 0).sum()), L, d.max()))
        assert d.max() <= 1
        assert np.abs(pcm[b].astype(np.int32)).max() <= 32767
    assert np.abs(pcm[1].astype(np.int32)).max() == 32767   # the scaled row's peak sample is full scale


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_bad_arguments_enqueue_nothing(built_lib):
    """every TACO_EINVAL case returns before a launch: the outputs and the workspace keep their sentinel; the error string is set"""
    lib = built_lib
    B, L = 2, 5000
    x = dev(np.stack([wr.burst(L, 1200, 3100, 1e-5), wr.family('noise', L)]))
    sm = dev([L, 3000], torch.int32)
    G = Guarded({'out': ((B, L), torch.float32, 7.0), 'pcm': ((B, L), torch.int16, 7.0), 'bounds': ((B, 2), torch.int32, 7.0),
                 'peak': ((B,), torch.float32, 7.0), 'work': ((lib.wave_finish_workspace_floats(B, L),), torch.float32, 7.0)})
    fn = C.CDLL(lib.LIB_PATH).taco_wave_finish
    fn.restype, fn.argtypes = lib.EXPORTS['taco_wave_finish']
    good = dict(wave=lib.ptr(x), samples=lib.ptr(sm), a=0.97, db=40.0, out=lib.ptr(G['out']), pcm=lib.ptr(G['pcm']),
                bounds=lib.ptr(G['bounds']), peak=lib.ptr(G['peak']), work=lib.ptr(G['work']), B=B, L=L)
    order = ('wave', 'samples', 'a', 'db', 'out', 'pcm', 'bounds', 'peak', 'work', 'B', 'L')
    cases = [{'wave': None}, {'bounds': None}, {'peak': None}, {'work': None}, {'out': None, 'pcm': None}, {'out': good['wave']},
             {'B': 0}, {'B': -1}, {'L': 0}, {'L': -5}, {'a': -0.01}, {'a': 1.0}, {'a': 1.5}, {'a': float('nan')}, {'a': float('inf')},
             {'db': -1.0}, {'db': float('nan')}, {'db': float('-inf')}]
    everything = {k: torch.ones(G[k].shape, dtype=torch.bool, device='cuda') for k in ('out', 'pcm', 'bounds', 'peak', 'work')}
    for change in cases:
        for samples in (good['samples'], None):
            a = dict(good, samples=samples)
            a.update(change)
            lib.wave_finish_workspace_floats(B, L)   # (a successful call in between: the string below is this refusal's)
            rc = fn(*[a[k] for k in order], lib.stream_ptr())
            torch.cuda.synchronize()
            msg = lib.last_error()
            print('  %r, samples %s: rc %d, %s' % (change, 'given' if samples else 'NULL', rc, msg))
            assert rc == -1, (change, rc)
            assert 'wave_finish' in msg
            for name, m in everything.items():
                assert G.margin_intact(name, m), '%s was written although %r is refused' % (name, change)
    G.check()
    for Bx, Lx in ((0, 100), (-1, 100), (2, 0), (2, -3)):
        with pytest.raises(lib.TacoError):
            lib.wave_finish_workspace_floats(Bx, Lx)
    # and the good arguments do run, with every nullable argument NULL in turn
    for null in ((), ('samples',), ('out',), ('pcm',), ('samples', 'pcm')):
        a = dict(good)
        for k in null:
            a[k] = None
        G.refill('out', 'pcm', 'bounds', 'peak', 'work')
        assert fn(*[a[k] for k in order], lib.stream_ptr()) == 0, null
        torch.cuda.synchronize()
        G.check()
        for k in ('out', 'pcm'):
            if k in null:
                assert G.margin_intact(k, everything[k])
            else:
                assert not bool(torch.isnan(G[k].float()).any()) and not G.margin_intact(k, everything[k])
        e = G['bounds'].cpu().numpy()
        assert (e[:, 1] > e[:, 0]).all() and bool((G['peak'] > 0).all())


def test_graph_replay_follows_the_device_samples(built_lib):
    """one capture on a side stream; the replay reads `samples` at replay time"""
    B, L = 3, 9000
    x = dev(np.stack([wr.burst(L, 2000, 7000, 1e-5), wr.family('noise', L), wr.family('bursts', L)]))
    first, second = [L, 4500, 0], [700, L, 2049]
    samples = dev(first, torch.int32)
    G = Guarded({'out': ((B, L), torch.float32, 'qnan'), 'pcm': ((B, L), torch.int16, 'ones'), 'bounds': ((B, 2), torch.int32, 'qnan'),
                 'peak': ((B,), torch.float32, 'qnan'), 'work': ((built_lib.wave_finish_workspace_floats(B, L),), torch.float32, 'qnan')})
    call = lambda: built_lib.wave_finish(x, samples, deemphasis=0.97, trim_top_db=40.0, out=G['out'], pcm=G['pcm'],  # noqa: E731
                                         bounds=G['bounds'], peak=G['peak'], work=G['work'])
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            call()
    torch.cuda.synchronize()
    for sm in (first, second, first):
        samples.copy_(dev(sm, torch.int32))
        G.refill('out', 'pcm', 'bounds', 'peak', 'work')
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        G.check('out', 'bounds', 'peak')
        want = _finish(built_lib, x, sm, a=0.97, db=40.0)
        for name, w in zip(('out', 'pcm', 'bounds', 'peak'), want):
            got = G[name].cpu().numpy()
            assert np.array_equal(got.view(np.uint8), w.view(np.uint8)), 'replay with samples %s differs from the eager call in %s' % (sm, name)


# ---- host layers ----------------------------------------------------------------------------------------------------------------
def test_finish_waveform_forms_the_samples_on_the_device(built_lib):
    from tacotron_amd.griffinlim import finish_samples, finish_waveform
    r, F = 2, 24
    L = 300 * (F - 1)
    x = dev(np.stack([wr.burst(L, 1500, 5200, 1e-5), wr.family('noise', L), wr.family('bursts', L), wr.family('sine_dc', L)]))
    lengths = dev([12, 5, 2, 40], torch.int32)   # 24, 10, 4 (< 5: none) and 80 -> 24 frames
    want_n = [300 * 23, 300 * 9, 0, 300 * 23]
    assert finish_samples(lengths, r, L).tolist() == want_n
    got = finish_waveform(x, lengths, r, deemphasis=0.97, trim_top_db=40.0)
    ref = built_lib.wave_finish(x, dev(want_n, torch.int32), deemphasis=0.97, trim_top_db=40.0)
    torch.cuda.synchronize()
    for g, w in zip(got, ref):
        assert torch.equal(g, w)
    assert got[2].cpu().numpy()[2].tolist() == [0, 0]
    full = finish_waveform(x, deemphasis=0.97)
    assert full[2].cpu().numpy().tolist() == [[0, L]] * 4


RULE = dict(end_offset=200, hold=1, min_steps=5)   # target 0: every row stops after step 4 -> len_b = 8


def _raises(*a, **k):
    raise AssertionError('lib.wave_finish reached without --deemphasis / --trim-db')


def test_driver_finishes_on_the_device(built_lib, tmp_path, monkeypatch):
    """test() with deemphasis 0.97 and trim_db 40 writes wavs whose frames are the device's pcm[:e - s] and _trim.npy; it combines
    with stop and vocode_lengths; without the options the driver never reaches the entry point and its files are unchanged"""
    from tacotron_amd import test as drv
    from tacotron_amd.config import Config
    prompts = ['hello world.\n', 'a somewhat longer prompt, with punctuation!\n', 'short\n']

    def cfg():
        c = Config()
        c.data_path = str(tmp_path / 'no_data') + '/'
        c.max_decode_iter = 16
        return c

    seen = []
    real = built_lib.wave_finish

    def spy(*a, **k):
        r = real(*a, **k)
        seen.append((r[1].cpu().numpy(), r[2].cpu().numpy(), None if a[1] is None else a[1].cpu().numpy()))
        return r

    a = drv.parse_args(['--deemphasis', '--trim-db', '40'])
    assert a.deemphasis == 0.97 and a.trim_db == 40.0
    monkeypatch.setattr(built_lib, 'wave_finish', spy)
    r = cfg().r
    L = 300 * (16 * r - 1)
    fin, plain = tmp_path / 'fin', tmp_path / 'plain'
    assert drv.test(cfg(), prompts, out_dir=str(fin), n_iter=2, deemphasis=a.deemphasis, trim_db=a.trim_db) == 3
    assert len(seen) == 1 and seen[0][2] is None
    pcm, trim, _ = seen[0]
    for i in range(3):
        s, e = trim[i]
        assert np.load(fin / ('prompt_%03d_trim.npy' % i)).tolist() == [s, e] and 0 <= s < e <= L
        with wavefile.open(str(fin / ('prompt_%03d.wav' % i))) as f:
            assert f.getnframes() == e - s and f.getframerate() == 16000 and f.getsampwidth() == 2 and f.getnchannels() == 1
            assert f.readframes(e - s) == pcm[i, :e - s].astype('<i2').tobytes()
    # with stop and vocode_lengths: every row over the samples of its own 8 r frames
    rule = built_lib.TacoStopRule(**RULE)
    del seen[:]
    both = tmp_path / 'both'
    assert drv.test(cfg(), prompts, out_dir=str(both), n_iter=3, stop=rule, vocode_lengths=True, gl_momentum=0.99, deemphasis=0.9,
                    trim_db=None) == 3
    n = 300 * (8 * r - 1)
    assert len(seen) == 1 and seen[0][2].tolist() == [n] * 3
    for i in range(3):
        assert np.load(both / ('prompt_%03d_trim.npy' % i)).tolist() == [0, n]
        assert np.load(both / ('prompt_%03d_len.npy' % i)) == 8
        assert np.load(both / ('prompt_%03d_conv.npy' % i)).shape == (4,)
        with wavefile.open(str(both / ('prompt_%03d.wav' % i))) as f:
            assert f.getnframes() == n and f.readframes(n) == seen[0][0][i, :n].astype('<i2').tobytes()
    # stop without vocode_lengths: the vocoder runs over the full length, the finishing over the row's own samples
    del seen[:]
    assert drv.test(cfg(), prompts, out_dir=str(tmp_path / 'stop'), n_iter=2, stop=rule, trim_db=25.0) == 3
    assert seen[0][2].tolist() == [n] * 3
    # without the options: the entry point is never reached, and spectrogram / alignment files are those of the finished run
    monkeypatch.setattr(built_lib, 'wave_finish', _raises)
    assert drv.test(cfg(), prompts, out_dir=str(plain), n_iter=2) == 3
    assert not list(plain.glob('*_trim.npy'))
    for i in range(3):
        for kind in ('spec', 'align'):
            name = 'prompt_%03d_%s.npy' % (i, kind)
            assert open(fin / name, 'rb').read() == open(plain / name, 'rb').read(), name
        with wavefile.open(str(plain / ('prompt_%03d.wav' % i))) as f:
            assert f.getnframes() == L
    with pytest.raises(AssertionError):
        drv.test(cfg(), prompts, out_dir=str(tmp_path / 'x'), n_iter=2, deemphasis=0.97)
