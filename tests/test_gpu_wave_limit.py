"""GPU: taco_wave_limit (include/taco_hip.h) through the C ABI -- out, pcm, peaks and counts BIT FOR BIT against the float32
restatement (tests/limiter_ref.py: the entry point has no recursion, so there is no tolerance anywhere in that comparison), the
meter alone, griffinlim.level_waveform(limit=True), the per-row contract, determinism, poisoned buffers between guard bands, every
TACO_EINVAL case, graph replay and the driver's --limit.

THE TRUE-PEAK BAR of the composition.  The limiter bounds e s, the envelope of the input times the gain, not the envelope of the
product: the interpolated phases of (G x) s differ from those of G x times s where s moves.  On the two synthetic voiced rows below
(2 s at 16 kHz, target -16 LUFS, ceiling -1 dBTP, W = 24, P = 4, two passes) the float32 restatement's output reads at worst
WORST_OVER = 1.68e-6 above the ceiling (relative; 1.5e-5 dB) through the same meter.  The test asserts 4 x that, 6.7e-6, under a cap
of 0.1 dB (1.16e-2).  The cap is a condition: a kernel that needs more is wrong."""
import ctypes as C
import functools
import math
import wave as wavefile

import numpy as np
import pytest
import torch

from tests import limiter_ref as mr, wave_ref as wr
from tests.poison import Guarded

pytestmark = pytest.mark.gpu

WORST_OVER = 1.68e-6   # measured on the restatement, see above
DELTA = min(4 * WORST_OVER, 10.0 ** (0.1 / 20.0) - 1.0)
TWO_22 = 2.0 ** -22
W0, P0, T0 = mr.CASE_W, mr.CASE_P, mr.CASE_T


def dev(x, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(x), dtype=dtype, device='cuda')


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _limit(lib, x, samples=None, gain=None, ceiling=1.0, taps=None, window=None, want_out=None, want_pcm=None, fill='qnan', alias=False):
    """lib.wave_limit into poisoned buffers between guard bands (the workspace poisoned as well); every element of out, peaks and counts
    must have been written.  -> (out, pcm, peaks, counts) as NumPy arrays (None for an output not asked for).  alias: out is the wave"""
    xt = x.clone() if torch.is_tensor(x) else dev(x)
    B, L = xt.shape
    emit = window is not None
    want_out = emit if want_out is None else want_out
    want_pcm = emit if want_pcm is None else want_pcm
    W = 0 if window is None else len(window) // 2
    spec = {'peaks': ((B, 4), torch.float32, fill), 'counts': ((B, 2), torch.int32, fill),
            'work': ((lib.wave_limit_workspace_floats(B, L, W),), torch.float32, fill)}
    if want_out and not alias:
        spec['out'] = ((B, L), torch.float32, fill)
    if want_pcm:
        spec['pcm'] = ((B, L), torch.int16, fill)
    G = Guarded(spec)
    st = samples if samples is None or torch.is_tensor(samples) else dev(samples, torch.int32)
    gt = gain if gain is None or torch.is_tensor(gain) else dev(gain)
    r = lib.wave_limit(xt, st, gt, ceiling=ceiling, taps=taps, window=window, want_out=want_out, want_pcm=want_pcm,
                       out=(xt if alias else G['out']) if want_out else None, pcm=G['pcm'] if want_pcm else None, peaks=G['peaks'],
                       counts=G['counts'], work=G['work'])
    torch.cuda.synchronize()
    assert r[2] is G['peaks'] and r[3] is G['counts'] and (r[0] is None) == (not want_out) and (r[1] is None) == (not want_pcm)
    # (0 is a legal sample and the fill of the clean run; every int16 value is a legal PCM sample: that `pcm` is written everywhere is
    # shown by test_same_arguments_same_bits_and_poison_changes_nothing, where all-zero and all-ones fills end in the same bits)
    G.check(*[k for k in ('out', 'peaks', 'counts') if k in spec and fill != 'zeros'])
    return tuple(None if t is None else t.cpu().numpy() for t in r)


def _against(name, got, want):
    for what, g, w in zip(('out', 'pcm', 'peaks', 'counts'), got, want):
        if w is None:
            assert g is None
            continue
        if not same_bits(g, w):
            bad = np.argwhere(np.ascontiguousarray(g).view({2: np.uint16, 4: np.uint32}[g.dtype.itemsize])
                              != np.ascontiguousarray(w).view({2: np.uint16, 4: np.uint32}[w.dtype.itemsize]))
            first = tuple(bad[0])
            raise AssertionError('%s: %s differs from the float32 restatement in %d places, first at %s: %r, expected %r'
                                 % (name, what, len(bad), first, g[first], w[first]))


# ---- 1: bit for bit -----------------------------------------------------------------------------------------------------------
def test_edges_bit_for_bit(built_lib):
    """n_b in {0, 1, 5, 6, 16, 17, 33, 2047, 2048, 2049, 2064, 4097}, NaN behind n_b, an impulse at sample 0, n_b - 1, 2047 and 2048:
    the dips straddle the chunk edge and the rows' ends.  P = 4, T = 12, W = 8; L = 4099 puts the rows at every alignment"""
    x, ns, gain, ceiling = mr.edge_rows()
    tp, win = mr.taps(P0, T0), mr.window(W0)
    got = _limit(built_lib, x, ns, gain, ceiling, tp, win)
    clean = np.nan_to_num(x, nan=0.0)
    want = mr.limit_rows(clean, ns, gain, ceiling=ceiling, tp=tp, win=win)
    _against('edges', got, want)
    assert got[3][:, 0].tolist() == list(mr.EDGE_NS) and (got[3][2:, 1] > 0).all()
    assert got[2][0].tolist() == [0.0, float(gain[0]), 1.0, 0.0]
    for b, n in enumerate(ns):
        assert not got[0][b, n:].view(np.uint32).any() and not got[1][b, n:].any()


def test_shapes_bit_for_bit(built_lib):
    """merging and separate dips, a plateau across the chunk edge, the fs/4 sine at 45 degrees (limited at P = 4, untouched at P = 1),
    a row under the ceiling (nothing limited, out = fl(G x) exactly) and noise at G = 4"""
    x, gain = mr.shape_rows()
    tp, win = mr.taps(P0, T0), mr.window(W0)
    got = _limit(built_lib, x, None, gain, mr.SHAPE_CEILING, tp, win)
    _against('shapes', got, mr.limit_rows(x, None, gain, ceiling=mr.SHAPE_CEILING, tp=tp, win=win))
    out, pcm, peaks, counts = got
    assert counts[2, 1] > 0 and peaks[2, 0] > mr.SHAPE_CEILING > np.abs(x[2]).max()      # the sine: only its true peak is over
    assert counts[3, 1] == 0 and peaks[3, 2] == 1.0 and same_bits(out[3], np.float32(2.0) * x[3])
    assert counts[4, 1] > 0 and peaks[4, 3] <= np.float32(mr.SHAPE_CEILING) * (1 + TWO_22)
    one = _limit(built_lib, x[2:3], None, None, mr.SHAPE_CEILING, np.zeros((0, T0), np.float32), win)
    _against('sine at P = 1', one, mr.limit_rows(x[2:3], ceiling=mr.SHAPE_CEILING, tp=None, win=win))
    assert one[3][0, 1] == 0 and same_bits(one[0][0], x[2])


@pytest.mark.parametrize('P,T,W', [(4, 12, 0), (4, 12, 1), (4, 12, 512), (1, 12, 8), (2, 12, 8), (8, 12, 8), (4, 2, 8), (4, 32, 8)])
def test_other_settings_bit_for_bit(built_lib, P, T, W):
    """one noise row of L = 4100 at G = 4 per setting: the shortest and the longest look-ahead, the fewest and the most phases and taps"""
    x = wr.family('noise', mr.SHAPE_L)[None, :4100]
    tp, win = mr.taps(P, T), mr.window(W)
    got = _limit(built_lib, x, None, [4.0], mr.SHAPE_CEILING, tp, win)
    _against('P = %d, T = %d, W = %d' % (P, T, W), got, mr.limit_rows(x, None, [4.0], ceiling=mr.SHAPE_CEILING, tp=tp, win=win))
    assert got[3][0, 1] > 0


# ---- 2: the meter -----------------------------------------------------------------------------------------------------------------
def test_measure_only(built_lib):
    """tp_in bit-equal to the restatement; peaks = (tp_in, 1, 1, max |x|), counts = (n_b, 0); gain, ceiling, window and W are not
    looked at: NaN, NULL and out-of-range values pass"""
    lib = built_lib
    x, ns, gain, _ = mr.edge_rows()
    tp = mr.taps(P0, T0)
    _, _, peaks, counts = _limit(lib, x, ns, None, taps=tp)
    want = mr.limit_rows(np.nan_to_num(x, nan=0.0), ns, tp=tp)
    assert same_bits(peaks, want[2]) and np.array_equal(counts, want[3])
    assert (peaks[:, 1:3] == 1.0).all() and (counts[:, 1] == 0).all()
    sx, _ = mr.shape_rows()
    _, _, p2, c2 = _limit(lib, sx, taps=tp)
    assert same_bits(p2, mr.limit_rows(sx, tp=tp)[2]) and -0.4 <= 20 * math.log10(p2[2, 0] / 0.5) <= 0.2   # (Tech 3341; the row's ends included)
    assert same_bits(_limit(lib, sx, taps=np.zeros((0, T0), np.float32))[2][:, 0], np.abs(sx).max(axis=1))   # P = 1: the sample peak
    fn = C.CDLL(lib.LIB_PATH).taco_wave_limit
    fn.restype, fn.argtypes = lib.EXPORTS['taco_wave_limit']
    xt, st, tt = dev(x), dev(ns, torch.int32), dev(tp)
    for g, ceiling, win, W in ((None, float('nan'), None, -5), (dev(np.full(len(ns), np.nan, np.float32)), -1.0, None, 9999),
                               (None, 2.0, dev(np.full(3, np.nan, np.float32)), 1)):
        G = Guarded({'peaks': ((len(ns), 4), torch.float32, 'qnan'), 'counts': ((len(ns), 2), torch.int32, 'qnan'),
                     'work': ((lib.wave_limit_workspace_floats(len(ns), x.shape[1], 0),), torch.float32, 'qnan')})
        assert fn(lib.ptr(xt), lib.ptr(st), lib.ptr(g), ceiling, lib.ptr(tt), P0, T0, lib.ptr(win), W, None, None, lib.ptr(G['peaks']),
                  lib.ptr(G['counts']), lib.ptr(G['work']), len(ns), x.shape[1], lib.stream_ptr()) == 0
        torch.cuda.synchronize()
        G.check('peaks', 'counts')
        assert same_bits(G['peaks'].cpu().numpy(), peaks) and np.array_equal(G['counts'].cpu().numpy(), counts)


# ---- 3: the composition -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _voiced():
    x = np.stack([mr.voiced(32000, 16000, 110.0, 3), mr.voiced(32000, 16000, 180.0, 5)])
    x.setflags(write=False)
    return x


def test_level_waveform_reaches_the_target_under_the_true_peak(built_lib):
    """two synthetic voiced rows of 2 s with one click each, target -16 LUFS, ceiling -1 dB: today's path holds both rows down
    (blocks[:, 3] == 1, asserted first) and delivers them more than 10 LU low; level_waveform(limit=True, passes=2) reaches the target
    far nearer, with sample peak <= ceiling (1 + 2^-22) and the meter's true peak of the output <= ceiling (1 + DELTA).
    Measured on the restatement: overshoot 1.68e-6 at worst, DELTA = 6.7e-6; see the module's docstring"""
    from tacotron_amd.griffinlim import level_waveform
    lib = built_lib
    target, ceiling_db = -16.0, -1.0
    c32 = float(np.float32(10.0 ** (ceiling_db / 20.0)))
    x = dev(_voiced())
    held = lib.wave_loudness(x, None, sr=16000, target=target, ceiling=10.0 ** (ceiling_db / 20.0))
    assert bool((held[3][:, 3] == 1).all())
    I_in, g_held = held[2][:, 0].cpu().numpy().astype(np.float64), held[2][:, 2].cpu().numpy().astype(np.float64)
    reached_held = I_in + 20 * np.log10(g_held)
    out, pcm, loud, blocks, peaks, counts = level_waveform(x, target=target, ceiling_db=ceiling_db, limit=True, passes=2)
    tp_out = lib.wave_limit(out)[2][:, 0].cpu().numpy().astype(np.float64)
    I_out, pk = loud[:, 0].cpu().numpy().astype(np.float64), peaks.cpu().numpy()
    n_lim = counts.cpu().numpy()
    for b in range(2):
        print('  row %d: %.2f LUFS; held down -> %.2f; limited -> %.2f (asked %g); G %.3f, deepest %.2f dB, %d samples limited; '
              'sample peak / ceiling - 1 = %.2e, true peak / ceiling - 1 = %.2e (bar %.2e)'
              % (b, I_in[b], reached_held[b], I_out[b], target, pk[b, 1], 20 * math.log10(pk[b, 2]), n_lim[b, 1], pk[b, 3] / c32 - 1,
                 tp_out[b] / c32 - 1, DELTA))
        # what the restatement does with the gain the device arrived at
        ref = mr.limit(_voiced()[b], pk[b, 1], 10.0 ** (ceiling_db / 20.0), mr.taps(), mr.window(24))
        assert same_bits(out[b].cpu().numpy(), ref['out']) and same_bits(pcm[b].cpu().numpy(), ref['pcm'])
        print('         the restatement with that G: true peak / ceiling - 1 = %.2e' % (float(mr.limit(ref['out'], tp=mr.taps())['peaks'][0]) / c32 - 1))
    assert (np.abs(I_out - target) < np.abs(reached_held - target)).all() and (np.abs(I_out - target) < 1.0).all()
    assert (reached_held < target - 10.0).all()
    assert (pk[:, 3] <= c32 * (1 + TWO_22)).all()
    assert (tp_out <= c32 * (1 + DELTA)).all(), (tp_out / c32 - 1, DELTA)
    assert (n_lim[:, 0] == 32000).all() and (n_lim[:, 1] > 0).all() and (n_lim[:, 1] < 3200).all()   # a neighbourhood, not the row
    assert same_bits(pcm.cpu().numpy(), mr.pcm16(out.cpu().numpy())) and bool((blocks[:, 3] == 0).all())
    one = level_waveform(x, target=target, ceiling_db=ceiling_db, limit=True, passes=1)
    assert (np.abs(one[2][:, 0].cpu().numpy() - target) >= np.abs(I_out - target) - 1e-3).all()   # the second pass does not lose ground
    sample = level_waveform(x, target=target, ceiling_db=ceiling_db, limit=True, oversample=1, lookahead_ms=0.0, passes=1)
    assert bool((sample[4][:, 3] <= c32 * (1 + TWO_22)).all())


# ---- 4: the contract ---------------------------------------------------------------------------------------------------------------
ROWS_N = [6000, 0, 1, 2049, 4500]


def _rows_input():
    x = np.stack([wr.burst(6000, 1000, 5000, 1e-5), wr.family('noise', 6000), wr.family('bursts', 6000), wr.burst(6000, 500, 2040, 3e-6),
                  wr.family('same_sign', 6000)]).astype(np.float32)
    x[3, 2047] = 0.9
    xin = x.copy()
    for b, n in enumerate(ROWS_N):
        xin[b, n:] = np.nan
    return x, xin, np.array([3.0, 2.0, 1.0, 2.5, 6.0], np.float32)


def test_rows_are_the_call_on_each_row_alone(built_lib):
    """B = 5, L = 6000, samples = [L, 0, 1, 2049, 4500], NaN behind each n_b: row b is bit-identical to its own B = 1, L = n_b call on
    a contiguous copy, for out, pcm, peaks and counts; and out aliasing wave gives the bits of the separate buffer"""
    x, xin, gain = _rows_input()
    tp, win = mr.taps(), mr.window(24)
    out, pcm, peaks, counts = _limit(built_lib, xin, ROWS_N, gain, 0.5, tp, win)
    assert np.isfinite(out).all() and counts[:, 1].sum() > 0
    for b, n in enumerate(ROWS_N):
        assert not out[b, n:].view(np.uint32).any() and not pcm[b, n:].any()
        if n == 0:
            assert peaks[b].tolist() == [0.0, 2.0, 1.0, 0.0] and counts[b].tolist() == [0, 0]
            continue
        o1, p1, k1, c1 = _limit(built_lib, np.ascontiguousarray(x[b:b + 1, :n]), None, gain[b:b + 1], 0.5, tp, win)
        assert same_bits(peaks[b:b + 1], k1) and np.array_equal(counts[b:b + 1], c1), (b, peaks[b], k1)
        assert same_bits(out[b, :n], o1[0]) and same_bits(pcm[b, :n], p1[0]), b
    a = _limit(built_lib, xin, ROWS_N, gain, 0.5, tp, win, alias=True)
    assert same_bits(a[0], out) and same_bits(a[1], pcm) and same_bits(a[2], peaks) and np.array_equal(a[3], counts)
    a = _limit(built_lib, xin, ROWS_N, gain, 0.5, tp, mr.window(512), alias=True, want_pcm=False)   # the widest halo, across three chunks
    b = _limit(built_lib, xin, ROWS_N, gain, 0.5, tp, mr.window(512), want_pcm=False)
    assert same_bits(a[0], b[0]) and same_bits(a[2], b[2])
    o_only = _limit(built_lib, xin, ROWS_N, gain, 0.5, tp, win, want_pcm=False)
    p_only = _limit(built_lib, xin, ROWS_N, gain, 0.5, tp, win, want_out=False)
    assert same_bits(o_only[0], out) and same_bits(p_only[1], pcm) and same_bits(o_only[2], peaks) and same_bits(p_only[2], peaks)


def test_same_arguments_same_bits_and_poison_changes_nothing(built_lib):
    """two calls give the same bits; a NaN / all-ones / noise workspace and output fill give the bits of the zero-filled call"""
    x, xin, gain = _rows_input()
    tp, win = mr.taps(), mr.window(24)
    ref = _limit(built_lib, xin, ROWS_N, gain, 0.5, tp, win, fill='zeros')
    for fill in ('zeros', 'qnan', 'ones', 'noise'):
        got = _limit(built_lib, xin, ROWS_N, gain, 0.5, tp, win, fill=fill)
        for name, r, g in zip(('out', 'pcm', 'peaks', 'counts'), ref, got):
            assert same_bits(r, g), (fill, name)
        got = _limit(built_lib, xin, ROWS_N, gain, 0.5, tp, win, fill=fill, alias=True)
        assert same_bits(ref[0], got[0]) and same_bits(ref[1], got[1]), fill
    m_ref = _limit(built_lib, xin, ROWS_N, taps=tp, fill='zeros')
    m_got = _limit(built_lib, xin, ROWS_N, taps=tp, fill='noise')
    assert same_bits(m_ref[2], m_got[2]) and np.array_equal(m_ref[3], m_got[3]) and same_bits(m_ref[2][:, 0], ref[2][:, 0])


@pytest.mark.parametrize('L', [4097, 4098, 4099])
def test_odd_row_pitches(built_lib, L):
    """row pitches that are no multiple of 4: the rows of out and pcm start at every 4-byte / 2-byte alignment"""
    rng = np.random.default_rng(L)
    x = (0.3 * rng.standard_normal((4, L))).astype(np.float32)
    ns = [L, L - 1, 2050, 3]
    tp, win = mr.taps(), mr.window(W0)
    got = _limit(built_lib, x, ns, None, 0.5, tp, win)
    _against('L = %d' % L, got, mr.limit_rows(x, ns, ceiling=0.5, tp=tp, win=win))


def test_bad_arguments_enqueue_nothing(built_lib):
    """every TACO_EINVAL case returns before a launch: the outputs and the workspace keep their sentinel; the error string names
    wave_limit; the size function refuses the same shapes; the good arguments run with every nullable argument NULL in turn"""
    lib = built_lib
    B, L, W = 2, 5000, 8
    x = dev(np.stack([wr.burst(L, 1200, 3100, 1e-5), wr.family('noise', L)]))
    sm, gn = dev([L, 3000], torch.int32), dev([2.0, 5.0])
    tp, win = dev(mr.taps()), dev(mr.window(W))
    G = Guarded({'out': ((B, L), torch.float32, 7.0), 'pcm': ((B, L), torch.int16, 7.0), 'peaks': ((B, 4), torch.float32, 7.0),
                 'counts': ((B, 2), torch.int32, 7.0), 'work': ((lib.wave_limit_workspace_floats(B, L, W),), torch.float32, 7.0)})
    fn = C.CDLL(lib.LIB_PATH).taco_wave_limit
    fn.restype, fn.argtypes = lib.EXPORTS['taco_wave_limit']
    good = dict(wave=lib.ptr(x), samples=lib.ptr(sm), gain=lib.ptr(gn), ceiling=0.5, taps=lib.ptr(tp), P=4, T=12, window=lib.ptr(win), W=W,
                out=lib.ptr(G['out']), pcm=lib.ptr(G['pcm']), peaks=lib.ptr(G['peaks']), counts=lib.ptr(G['counts']), work=lib.ptr(G['work']),
                B=B, L=L)
    order = ('wave', 'samples', 'gain', 'ceiling', 'taps', 'P', 'T', 'window', 'W', 'out', 'pcm', 'peaks', 'counts', 'work', 'B', 'L')
    cases = [{'wave': None}, {'peaks': None}, {'counts': None}, {'work': None}, {'B': 0}, {'B': -1}, {'L': 0}, {'L': -5},
             {'P': 0}, {'P': 9}, {'P': -1}, {'T': 0}, {'T': 1}, {'T': 11}, {'T': 34}, {'T': -2}, {'W': -1}, {'W': 513},
             {'taps': None}, {'window': None}, {'window': None, 'out': None}, {'window': None, 'pcm': None},
             {'ceiling': 0.0}, {'ceiling': -0.5}, {'ceiling': 1.5}, {'ceiling': float('nan')}, {'ceiling': float('inf')},
             {'ceiling': 2.0, 'out': None}, {'W': 600, 'pcm': None},
             {'out': None, 'pcm': None, 'P': 9}, {'out': None, 'pcm': None, 'T': 3}, {'out': None, 'pcm': None, 'taps': None}]
    everything = {k: torch.ones(G[k].shape, dtype=torch.bool, device='cuda') for k in ('out', 'pcm', 'peaks', 'counts', 'work')}
    for change in cases:
        for samples in (good['samples'], None):
            a = dict(good, samples=samples)
            a.update(change)
            lib.wave_limit_workspace_floats(B, L, W)   # (a successful call in between: the string below is this refusal's)
            rc = fn(*[a[k] for k in order], lib.stream_ptr())
            torch.cuda.synchronize()
            msg = lib.last_error()
            print('  %r, samples %s: rc %d, %s' % (change, 'given' if samples else 'NULL', rc, msg))
            assert rc == -1, (change, rc)
            assert 'wave_limit: ' in msg
            for name, m in everything.items():
                assert G.margin_intact(name, m), '%s was written although %r is refused' % (name, change)
    G.check()
    size = C.CDLL(lib.LIB_PATH).taco_wave_limit_workspace_bytes
    size.restype, size.argtypes = lib.EXPORTS['taco_wave_limit_workspace_bytes']
    assert [size(*a) for a in ((0, L, W), (-1, L, W), (B, 0, W), (B, -5, W), (B, L, -1), (B, L, 513))] == [-1] * 6 and size(B, L, 512) > 0
    # and the good arguments do run, with every nullable argument NULL in turn; P = 1 does not look at taps
    for null, extra in (((), {}), (('samples',), {}), (('gain',), {}), (('out',), {}), (('pcm',), {}), (('samples', 'gain', 'pcm'), {}),
                        (('taps',), {'P': 1}), (('out', 'pcm', 'window', 'gain'), {'ceiling': float('nan'), 'W': -1})):
        a = dict(good, **extra)
        for k in null:
            a[k] = None
        G.refill('out', 'pcm', 'peaks', 'counts', 'work')
        assert fn(*[a[k] for k in order], lib.stream_ptr()) == 0, null
        torch.cuda.synchronize()
        G.check()
        for k in ('out', 'pcm'):
            if k in null:
                assert G.margin_intact(k, everything[k])
            else:
                assert not bool(torch.isnan(G[k].float()).any()) and not G.margin_intact(k, everything[k])
        assert bool(torch.isfinite(G['peaks']).all()) and bool((G['counts'][:, 0] > 0).all())
        if 'out' in null and 'pcm' in null:
            assert G['peaks'][:, 1].tolist() == [1.0, 1.0] and G['counts'][:, 1].tolist() == [0, 0]


def test_graph_replay_follows_the_device_samples_and_gain(built_lib):
    """one linear capture on a side stream; three replays under different `samples` and `gain` equal the eager calls"""
    B, L = 3, 9000
    x = dev(np.stack([wr.burst(L, 2000, 7000, 1e-5), wr.family('noise', L), wr.family('bursts', L)]))
    runs = (([L, 4500, 0], [3.0, 4.0, 1.0]), ([700, L, 2049], [1.0, float('nan'), 8.0]), ([6400, 1, 8999], [0.5, 2.0, -1.0]))
    samples, gain = dev(runs[0][0], torch.int32), dev(runs[0][1])
    tp, win = dev(mr.taps()), dev(mr.window(24))
    G = Guarded({'out': ((B, L), torch.float32, 'qnan'), 'pcm': ((B, L), torch.int16, 'ones'), 'peaks': ((B, 4), torch.float32, 'qnan'),
                 'counts': ((B, 2), torch.int32, 'qnan'), 'work': ((built_lib.wave_limit_workspace_floats(B, L, 24),), torch.float32, 'qnan')})
    call = lambda: built_lib.wave_limit(x, samples, gain, ceiling=0.5, taps=tp, window=win, out=G['out'], pcm=G['pcm'],  # noqa: E731
                                        peaks=G['peaks'], counts=G['counts'], work=G['work'])
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            call()
    torch.cuda.synchronize()
    for sm, gn in runs:
        samples.copy_(dev(sm, torch.int32))
        gain.copy_(dev(gn))
        G.refill('out', 'pcm', 'peaks', 'counts', 'work')
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        G.check('out', 'peaks', 'counts')
        want = _limit(built_lib, x, sm, gn, 0.5, mr.taps(), mr.window(24))
        for name, w in zip(('out', 'pcm', 'peaks', 'counts'), want):
            assert same_bits(G[name].cpu().numpy(), w), 'replay with samples %s, gain %s differs from the eager call in %s' % (sm, gn, name)
        assert want[2][:, 1].tolist() == [v if v > 0 else 1.0 for v in gn]   # (a gain that is no finite positive number counts as 1)


# ---- 5: the driver ------------------------------------------------------------------------------------------------------------------
RULE = dict(end_offset=200, hold=1, min_steps=5)   # target 0: every row stops after step 4 -> len_b = 8
LONG = ('the first sentence of this prompt is long enough to fill a good part of one piece on its own, and it ends here. '
        'the second one has no full stop for a long while, only a comma after a run of words that goes on and on and on, '
        'and then more words that follow the comma until the line has well over three hundred characters in it.\n')


def _raises(*a, **k):
    raise AssertionError('lib.wave_limit reached without --limit')


def test_driver_limits_on_the_device(built_lib, tmp_path, monkeypatch, capsys):
    """test() with loudness -16 and limit writes wavs whose frames are the kernel's pcm, _limit.npy with the eight columns and the
    line; with long the joined prompt is limited; the same run without limit never reaches lib.wave_limit and writes byte-identical
    files to a run whose options were parsed without the flag"""
    from tacotron_amd import test as drv
    from tacotron_amd.config import Config
    prompts = ['hello world.\n', 'a somewhat longer prompt, with punctuation!\n', 'short\n']

    def cfg():
        c = Config()
        c.data_path = str(tmp_path / 'no_data') + '/'
        c.max_decode_iter = 16
        return c

    seen = []
    real = built_lib.wave_limit

    def spy(*a, **k):
        r = real(*a, **k)
        seen.append(tuple(None if t is None else t.cpu().numpy() for t in r) + (k,))
        return r

    a = drv.parse_args(['--loudness', '-16', '--limit'])
    monkeypatch.setattr(built_lib, 'wave_limit', spy)
    r = cfg().r
    L = 300 * (16 * r - 1)
    lim = tmp_path / 'lim'
    kw = dict(n_iter=2, loudness=a.loudness, peak_db=a.peak_db, limit=a.limit, limit_ms=a.limit_ms, true_peak=a.true_peak,
              limit_passes=a.limit_passes)
    assert drv.test(cfg(), prompts, out_dir=str(lim), **kw) == 3
    assert len(seen) == 3 and seen[2][0] is None   # two passes, then the meter on the output
    assert abs(seen[0][4]['ceiling'] - 10 ** (-1 / 20)) < 1e-12 and tuple(seen[0][4]['window'].shape) == (49,)
    pcm, peaks, counts, tp_out = seen[1][1], seen[1][2], seen[1][3], seen[2][2][:, 0]
    printed = capsys.readouterr().out
    for i in range(3):
        row = np.load(lim / ('prompt_%03d_limit.npy' % i))
        assert row.dtype == np.float64 and row.shape == (8,)
        assert row[:6].tolist() == peaks[i].astype(np.float64).tolist() + counts[i].astype(np.float64).tolist() and row[7] == tp_out[i]
        assert row[4] == L and row[3] <= float(np.float32(10 ** (-1 / 20))) * (1 + TWO_22)
        line = [ln for ln in printed.splitlines() if ln.startswith('prompt %d: ' % i)]
        assert len(line) == 1 and ('(asked -16.0), true peak ' in line[0] or 'level unchanged' in line[0]), line
        assert not (lim / ('prompt_%03d_loud.npy' % i)).exists()
        with wavefile.open(str(lim / ('prompt_%03d.wav' % i))) as f:
            assert f.getnframes() == L and f.getframerate() == 16000 and f.getsampwidth() == 2 and f.getnchannels() == 1
            assert f.readframes(L) == pcm[i].astype('<i2').tobytes()
    # with long: the JOINED prompts are limited, once per group
    del seen[:]
    rule = built_lib.TacoStopRule(**RULE)
    joined = tmp_path / 'joined'
    assert drv.test(cfg(), prompts[:2] + [LONG], out_dir=str(joined), n_iter=2, stop=rule, long=True, loudness=-16.0, limit=True,
                    limit_passes=1, true_peak=2, limit_ms=3.0) == 3
    assert len(seen) == 2 and seen[0][1].shape[0] == 3 and tuple(seen[0][4]['window'].shape) == (97,) and tuple(seen[0][4]['taps'].shape) == (1, 12)
    total = seen[0][3][:, 0]
    for i in range(3):
        row = np.load(joined / ('prompt_%03d_limit.npy' % i))
        assert row[4] == total[i] and row[:4].tolist() == seen[0][2][i].astype(np.float64).tolist()
        with wavefile.open(str(joined / ('prompt_%03d.wav' % i))) as f:
            assert f.getnframes() == total[i] and f.readframes(int(total[i])) == seen[0][1][i, :total[i]].astype('<i2').tobytes()
    assert not list(joined.glob('prompt_002_k*_limit.npy'))
    # without the flag: the entry point is never reached, and every file is the one of a run that was never given the keywords
    monkeypatch.setattr(built_lib, 'wave_limit', _raises)
    b = drv.parse_args(['--loudness', '-16'])
    off, before = tmp_path / 'off', tmp_path / 'before'
    assert drv.test(cfg(), prompts, out_dir=str(off), n_iter=2, loudness=b.loudness, peak_db=b.peak_db, limit=b.limit, limit_ms=b.limit_ms,
                    true_peak=b.true_peak, limit_passes=b.limit_passes) == 3
    assert drv.test(cfg(), prompts, out_dir=str(before), n_iter=2, loudness=-16.0) == 3
    names = sorted(p.name for p in off.iterdir())
    assert names == sorted(p.name for p in before.iterdir()) and not list(off.glob('*_limit.npy')) and len(list(off.glob('*_loud.npy'))) == 3
    for name in names:
        assert open(off / name, 'rb').read() == open(before / name, 'rb').read(), name
    with pytest.raises(AssertionError):
        drv.test(cfg(), prompts, out_dir=str(tmp_path / 'x'), n_iter=2, loudness=-16.0, limit=True)
