"""GPU: taco_wave_loudness (include/taco_hip.h) through the C ABI -- the readings against the fp64 restatement
(tests/loudness_ref.py) on inputs whose distance from both gates the test asserts first, the carry across chunks, the smallest rows,
the gain and PCM16 bit for bit against the entry point's fp32 rule, the per-row contract, determinism, poisoned buffers between
guard bands, every TACO_EINVAL case, graph replay, griffinlim.level_waveform and the driver's --loudness / --peak-db.

THE BAR.  The worst |I - I_ref| and |M - M_ref| over the fp64 cases below (six rows of 107,700 samples at 16 and 24 kHz, the two
chunk-carry rows at 48 kHz), measured on an MI355X, is WORST_LU = 2.23e-6 LU -- the impulse row at 48 kHz, which reads -29.99: one
unit in the last place of an fp32 reading between -16 and -32 is 1.9e-6.  (16 kHz rows: 1.32e-6 at worst, 60 Hz + DC; 24 kHz rows:
7.2e-7; the DC step at 48 kHz: 2.9e-7.)  The tests assert 4 x that figure, 8.9e-6 LU -- room for box-to-box differences in nothing
but summation order -- under a cap of 0.01 LU, a tenth of the meter tolerance of EBU Tech 3341.  The cap is a condition: a kernel
that needs more is wrong, not imprecise.  (A first form of the kernel, with its zero-state runs in fp32, read the DC step 0.0156 LU
high and was: DESIGN.md 4b.)"""
import ctypes as C
import functools
import math
import wave as wavefile

import numpy as np
import pytest
import torch

from tests import loudness_ref as lr, wave_ref as wr
from tests.poison import Guarded

pytestmark = pytest.mark.gpu

L_FULL = wr.L_FULL
WORST_LU = 2.23e-6   # measured, see above
BAR = min(4 * WORST_LU, 0.01)
MARGIN = 0.05       # LU: no block of a compared row lies nearer to either gate


def dev(x, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(x), dtype=dtype, device='cuda')


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({2: np.uint16, 4: np.uint32}[x.dtype.itemsize])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def _loud(lib, x, samples=None, sr=16000, target=None, ceiling=1.0, want_out=None, want_pcm=None, fill='qnan', alias=False):
    """lib.wave_loudness into poisoned buffers between guard bands (the workspace poisoned as well); every element of every output
    must have been written.  -> (out, pcm, loud, blocks) as NumPy arrays (None for an output not asked for).  alias: out is the wave"""
    xt = x.clone() if torch.is_tensor(x) else dev(x)
    B, L = xt.shape
    want_out = target is not None if want_out is None else want_out
    want_pcm = target is not None if want_pcm is None else want_pcm
    spec = {'loud': ((B, 4), torch.float32, fill), 'blocks': ((B, 4), torch.int32, fill),
            'work': ((lib.wave_loudness_workspace_floats(B, L, sr),), torch.float32, fill)}
    if want_out and not alias:
        spec['out'] = ((B, L), torch.float32, fill)
    if want_pcm:
        spec['pcm'] = ((B, L), torch.int16, fill)
    G = Guarded(spec)
    st = samples if samples is None or torch.is_tensor(samples) else dev(samples, torch.int32)
    r = lib.wave_loudness(xt, st, sr=sr, target=target, ceiling=ceiling, want_out=want_out, want_pcm=want_pcm,
                          out=(xt if alias else G['out']) if want_out else None, pcm=G['pcm'] if want_pcm else None, loud=G['loud'],
                          blocks=G['blocks'], work=G['work'])
    torch.cuda.synchronize()
    assert r[2] is G['loud'] and r[3] is G['blocks'] and (r[0] is None) == (not want_out) and (r[1] is None) == (not want_pcm)
    # (0 is a legal sample and the fill of the clean run; every int16 value is a legal PCM sample: that `pcm` is written everywhere is
    # shown by test_same_arguments_same_bits_and_poison_changes_nothing, where all-zero and all-ones fills end in the same bits)
    G.check(*[k for k in ('out', 'loud', 'blocks') if k in spec and fill != 'zeros'])
    return tuple(None if t is None else t.cpu().numpy() for t in r)


# ---- against fp64 ------------------------------------------------------------------------------------------------------------
FP64_ROWS = wr.FAMILIES + ('burst', 'hum_dc')


@functools.lru_cache(maxsize=None)
def _fp64_input():
    x = np.stack([wr.family(f) for f in wr.FAMILIES] + [wr.burst(L_FULL, 20011, 70003, 1e-5), lr.hum_dc(L_FULL, 16000)])
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _fp64_reference(sr):
    return [lr.measure(row, sr) for row in _fp64_input()]


def _compare(name, got_loud, got_blocks, ref):
    """precondition first, then equal blocks and readings under the bar -> the worst difference in LU"""
    assert ref['margin'] >= MARGIN, 'the input does not satisfy the precondition: a block of %s lies %.3f LU from a gate' % (name, ref['margin'])
    dI, dM = abs(float(got_loud[0]) - ref['I']), abs(float(got_loud[1]) - ref['M'])
    print('  %-10s blocks %s (fp64 %s), I %.5f (fp64 %.5f, off %.2e), M %.5f (off %.2e), nearest block %.2f LU from a gate'
          % (name, tuple(int(v) for v in got_blocks[:3]), ref['blocks'], got_loud[0], ref['I'], dI, got_loud[1], dM, ref['margin']))
    assert tuple(int(v) for v in got_blocks[:3]) == ref['blocks'], name
    assert dI <= BAR and dM <= BAR, (name, dI, dM, BAR)
    return max(dI, dM)


@pytest.mark.parametrize('sr', [16000, 24000])
def test_readings_against_fp64(built_lib, sr):
    """the four families of tests/wave_ref.py, a burst row (both gates cut blocks) and 60 Hz + DC (what the high-pass removes) at
    L = 107,700: no block within 0.05 LU of a gate (asserted on the restatement), then blocks EQUAL and |I - I_ref|, |M - M_ref| <= BAR.
    Measured on an MI355X: see WORST_LU"""
    x = _fp64_input()
    refs = _fp64_reference(sr)
    _, _, loud, blocks = _loud(built_lib, x, sr=sr)
    worst = max(_compare(name, loud[i], blocks[i], refs[i]) for i, name in enumerate(FP64_ROWS))
    print('  sr %d: worst difference %.3e LU (bar %.3e)' % (sr, worst, BAR))
    assert (loud[:, 2] == 1.0).all() and (blocks[:, 3] == 0).all()                   # measure-only
    assert np.array_equal(loud[:, 3], np.abs(x).max(axis=1))                         # peak_out = peak_in, exact
    assert refs[4]['blocks'][2] < refs[4]['blocks'][1] < refs[4]['blocks'][0]        # (the burst row does meet both gates)


def test_chunk_carry(built_lib):
    """sr 48000 (pole radius 0.995: a state has 3.7e-5 of itself left after a chunk), L = 5 chunks + 1: a unit impulse at the LAST
    sample of every chunk -- all of its response lies in the next chunk -- and a DC step in the middle of a chunk.  A kernel that drops or
    misplaces the state between chunks loses most of that energy; the rows meet the bar of the fp64 comparison"""
    chunk = built_lib.LOUD_CHUNK
    x = lr.chunk_carry_rows(chunk)
    assert x.shape == (2, 5 * chunk + 1) and x[0].sum() == 5 and x[0, chunk - 1] == 1 and x[0, 5 * chunk - 1] == 1
    _, _, loud, blocks = _loud(built_lib, x, sr=48000)
    for i, name in enumerate(('impulses', 'step')):
        ref = lr.measure(x[i], 48000)
        _compare(name, loud[i], blocks[i], ref)
        # what dropping the carry would cost: the row filtered chunk by chunk from a zero state
        cut = np.concatenate([lr.k_filter(x[i, c:c + chunk], 48000) for c in range(0, x.shape[1], chunk)])
        lost = abs(lr.lufs(float(np.mean(cut * cut))) - ref['I'])
        print('  %s: a kernel without the carry would be off by %.2f LU' % (name, lost))
        assert lost > 0.05   # (five times the cap on the bar)


# ---- smallest shapes -----------------------------------------------------------------------------------------------------------
def test_smallest_rows(built_lib):
    """n_b in {0, 1, H - 1, H, 4H - 1, 4H, 4H + 1, 5H, CHUNK - 1, CHUNK, CHUNK + 1} and an all-zero row, NaN behind n_b"""
    sr, H, chunk = 16000, 1600, built_lib.LOUD_CHUNK
    ns = [0, 1, H - 1, H, 4 * H - 1, 4 * H, 4 * H + 1, 5 * H, chunk - 1, chunk, chunk + 1, 5 * H]
    L = 5 * H + 3
    x = (0.1 * np.random.default_rng(5).standard_normal((len(ns), L))).astype(np.float32)
    x[-1] = 0.0   # the all-zero row
    xin = x.copy()
    for b, n in enumerate(ns):
        xin[b, n:] = np.nan
    out, pcm, loud, blocks = _loud(built_lib, xin, ns, sr=sr, target=-23.0, ceiling=1.0)
    for b, n in enumerate(ns):
        ref = lr.level(x[b, :n], sr, -23.0, 1.0)
        nb = 0 if n == 0 else (1 if n < 5 * H else 2)
        assert blocks[b, 0] == nb == ref['blocks'][0], (n, blocks[b])
        assert not bits(out[b, n:]).any() and not pcm[b, n:].any(), n
        if n == 0 or b == len(ns) - 1:
            assert loud[b, 0] == -np.inf and loud[b, 1] == -np.inf and loud[b, 2] == 1.0 and loud[b, 3] == 0.0, (n, loud[b])
            assert tuple(blocks[b]) == (nb, 0, 0, 0)
            assert same_bits(out[b, :n], x[b, :n]) and not pcm[b].any()
            continue
        if n < 4 * H:   # the one-block rule: the mean square of all n_b samples
            y = lr.k_filter(x[b, :n], sr)
            assert abs(loud[b, 0] - lr.lufs(float(np.sum(y * y) / n))) <= BAR and loud[b, 0] == loud[b, 1], (n, loud[b])
        _compare('n_b = %d' % n, loud[b], blocks[b], ref)
        assert same_bits(out[b, :n], x[b, :n] * loud[b, 2])
        assert abs(20 * math.log10(loud[b, 2]) - 20 * math.log10(ref['g'])) <= BAR and blocks[b, 3] == ref['limited'], (n, loud[b], ref['g'])


# ---- gain ----------------------------------------------------------------------------------------------------------------------
def _gain_input():
    L = 30001   # (odd: the rows of out and pcm start at every alignment)
    rng = np.random.default_rng(9)
    x = np.stack([0.02 * rng.standard_normal(L), 0.3 * rng.standard_normal(L), wr.burst(L, 3000, 25000, 1e-5), 0.02 * rng.standard_normal(L),
                  np.zeros(L)]).astype(np.float32)
    x[3, 12345] = -0.9   # one large sample: the ceiling binds
    return x


def test_gain_and_pcm_rule(built_lib):
    """out = x g bit for bit with g read from loud; pcm bit for bit the NumPy-fp32 restatement of step 5; peak_out exact; a second,
    measure-only call on out reads the target within the bar where the ceiling did not bind; the row with one large sample takes the
    limited branch; the all-zero row passes unchanged; out aliasing wave gives the bits of the separate buffer"""
    target, ceiling = -20.0, 0.5
    x = _gain_input()
    out, pcm, loud, blocks = _loud(built_lib, x, target=target, ceiling=ceiling)
    c32 = float(np.float32(ceiling))
    for b in range(len(x)):
        want_out, want_pcm = lr.pcm_fp32(x[b], loud[b, 2])
        assert same_bits(out[b], want_out), b
        assert same_bits(pcm[b], want_pcm), b
        assert loud[b, 3] == np.abs(out[b]).max(), b
        ref = lr.level(x[b], 16000, target, ceiling)
        print('  row %d: I %.3f, g %.5f (fp64 %.5f), peak_out %.5f, limited %d' % (b, loud[b, 0], loud[b, 2], ref['g'], loud[b, 3], blocks[b, 3]))
        assert blocks[b, 3] == ref['limited']
    assert blocks[:, 3].tolist() == [0, 0, 0, 1, 0]
    assert loud[3, 3] <= c32 * (1 + 2.0 ** -23) and loud[3, 0] + 20 * math.log10(loud[3, 2]) < target
    assert loud[3, 2] == np.float32(ceiling) / np.float32(0.9)                       # one IEEE fp32 division
    assert loud[4, 0] == -np.inf and loud[4, 2] == 1.0 and not bits(out[4]).any() and not pcm[4].any()
    assert loud[0, 2] > 1.0 > loud[1, 2]                                              # (one row is raised, one lowered)
    _, _, again, _ = _loud(built_lib, out)
    for b in (0, 1, 2):
        print('  row %d measured again: %.7f LUFS (target %g)' % (b, again[b, 0], target))
        assert abs(again[b, 0] - target) <= BAR, (b, again[b, 0])
    a_out, a_pcm, a_loud, a_blocks = _loud(built_lib, x, target=target, ceiling=ceiling, alias=True)
    assert same_bits(a_out, out) and same_bits(a_pcm, pcm) and same_bits(a_loud, loud) and np.array_equal(a_blocks, blocks)
    # one output at a time
    o_only = _loud(built_lib, x, target=target, ceiling=ceiling, want_pcm=False)
    p_only = _loud(built_lib, x, target=target, ceiling=ceiling, want_out=False)
    assert same_bits(o_only[0], out) and same_bits(p_only[1], pcm) and same_bits(o_only[2], loud) and same_bits(p_only[2], loud)


# ---- rows, determinism, poison ------------------------------------------------------------------------------------------------
ROWS_N = [L_FULL, 0, 1, 59700, 12345]


def _rows_input():
    x = np.stack([wr.burst(L_FULL, 20011, 70003, 1e-5), wr.family('noise'), wr.family('bursts'), wr.burst(L_FULL, 8000, 59700, 3e-6),
                  wr.family('same_sign')])
    xin = x.copy()
    for b, n in enumerate(ROWS_N):
        xin[b, n:] = np.nan
    return x, xin


def test_rows_are_the_call_on_each_row_alone(built_lib):
    """B = 5, L = 107,700, samples = [L, 0, 1, 59700, 12345], NaN behind each n_b: row b is bit-identical to its own B = 1,
    L = n_b call on a contiguous copy, for out, pcm, loud and blocks"""
    x, xin = _rows_input()
    out, pcm, loud, blocks = _loud(built_lib, xin, ROWS_N, target=-23.0, ceiling=0.9)
    assert np.isfinite(out).all()
    for b, n in enumerate(ROWS_N):
        assert not bits(out[b, n:]).any() and not pcm[b, n:].any()
        if n == 0:
            assert loud[b].tolist() == [-np.inf, -np.inf, 1.0, 0.0] and blocks[b].tolist() == [0, 0, 0, 0]
            continue
        o1, p1, l1, b1 = _loud(built_lib, np.ascontiguousarray(x[b:b + 1, :n]), None, target=-23.0, ceiling=0.9)
        assert same_bits(loud[b:b + 1], l1) and np.array_equal(blocks[b:b + 1], b1), (b, loud[b], l1)
        assert same_bits(out[b, :n], o1[0]) and same_bits(pcm[b, :n], p1[0]), b


def test_same_arguments_same_bits_and_poison_changes_nothing(built_lib):
    """two calls give the same bits; a NaN / all-ones / noise workspace and output fill give the bits of the zero-filled call"""
    x, xin = _rows_input()
    ref = _loud(built_lib, xin, ROWS_N, target=-23.0, ceiling=0.9, fill='zeros')
    for fill in ('zeros', 'qnan', 'ones', 'noise'):
        got = _loud(built_lib, xin, ROWS_N, target=-23.0, ceiling=0.9, fill=fill)
        for name, r, g in zip(('out', 'pcm', 'loud', 'blocks'), ref, got):
            assert r.dtype == g.dtype and np.array_equal(r.view(np.uint8), g.view(np.uint8)), (fill, name)
    m_ref = _loud(built_lib, xin, ROWS_N, fill='zeros')
    m_got = _loud(built_lib, xin, ROWS_N, fill='noise')
    assert same_bits(m_ref[2], m_got[2]) and np.array_equal(m_ref[3], m_got[3])
    assert same_bits(m_ref[2][:, :2], ref[2][:, :2]) and np.array_equal(m_ref[3][:, :3], ref[3][:, :3])   # the readings do not depend on the gain


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_bad_arguments_enqueue_nothing(built_lib):
    """every TACO_EINVAL case returns before a launch: the outputs and the workspace keep their sentinel; the error string names
    wave_loudness; the good arguments run with every nullable argument NULL in turn"""
    lib = built_lib
    B, L = 2, 5000
    x = dev(np.stack([wr.burst(L, 1200, 3100, 1e-5), wr.family('noise', L)]))
    sm = dev([L, 3000], torch.int32)
    G = Guarded({'out': ((B, L), torch.float32, 7.0), 'pcm': ((B, L), torch.int16, 7.0), 'loud': ((B, 4), torch.float32, 7.0),
                 'blocks': ((B, 4), torch.int32, 7.0), 'work': ((lib.wave_loudness_workspace_floats(B, L, 16000),), torch.float32, 7.0)})
    fn = C.CDLL(lib.LIB_PATH).taco_wave_loudness
    fn.restype, fn.argtypes = lib.EXPORTS['taco_wave_loudness']
    good = dict(wave=lib.ptr(x), samples=lib.ptr(sm), sr=16000, target=-23.0, ceiling=0.9, out=lib.ptr(G['out']), pcm=lib.ptr(G['pcm']),
                loud=lib.ptr(G['loud']), blocks=lib.ptr(G['blocks']), work=lib.ptr(G['work']), B=B, L=L)
    order = ('wave', 'samples', 'sr', 'target', 'ceiling', 'out', 'pcm', 'loud', 'blocks', 'work', 'B', 'L')
    cases = [{'wave': None}, {'loud': None}, {'blocks': None}, {'work': None}, {'B': 0}, {'B': -1}, {'L': 0}, {'L': -5},
             {'sr': 7999}, {'sr': 16005}, {'sr': 48010}, {'sr': 0},
             {'target': -70.5}, {'target': 0.5}, {'target': float('nan')}, {'target': float('-inf')},
             {'ceiling': 0.0}, {'ceiling': -0.5}, {'ceiling': 1.5}, {'ceiling': float('nan')}, {'ceiling': float('inf')},
             {'target': 5.0, 'pcm': None}, {'ceiling': 2.0, 'out': None}]
    everything = {k: torch.ones(G[k].shape, dtype=torch.bool, device='cuda') for k in ('out', 'pcm', 'loud', 'blocks', 'work')}
    for change in cases:
        for samples in (good['samples'], None):
            a = dict(good, samples=samples)
            a.update(change)
            lib.wave_loudness_workspace_floats(B, L, 16000)   # (a successful call in between: the string below is this refusal's)
            rc = fn(*[a[k] for k in order], lib.stream_ptr())
            torch.cuda.synchronize()
            msg = lib.last_error()
            print('  %r, samples %s: rc %d, %s' % (change, 'given' if samples else 'NULL', rc, msg))
            assert rc == -1, (change, rc)
            assert 'wave_loudness' in msg
            for name, m in everything.items():
                assert G.margin_intact(name, m), '%s was written although %r is refused' % (name, change)
    G.check()
    # and the good arguments do run, with every nullable argument NULL in turn; a measure-only call looks at neither target nor ceiling
    for null, extra in (((), {}), (('samples',), {}), (('out',), {}), (('pcm',), {}), (('samples', 'pcm'), {}),
                        (('out', 'pcm'), {'target': float('nan'), 'ceiling': -1.0})):
        a = dict(good, **extra)
        for k in null:
            a[k] = None
        G.refill('out', 'pcm', 'loud', 'blocks', 'work')
        assert fn(*[a[k] for k in order], lib.stream_ptr()) == 0, null
        torch.cuda.synchronize()
        G.check()
        for k in ('out', 'pcm'):
            if k in null:
                assert G.margin_intact(k, everything[k])
            else:
                assert not bool(torch.isnan(G[k].float()).any()) and not G.margin_intact(k, everything[k])
        assert bool(torch.isfinite(G['loud']).all()) and bool((G['blocks'][:, 0] > 0).all())
        if 'out' in null and 'pcm' in null:
            assert G['loud'][:, 2].tolist() == [1.0, 1.0] and G['blocks'][:, 3].tolist() == [0, 0]


def test_graph_replay_follows_the_device_samples(built_lib):
    """one capture on a side stream; three replays under different `samples` equal the eager calls"""
    B, L = 3, 9000
    x = dev(np.stack([wr.burst(L, 2000, 7000, 1e-5), wr.family('noise', L), wr.family('bursts', L)]))
    first, second, third = [L, 4500, 0], [700, L, 2049], [6400, 1, 8999]
    samples = dev(first, torch.int32)
    G = Guarded({'out': ((B, L), torch.float32, 'qnan'), 'pcm': ((B, L), torch.int16, 'ones'), 'loud': ((B, 4), torch.float32, 'qnan'),
                 'blocks': ((B, 4), torch.int32, 'qnan'),
                 'work': ((built_lib.wave_loudness_workspace_floats(B, L, 16000),), torch.float32, 'qnan')})
    call = lambda: built_lib.wave_loudness(x, samples, target=-23.0, ceiling=0.9, out=G['out'], pcm=G['pcm'], loud=G['loud'],  # noqa: E731
                                           blocks=G['blocks'], work=G['work'])
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            call()
    torch.cuda.synchronize()
    for sm in (first, second, third):
        samples.copy_(dev(sm, torch.int32))
        G.refill('out', 'pcm', 'loud', 'blocks', 'work')
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        G.check('out', 'loud', 'blocks')
        want = _loud(built_lib, x, sm, target=-23.0, ceiling=0.9)
        for name, w in zip(('out', 'pcm', 'loud', 'blocks'), want):
            got = G[name].cpu().numpy()
            assert np.array_equal(got.view(np.uint8), w.view(np.uint8)), 'replay with samples %s differs from the eager call in %s' % (sm, name)


# ---- host layers ----------------------------------------------------------------------------------------------------------------
def test_level_waveform_forms_the_samples_on_the_device(built_lib):
    from tacotron_amd.griffinlim import level_waveform
    L = 9000
    x = dev(np.stack([wr.burst(L, 1500, 5200, 1e-5), wr.family('noise', L), wr.family('bursts', L), wr.family('sine_dc', L)]))
    bounds = dev([[512, 6000], [0, L], [100, 100], [0, 1]], torch.int32)
    n = [5488, L, 0, 1]
    ceiling = 10.0 ** (-1.0 / 20.0)
    ref = built_lib.wave_loudness(x, dev(n, torch.int32), sr=16000, target=-23.0, ceiling=ceiling)
    for got in (level_waveform(x, bounds=bounds), level_waveform(x, total=dev(n, torch.int32))):
        torch.cuda.synchronize()
        for g, w in zip(got, ref):
            assert torch.equal(g.view(torch.int32) if g.dtype == torch.float32 else g, w.view(torch.int32) if w.dtype == torch.float32 else w)
    full = level_waveform(x, target=-16.0, ceiling_db=-3.0, want_out=False)
    want = built_lib.wave_loudness(x, None, target=-16.0, ceiling=10.0 ** (-3.0 / 20.0), want_out=False)
    assert full[0] is None and torch.equal(full[1], want[1]) and torch.equal(full[3], want[3])
    measured = level_waveform(x, bounds=bounds, target=None)
    assert measured[0] is None and measured[1] is None and torch.equal(measured[3][:, :3], ref[3][:, :3])


RULE = dict(end_offset=200, hold=1, min_steps=5)   # target 0: every row stops after step 4 -> len_b = 8
LONG = ('the first sentence of this prompt is long enough to fill a good part of one piece on its own, and it ends here. '
        'the second one has no full stop for a long while, only a comma after a run of words that goes on and on and on, '
        'and then more words that follow the comma until the line has well over three hundred characters in it.\n')


def _raises(*a, **k):
    raise AssertionError('lib.wave_loudness reached without --loudness')


def test_driver_levels_on_the_device(built_lib, tmp_path, monkeypatch, capsys):
    """test() with loudness -23 writes wavs whose frames are the device's pcm and _loud.npy; it combines with stop, vocode_lengths
    and long (where the joined prompt is levelled once); without the option the driver never reaches the entry point and its
    spectrogram and alignment files are the same bytes"""
    from tacotron_amd import test as drv
    from tacotron_amd.config import Config
    prompts = ['hello world.\n', 'a somewhat longer prompt, with punctuation!\n', 'short\n']

    def cfg():
        c = Config()
        c.data_path = str(tmp_path / 'no_data') + '/'
        c.max_decode_iter = 16
        return c

    seen = []
    real = built_lib.wave_loudness

    def spy(*a, **k):
        r = real(*a, **k)
        seen.append((r[1].cpu().numpy(), r[2].cpu().numpy(), r[3].cpu().numpy(), None if a[1] is None else a[1].cpu().numpy(), k))
        return r

    a = drv.parse_args(['--loudness', '-23'])
    monkeypatch.setattr(built_lib, 'wave_loudness', spy)
    r = cfg().r
    L = 300 * (16 * r - 1)
    lev, plain = tmp_path / 'lev', tmp_path / 'plain'
    assert drv.test(cfg(), prompts, out_dir=str(lev), n_iter=2, loudness=a.loudness, peak_db=a.peak_db) == 3
    assert len(seen) == 1 and seen[0][3].tolist() == [L] * 3
    assert seen[0][4]['target'] == -23.0 and abs(seen[0][4]['ceiling'] - 10 ** (-1 / 20)) < 1e-12
    pcm, loud, blocks = seen[0][:3]
    printed = capsys.readouterr().out
    for i in range(3):
        row = np.load(lev / ('prompt_%03d_loud.npy' % i))
        assert row.dtype == np.float64 and row.tolist() == loud[i].astype(np.float64).tolist() + blocks[i].astype(np.float64).tolist()
        assert np.load(lev / ('prompt_%03d_trim.npy' % i)).tolist() == [0, L]
        assert drv.loud_line('prompt %d' % i, row, -1.0) in printed
        with wavefile.open(str(lev / ('prompt_%03d.wav' % i))) as f:
            assert f.getnframes() == L and f.getframerate() == 16000 and f.getsampwidth() == 2 and f.getnchannels() == 1
            assert f.readframes(L) == pcm[i].astype('<i2').tobytes()
        if np.isfinite(row[0]) and not row[7]:
            assert abs(row[0] + 20 * math.log10(row[2]) - (-23.0)) < 1e-4
    # with stop, vocode_lengths, de-emphasis and a ceiling: every row over the samples of its own 8 r frames
    rule = built_lib.TacoStopRule(**RULE)
    del seen[:]
    both = tmp_path / 'both'
    assert drv.test(cfg(), prompts, out_dir=str(both), n_iter=3, stop=rule, vocode_lengths=True, gl_momentum=0.99, deemphasis=0.9,
                    loudness=-30.0, peak_db=-6.0) == 3
    n = 300 * (8 * r - 1)
    assert len(seen) == 1 and seen[0][3].tolist() == [n] * 3 and abs(seen[0][4]['ceiling'] - 10 ** (-6 / 20)) < 1e-12
    for i in range(3):
        assert np.load(both / ('prompt_%03d_trim.npy' % i)).tolist() == [0, n]
        row = np.load(both / ('prompt_%03d_loud.npy' % i))
        assert row[3] <= 10 ** (-6 / 20) * (1 + 2.0 ** -22)
        with wavefile.open(str(both / ('prompt_%03d.wav' % i))) as f:
            assert f.getnframes() == n and f.readframes(n) == seen[0][0][i, :n].astype('<i2').tobytes()
    # with long: the JOINED prompts are levelled, once per group
    del seen[:]
    joined = tmp_path / 'joined'
    assert drv.test(cfg(), prompts[:2] + [LONG], out_dir=str(joined), n_iter=2, stop=rule, long=True, loudness=-23.0) == 3
    assert len(seen) == 1 and seen[0][0].shape[0] == 3
    total = seen[0][3]
    pieces = np.load(joined / 'prompt_002_pieces.npy')
    assert total[2] == pieces[-1, 0] + pieces[-1, 1] and total[0] == n
    for i in range(3):
        row = np.load(joined / ('prompt_%03d_loud.npy' % i))
        assert row.tolist() == seen[0][1][i].astype(np.float64).tolist() + seen[0][2][i].astype(np.float64).tolist()
        with wavefile.open(str(joined / ('prompt_%03d.wav' % i))) as f:
            assert f.getnframes() == total[i] and f.readframes(int(total[i])) == seen[0][0][i, :total[i]].astype('<i2').tobytes()
    assert not list(joined.glob('prompt_002_k*_loud.npy'))
    # without the option: the entry point is never reached, and spectrogram / alignment files are those of the levelled run
    monkeypatch.setattr(built_lib, 'wave_loudness', _raises)
    assert drv.test(cfg(), prompts, out_dir=str(plain), n_iter=2) == 3
    assert not list(plain.glob('*_loud.npy')) and not list(plain.glob('*_trim.npy'))
    for i in range(3):
        for kind in ('spec', 'align'):
            name = 'prompt_%03d_%s.npy' % (i, kind)
            assert open(lev / name, 'rb').read() == open(plain / name, 'rb').read(), name
    with pytest.raises(AssertionError):
        drv.test(cfg(), prompts, out_dir=str(tmp_path / 'x'), n_iter=2, loudness=-23.0)
