"""GPU: taco_wave_join (include/taco_hip.h) through the C ABI -- out, pcm, offsets, total and peak bit for bit against the NumPy
restatement (tests/join_ref.py) on the smallest shapes at which the kernels can go wrong (a full-length, an empty, a shorter-than-two-
ramps and a one-sample piece, a prompt without pieces, an odd Lj, an offset that is no multiple of 4, a piece across a tile edge, rows
and pointers off their vector alignment, a truncating Lj, more pieces per prompt than one scan chunk holds), the per-prompt contract,
determinism, poisoned buffers between guard bands, the PCM rule, every TACO_EINVAL case, and the driver's --long."""
import ctypes as C
import functools
import wave as wavefile

import numpy as np
import pytest
import torch

from tests import join_ref as jr
from tests.poison import Guarded, untouched

pytestmark = pytest.mark.gpu

CORE = jr.CORE


def dev(x, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(x), dtype=dtype, device='cuda')


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({2: np.uint16, 4: np.uint32}[x.dtype.itemsize])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


NAMES = ('out', 'pcm', 'offsets', 'total', 'peak')


def _join(lib, x, bounds, first, gap, fade, Lj, want_out=True, want_pcm=True, fill='qnan', L=None, skew=0):
    """lib.wave_join into poisoned buffers between guard bands (the workspace poisoned as well); every element of every output must
    have been written.  x (N, pitch): the pieces are its first L columns.  skew = 1: out starts one float behind a 16-byte boundary
    and pcm one sample behind an 8-byte boundary; the element in front of each must keep its fill.
    -> (out, pcm, offsets, total, peak) as NumPy arrays (None for an output not asked for)"""
    xt = x if torch.is_tensor(x) else dev(x)
    N = xt.shape[0]
    L = xt.shape[1] if L is None else L
    P = len(first) - 1
    spec = {'offsets': ((N,), torch.int32, fill), 'total': ((P,), torch.int32, fill), 'peak': ((P,), torch.float32, fill),
            'work': ((lib.wave_join_workspace_bytes(N, P, Lj),), torch.uint8, fill)}
    if want_out:
        spec['out'] = ((P * Lj + skew,), torch.float32, fill)
    if want_pcm:
        spec['pcm'] = ((P * Lj + skew,), torch.int16, fill)
    G = Guarded(spec)
    out = G['out'][skew:].view(P, Lj) if want_out else None
    pcm = G['pcm'][skew:].view(P, Lj) if want_pcm else None
    r = lib.wave_join(xt[:, :L], bounds if torch.is_tensor(bounds) else dev(bounds, torch.int32), first, gap, fade=fade, Lj=Lj,
                      want_out=want_out, want_pcm=want_pcm, out=out, pcm=pcm, offsets=G['offsets'], total=G['total'], peak=G['peak'],
                      work=G['work'])
    torch.cuda.synchronize()
    assert r[2] is G['offsets'] and r[3] is G['total'] and r[4] is G['peak']
    assert (r[0] is None) == (not want_out) and (r[1] is None) == (not want_pcm)
    G.check()   # the guard bands
    if fill != 'zeros':   # (every int16 value is a legal sample: that pcm is written everywhere is shown by the poison test)
        for name in ('out', 'offsets', 'total', 'peak'):
            if name in spec:
                left = untouched(G[name], G.marks[name])[skew if name == 'out' else 0:]
                assert not bool(left.any()), '%d element(s) of %r still hold the fill' % (int(left.sum()), name)
    for name in ('out', 'pcm'):
        if skew and name in spec:
            assert bool(untouched(G[name], G.marks[name])[0]), 'the element in front of %s was written' % name
    return tuple(None if t is None else t.cpu().numpy() for t in r)


@functools.lru_cache(maxsize=None)
def _core(fade=CORE['fade'], Lj=CORE['Lj'], pitch=CORE['L'], scale=0.3):
    """the small case and its restatement, computed once: (x (N, pitch), bounds, reference outputs)"""
    x, bounds = jr.core_pieces(scale=scale, pitch=pitch)
    ref = jr.join(x[:, :CORE['L']], bounds, CORE['first'], CORE['gap'], fade, Lj)
    for a in (x, bounds) + ref:
        a.setflags(write=False)
    return x, bounds, ref


def _equal(got, ref, what=''):
    for name, g, r in zip(NAMES, got, ref):
        if g is not None:
            assert same_bits(g, r), '%s differs from the restatement %s' % (name, what)


# ---- the core case -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['both', 'out_only', 'pcm_only', 'pitch_and_skew'])
def test_core_case_equals_the_restatement(built_lib, mode):
    """N = 5, P = 3, L = 2500, lens [2500, 0, 7, 1, 1300], first [0, 3, 3, 5], gap [100, 0, 5, 33, 9], fade 16, Lj = 4001"""
    pitch = CORE['L'] + 3 if mode == 'pitch_and_skew' else CORE['L']
    x, bounds, ref = _core(pitch=pitch)
    assert ref[2].tolist() == [0, 2600, 2600, 0, 34] and ref[3].tolist() == [2607, 0, 1334]
    got = _join(built_lib, x, bounds, CORE['first'], CORE['gap'], CORE['fade'], CORE['Lj'], want_out=mode != 'pcm_only',
                want_pcm=mode != 'out_only', L=CORE['L'], skew=int(mode == 'pitch_and_skew'),
                fill='ones' if mode == 'pitch_and_skew' else 'qnan')   # (all-ones: the int16 in front of pcm is -1, not a silent 0)
    assert (got[0] is None) == (mode == 'pcm_only') and (got[1] is None) == (mode == 'out_only')
    _equal(got, ref, mode)
    if got[0] is not None:
        assert np.isfinite(got[0]).all()
        for p in range(CORE['P']):
            assert got[4][p] == np.abs(got[0][p]).max()


def test_fade_0_copies_every_sample(built_lib):
    x, bounds, ref = _core(fade=0)
    got = _join(built_lib, x, bounds, CORE['first'], CORE['gap'], 0, CORE['Lj'])
    _equal(got, ref)
    off, lens = got[2], CORE['lens']
    for i, p in enumerate([0, 0, 0, 2, 2]):
        assert same_bits(got[0][p, off[i]:off[i] + lens[i]], x[i, :lens[i]]), i


def test_a_short_lj_truncates(built_lib):
    x, bounds, ref = _core(Lj=2550)
    got = _join(built_lib, x, bounds, CORE['first'], CORE['gap'], CORE['fade'], 2550)
    assert got[3].tolist() == [2550, 0, 1334] and got[2].tolist() == [0, 2550, 2550, 0, 34]
    _equal(got, ref)


@pytest.mark.parametrize('N', [70, 300])
def test_many_pieces_in_one_prompt(built_lib, N):
    """pieces of 1..64 samples in one prompt, L = 64: no cap on the pieces per prompt (300: more than one chunk of the offsets scan)"""
    rng = np.random.default_rng(N)
    L = 64
    lens = [int(v) for v in (np.arange(N) * 37) % 64 + 1]
    x, bounds = jr.core_pieces(scale=0.2, seed=N, L=L, lens=lens)
    gap = [int(v) for v in rng.integers(0, 9, size=N)]
    for first in ([0, N], [0, N - 3, N - 3, N]):
        Lj = sum(lens) + sum(gap) + 5
        ref = jr.join(x, bounds, first, gap, 4, Lj)
        assert ref[3][0] > 64 * 20
        _equal(_join(built_lib, x, bounds, first, gap, 4, Lj), ref, 'first %r' % (first,))


def test_default_lj_cuts_nothing(built_lib):
    x, bounds, _ = _core()
    out, pcm, offsets, total, peak = built_lib.wave_join(dev(x), dev(bounds, torch.int32), CORE['first'], CORE['gap'], fade=CORE['fade'])
    torch.cuda.synchronize()
    assert out.shape == pcm.shape == (3, 7600) and out.shape[1] % 8 == 0 and 3 * CORE['L'] + 100 <= out.shape[1]
    ref = jr.join(x, bounds, CORE['first'], CORE['gap'], CORE['fade'], 7600)
    _equal([t.cpu().numpy() for t in (out, pcm, offsets, total, peak)], ref)


# ---- prompts, determinism, poison ----------------------------------------------------------------------------------------------------
def test_prompts_are_the_call_on_each_prompt_alone(built_lib):
    x, bounds, _ = _core()
    first, gap = CORE['first'], CORE['gap']
    whole = _join(built_lib, x, bounds, first, gap, CORE['fade'], CORE['Lj'])
    for p in range(CORE['P']):
        lo, hi = first[p], first[p + 1]
        if lo == hi:
            assert not bits(whole[0][p]).any() and not whole[1][p].any() and whole[3][p] == 0 and whole[4][p] == 0
            continue
        alone = _join(built_lib, x[lo:hi], bounds[lo:hi], [0, hi - lo], gap[lo:hi], CORE['fade'], CORE['Lj'])
        assert same_bits(whole[0][p], alone[0][0]) and same_bits(whole[1][p], alone[1][0]), p
        assert same_bits(whole[2][lo:hi], alone[2]) and whole[3][p] == alone[3][0] and same_bits(whole[4][p:p + 1], alone[4])


def test_same_arguments_same_bits_and_poison_changes_nothing(built_lib):
    """two calls give the same bits; NaN behind every len_i (the input has it), and a NaN / all-ones / noise / zero fill of the
    workspace and the outputs, end in the bits of the restatement"""
    x, bounds, ref = _core()
    assert all(np.isnan(x[i, n:]).all() for i, n in enumerate(CORE['lens']))
    clean = x.copy()
    clean[np.isnan(clean)] = 0.0
    for fill in ('zeros', 'qnan', 'qnan', 'ones', 'noise'):
        for src in (x, clean):
            _equal(_join(built_lib, src, bounds, CORE['first'], CORE['gap'], CORE['fade'], CORE['Lj'], fill=fill), ref, fill)
        for kw in (dict(want_out=False), dict(want_pcm=False)):
            _equal(_join(built_lib, x, bounds, CORE['first'], CORE['gap'], CORE['fade'], CORE['Lj'], fill=fill, **kw), ref, fill)


def test_pcm_rule(built_lib):
    """wave_finish's rule with the PROMPT'S peak: one prompt above full scale (scaled by its peak), one below (unscaled)"""
    L = 3000
    rng = np.random.default_rng(8)
    x = rng.standard_normal((4, L)).astype(np.float32) * np.array([[2.0], [0.05], [0.1], [0.2]], np.float32)
    bounds = np.array([[0, L], [0, 2000], [0, L], [100, 1100]], np.int32)
    first, gap = [0, 2, 4], [160, 0, 7, 0]
    Lj = 2 * L + 160
    ref = jr.join(x, bounds, first, gap, 80, Lj)
    out, pcm, offsets, total, peak = _join(built_lib, x, bounds, first, gap, 80, Lj)
    _equal((out, pcm, offsets, total, peak), ref)
    assert peak[0] > 1.0 > peak[1] > 0 and total.tolist() == [L + 160 + 2000, L + 7 + 1000]
    assert np.abs(pcm[0].astype(np.int32)).max() == 32767 and np.abs(pcm[1].astype(np.int32)).max() < 32767 * 0.9
    # the quiet piece of the loud prompt is scaled by the prompt's peak, not by its own
    seg = slice(int(offsets[1]) + 80, int(offsets[1]) + 2000)
    assert np.array_equal(pcm[0, seg], np.trunc((out[0, seg] / peak[0]) * np.float32(32767.0)).astype(np.int16))
    assert np.array_equal(pcm[1], np.trunc(out[1] * np.float32(32767.0)).astype(np.int16))


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_enqueue_nothing(built_lib):
    """every TACO_EINVAL case returns before anything is enqueued: the outputs and the workspace keep their sentinel"""
    lib = built_lib
    N, P, L, Lj = CORE['N'], CORE['P'], CORE['L'], CORE['Lj']
    x, bounds, _ = _core()
    # (pieces in the arena as well: `out` overlapping them is one of the cases)
    G = Guarded({'pieces': ((N, L), torch.float32, 7.0), 'out': ((P, Lj), torch.float32, 7.0), 'pcm': ((P, Lj), torch.int16, 7.0),
                 'offsets': ((N,), torch.int32, 7.0), 'total': ((P,), torch.int32, 7.0), 'peak': ((P,), torch.float32, 7.0),
                 'work': ((lib.wave_join_workspace_bytes(N, P, Lj),), torch.uint8, 7.0)})
    bd = dev(bounds, torch.int32)
    fn = C.CDLL(lib.LIB_PATH).taco_wave_join
    fn.restype, fn.argtypes = lib.EXPORTS['taco_wave_join']
    i32 = lambda v: (C.c_int32 * len(v))(*v)   # noqa: E731
    pieces = G['pieces'].data_ptr()
    good = dict(pieces=C.c_void_p(pieces), pitch=L, bounds=lib.ptr(bd), first=i32(CORE['first']), gap=i32(CORE['gap']), fade=16,
                out=lib.ptr(G['out']), pcm=lib.ptr(G['pcm']), offsets=lib.ptr(G['offsets']), total=lib.ptr(G['total']),
                peak=lib.ptr(G['peak']), work=lib.ptr(G['work']), N=N, P=P, L=L, Lj=Lj)
    order = ('pieces', 'pitch', 'bounds', 'first', 'gap', 'fade', 'out', 'pcm', 'offsets', 'total', 'peak', 'work', 'N', 'P', 'L', 'Lj')
    cases = [{'pieces': None}, {'bounds': None}, {'first': None}, {'gap': None}, {'offsets': None}, {'total': None}, {'peak': None},
             {'work': None}, {'out': None, 'pcm': None},
             {'out': C.c_void_p(pieces)}, {'out': C.c_void_p(pieces + 4 * (N * L - 1))}, {'out': C.c_void_p(pieces - 4 * (P * Lj - 1))},
             {'N': 0}, {'N': -1}, {'P': 0}, {'P': -2}, {'L': 0}, {'L': -5}, {'Lj': 0}, {'Lj': -1}, {'pitch': L - 1}, {'pitch': 0},
             {'pitch': -L}, {'fade': -1},
             {'first': i32([1, 3, 3, 5])}, {'first': i32([0, 3, 2, 5])}, {'first': i32([0, 3, 3, 4])}, {'first': i32([0, 3, 3, 6])},
             {'first': i32([0, 6, 3, 5])}, {'gap': i32([100, 0, 5, 33, -1])}, {'gap': i32([-100, 0, 5, 33, 9])}]
    everything = {k: torch.ones(G[k].shape, dtype=torch.bool, device='cuda') for k in ('out', 'pcm', 'offsets', 'total', 'peak', 'work')}
    for change in cases:
        a = dict(good)
        a.update(change)
        lib.wave_join_workspace_bytes(N, P, Lj)   # (a successful call in between: the string below is this refusal's)
        rc = fn(*[a[k] for k in order], lib.stream_ptr())
        torch.cuda.synchronize()
        msg = lib.last_error()
        print('  %r: rc %d, %s' % (sorted(change), rc, msg))
        assert rc == -1, (change, rc)
        assert 'wave_join' in msg
        for name, m in everything.items():
            assert G.margin_intact(name, m), '%s was written although %r is refused' % (name, change)
    G.check()
    # and the good arguments do run, with every nullable argument NULL in turn
    G['pieces'].copy_(torch.nan_to_num(dev(x)))
    for null in ((), ('out',), ('pcm',)):
        a = dict(good)
        for k in null:
            a[k] = None
        G.refill('out', 'pcm', 'offsets', 'total', 'peak', 'work')
        assert fn(*[a[k] for k in order], lib.stream_ptr()) == 0, null
        torch.cuda.synchronize()
        G.check()
        for k in ('out', 'pcm'):
            assert G.margin_intact(k, everything[k]) == (k in null)
        assert G['total'].cpu().tolist() == [2607, 0, 1334]


# ---- the driver ----------------------------------------------------------------------------------------------------------------------
RULE = dict(end_offset=200, hold=1, min_steps=5)   # target 0: every row stops after step 4 -> len_b = 8

SHORTS = ['hello world.\n', 'a somewhat longer prompt, with punctuation!\n']
LONG = ('the first sentence of this prompt is long enough to fill a good part of one piece on its own, and it ends here. '
        'the second one has no full stop for a long while, only a comma after a run of words that goes on and on and on, '
        'and then more words that follow the comma until the line has well over three hundred characters in it.\n')


def _raises(*a, **k):
    raise AssertionError('lib.wave_join reached without --long')


def test_driver_joins_a_long_prompt_on_the_device(built_lib, tmp_path, monkeypatch):
    """test() with long=True: the long prompt's wav is the restatement's join of what lib.wave_finish wrote for its pieces,
    prompt_NNN_pieces.npy says where they lie, and the short prompts' files are those of a run without `long`"""
    from tacotron_amd import data, test as drv
    from tacotron_amd.config import Config
    pieces = data.split_prompt(LONG)
    kinds = [k for _, k in pieces]
    assert 320 <= len(LONG.strip()) <= 350 and len(pieces) >= 3 and data.SENTENCE in kinds and data.CLAUSE in kinds
    K = len(pieces)

    def cfg():
        c = Config()
        c.data_path = str(tmp_path / 'no_data') + '/'
        c.max_decode_iter = 16
        return c

    seen = []
    real = built_lib.wave_finish

    def spy(*a, **k):
        r = real(*a, **k)
        seen.append((None if r[0] is None else r[0].cpu().numpy(), r[2].cpu().numpy()))
        return r

    a = drv.parse_args(['--stop', '--long'])
    monkeypatch.setattr(built_lib, 'wave_finish', spy)
    rule = built_lib.TacoStopRule(**RULE)
    r = cfg().r
    L = 300 * (16 * r - 1)
    n = 300 * (8 * r - 1)
    joined, plain = tmp_path / 'joined', tmp_path / 'plain'
    assert drv.test(cfg(), SHORTS + [LONG], out_dir=str(joined), n_iter=2, stop=rule, long=a.long) == 3
    assert len(seen) == 1 and seen[0][0].shape == (2 + K, L)      # one batch of 2 + K rows, finished into fp32 rows
    rows, bounds = seen[0]
    assert bounds.tolist() == [[0, n]] * (2 + K)                  # de-emphasis and trim are off: [0, n_b)
    first = [0, 1, 2, 2 + K]
    gap = [0, 0] + [{data.SENTENCE: 4800, data.CLAUSE: 2400}.get(k, 0) for k in kinds]
    Lj = -(-(K * L + sum(gap)) // 8) * 8
    out, pcm, offsets, total, peak = jr.join(rows, bounds, first, gap, 80, Lj)
    assert total[2] == K * n + sum(gap[2:-1])
    with wavefile.open(str(joined / 'prompt_002.wav')) as f:
        assert f.getnframes() == total[2] and f.getframerate() == 16000 and f.getsampwidth() == 2 and f.getnchannels() == 1
        assert f.readframes(int(total[2])) == pcm[2, :total[2]].astype('<i2').tobytes()
    table = np.load(joined / 'prompt_002_pieces.npy')
    assert table.dtype == np.int32 and table.tolist() == [[int(offsets[2 + k]), n, 0 if k == K - 1 else gap[2 + k], kinds[k]]
                                                          for k in range(K)]
    for k in range(K):
        for kind, shape0 in (('spec', 8 * r), ('align', 8)):
            assert np.load(joined / ('prompt_002_k%02d_%s.npy' % (k, kind))).shape[0] == shape0
        assert np.load(joined / ('prompt_002_k%02d_len.npy' % k)) == 8
        assert np.load(joined / ('prompt_002_k%02d_trim.npy' % k)).tolist() == [0, n]
    assert not list(joined.glob('prompt_002_spec.npy')) and not list(joined.glob('prompt_00[01]_k*'))
    assert not list(joined.glob('prompt_00[01]_pieces.npy'))
    # the same short prompts with a stop rule and finishing, without `long`: the join is never reached and the files are the same bytes
    monkeypatch.setattr(built_lib, 'wave_join', _raises)
    assert drv.test(cfg(), SHORTS, out_dir=str(plain), n_iter=2, stop=rule, deemphasis=0.0) == 2
    names = sorted(p.name for p in plain.iterdir())
    assert names == sorted('prompt_%03d%s' % (i, s) for i in range(2) for s in ('.wav', '_spec.npy', '_align.npy', '_len.npy', '_trim.npy'))
    for name in names:
        assert open(joined / name, 'rb').read() == open(plain / name, 'rb').read(), name
    with pytest.raises(ValueError):     # and a long line without `long` is refused as before
        drv.test(cfg(), [LONG], out_dir=str(tmp_path / 'x'), n_iter=2, stop=rule, deemphasis=0.0)
    with pytest.raises(AssertionError):
        drv.test(cfg(), SHORTS, out_dir=str(tmp_path / 'y'), n_iter=2, stop=rule, long=True)
