"""GPU: every auxiliary entry point works inside a workspace of EXACTLY the bytes its size function states.

The size function and the entry point of each of these calls read one layout (WsCarver, csrc/common.h).  The other tests let the
wrapper allocate the workspace, and torch rounds an allocation up to 512 bytes, so a layout that walks past its stated size would go
unseen there.  Here each call runs three ways at the smallest shape that uses every array of its layout:
  1. through the wrapper with its default workspace: the reference outputs;
  2. with the workspace carved out of an arena (tests/poison.py) between two other buffers, guard bands of 4096 floats on both
     sides, cut to exactly the stated bytes and poisoned with quiet NaNs, then with finite noise: every output is bit-identical
     to the reference and the bands are intact;
  3. for the three calls that round the base of their workspace up (wave_finish, wave_join, frames_cepstats): the same with the
     view starting 4 (and for the two wave calls 8 and 12) bytes past a 256-byte boundary, still of exactly the stated size; the
     bytes of the buffer on either side of the view hold the guard word and are checked with the bands.
Outputs are handed in zero-filled, so that an element a call documents as untouched compares equal too."""
import numpy as np
import pytest
import torch

from tests import poison

pytestmark = pytest.mark.gpu

GUARD_FLOATS = 4096
DEV = 'cuda'


class Slot:
    """`nbytes` of workspace `offset` bytes into a buffer that sits between two others in one arena"""

    def __init__(self, nbytes, offset=0):
        words = -(-(offset + nbytes) // 4) + (4 if offset else 0)
        self.arena = poison.carve([('front', 64), ('ws', words), ('back', 64)], GUARD_FLOATS, DEV)
        self.lo, self.hi = offset, offset + nbytes
        self.u8 = self.arena.view('ws', torch.uint8)
        self.guard = torch.from_numpy(np.tile(poison._GUARD_BYTES, words).copy()).to(DEV)
        assert self.arena.f32('ws').data_ptr() % 256 == 0

    def fill(self, pattern, seed):
        poison.poison(self.arena.f32('ws'), pattern, seed=seed)
        self.u8[:self.lo] = self.guard[:self.lo]
        self.u8[self.hi:] = self.guard[self.hi:]

    def view(self, dtype):
        return self.u8[self.lo:self.hi].view(dtype)

    def check(self):
        rep = poison.guards_intact(self.arena)
        assert rep, repr(rep)
        assert torch.equal(self.u8[:self.lo], self.guard[:self.lo]), 'bytes in front of the workspace were written'
        assert torch.equal(self.u8[self.hi:], self.guard[self.hi:]), 'bytes behind the workspace were written'


def _bits(t):
    return None if t is None else t.contiguous().view(-1).view(torch.uint8)


def _same(got, ref, what):
    assert len(got) == len(ref), what
    for i, (g, r) in enumerate(zip(got, ref)):
        assert (g is None) == (r is None), (what, i)
        if g is not None:
            assert g.shape == r.shape and g.dtype == r.dtype and torch.equal(_bits(g), _bits(r)), '%s: output %d differs' % (what, i)


def _rand(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def _z(shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype, device=DEV)


def _i32(*v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


# ---- the cases: name -> (bytes of the workspace, its dtype in the wrapper, call(work) -> outputs, base offsets of step 3) --------
def _griffinlim(lib, form):
    B, F, n_iter = 2, 6, 2
    mag = _rand(1, B, 1025, F).abs().to(DEV)
    phase0 = (_rand(2, B, 1025, F) * 3.0).to(DEV)
    frames = _i32(6, 5)
    if form == 'plain':
        return (4 * lib.griffinlim_workspace_floats(B, F), torch.float32,
                lambda w: (lib.griffinlim(mag, phase0, n_iter=n_iter, out=_z((B, 300 * (F - 1))), work=w),), ())
    if form == 'rows':
        return (4 * lib.griffinlim_rows_workspace_floats(B, F), torch.float32,
                lambda w: (lib.griffinlim_rows(mag, frames, seed=3, n_iter=n_iter, out=_z((B, 300 * (F - 1))), work=w),), ())
    return (4 * lib.griffinlim_fast_workspace_floats(B, F), torch.float32,
            lambda w: lib.griffinlim_fast(mag, frames, seed=3, n_iter=n_iter, momentum=0.5, want_conv=True, out=_z((B, 300 * (F - 1))),
                                          conv=_z((B, n_iter + 1)), work=w), ())


def _wave(seed, B, L):
    """rows that are loud in the middle and quiet at both ends (the trim has something to cut), peaks above 0.5"""
    n = torch.arange(L, dtype=torch.float32)
    env = 0.001 + torch.sin(np.pi * (n + 0.5) / L) ** 8
    return (_rand(seed, B, L) * 0.4 * env).to(DEV)


def _wave_finish(lib):
    B, L = 2, 2049   # one sample past a chunk: two chunks per row
    wave, samples = _wave(3, B, L), _i32(L, 1500)
    return (4 * lib.wave_finish_workspace_floats(B, L), torch.float32,
            lambda w: lib.wave_finish(wave, samples, deemphasis=0.97, trim_top_db=20.0, out=_z((B, L)), pcm=_z((B, L), torch.int16),
                                      bounds=_z((B, 2), torch.int32), peak=_z((B,)), work=w), (4, 8, 12))


def _wave_loudness(lib):
    B, L, sr = 2, 2049, 8000
    wave, samples = _wave(4, B, L), _i32(L, 1500)
    return (4 * lib.wave_loudness_workspace_floats(B, L, sr), torch.float32,
            lambda w: lib.wave_loudness(wave, samples, sr=sr, target=-23.0, ceiling=0.9, out=_z((B, L)), pcm=_z((B, L), torch.int16),
                                        loud=_z((B, 4)), blocks=_z((B, 4), torch.int32), work=w), ())


def _wave_limit(lib):
    B, L, W = 2, 2049, 24
    wave0, samples = _wave(5, B, L), _i32(L, 1500)
    assert float(wave0.abs().max()) > 0.5
    window = lib.limit_window(W)

    def call(w):
        wave = wave0.clone()   # out is the wave: the halos are used
        return lib.wave_limit(wave, samples, ceiling=0.5, window=window, out=wave, pcm=_z((B, L), torch.int16), peaks=_z((B, 4)),
                              counts=_z((B, 2), torch.int32), work=w)
    return 4 * lib.wave_limit_workspace_floats(B, L, W), torch.float32, call, ()


def _wave_join(lib):
    N, P, L = 3, 2, 100
    pieces = _rand(6, N, L).mul(0.3).to(DEV)
    bounds = torch.tensor([[0, 100], [5, 90], [0, 50]], dtype=torch.int32, device=DEV)
    first, gap, fade = [0, 2, 3], [10, 0, 0], 4
    Lj = 216
    return (lib.wave_join_workspace_bytes(N, P, Lj), torch.uint8,
            lambda w: lib.wave_join(pieces, bounds, first, gap, fade=fade, Lj=Lj, want_out=False, pcm=_z((P, Lj), torch.int16),
                                    offsets=_z((N,), torch.int32), total=_z((P,), torch.int32), peak=_z((P,)), work=w), (4, 8, 12))


def _phase_estimate(lib, F):
    B = 1
    mag = _rand(7, B, 1025, F).abs().to(DEV)
    return (lib.phase_estimate_workspace_bytes(B, F), torch.uint8,
            lambda w: (lib.phase_estimate(mag, out=_z((B, 1025, F)), workspace=w),), ())


def _frames_cepstats(lib):
    B, C, F, lifter = 2, 17, 33, 8
    mag = (_rand(8, B, C, F).abs() + 0.01).to(DEV)
    frames = _i32(33, 20)
    return (lib.frames_cepstats_workspace_bytes(B, C, F, lifter), torch.uint8,
            lambda w: lib.frames_cepstats(mag, lifter=lifter, frames=frames, out=(_z((B, lifter + 1, 2), torch.float64),
                                                                                 _z((B,), torch.int32)), workspace=w), (4,))


def _f0_viterbi(lib):
    B, F, K, lag_min, lag_max = 2, 33, 3, 40, 60
    L = lag_max - lag_min + 3
    acf = _rand(9, B, L, F).to(DEV)
    frames = _i32(33, 20)
    return (lib.f0_viterbi_workspace_bytes(B, L, F, K), torch.uint8,
            lambda w: lib.f0_viterbi(acf, frames, lag_min=lag_min, lag_max=lag_max, candidates=K, threshold=0.1,
                                     out=(_z((B, F)), _z((B, F)), _z((B, 4), torch.int32), _z((B,))), workspace=w), ())


def _tensor_stats(lib):
    base = _rand(10, 30000).to(DEV)
    plan = lib.tensor_stats_plan([(0, 10), (16, 20000), (25000, 5000)], 30000, DEV)   # the second one: three work items
    assert plan.n == 3 and plan.n_items > plan.n
    NB = 2 * ((lib.STATS_E_HI - lib.STATS_E_LO + 1) << lib.STATS_SUB_BITS) + 1
    return (lib.tensor_stats_workspace_bytes(plan.n, plan.n_items, NB), torch.uint8,
            lambda w: tuple(lib.tensor_stats(base, plan, counts=_z((3, 6), torch.int64), moments=_z((3, 5), torch.float64),
                                             hist=_z((3, NB), torch.int64), work=w)), ())


def _param_ema(lib):
    n = 1025
    ema0, params = _rand(11, n).to(DEV), _rand(12, n).to(DEV)

    def call(w):
        ema = ema0.clone()   # (updated in place)
        return ema, lib.param_ema(ema, params, 0.25, stats=_z((3,), torch.float64), workspace=w)
    return lib.param_ema_workspace_bytes(n), torch.uint8, call, ()


def _audio_features(lib):
    from tacotron_amd import audio
    B, L, r, max_len = 2, 1200, 1, 1200   # the shortest max_len: a multiple of 300 above 1024 with 4 r frames
    wave = _wave(13, B, L)
    basis = torch.from_numpy(audio.mel_basis()).to(DEV)
    Td = ((1 + max_len // 300) // (4 * r)) * 4
    return (lib.audio_features_workspace_bytes(B, L), torch.uint8,
            lambda w: lib.audio_features(wave, [1200, 900], basis, r, max_len, torch.float32,
                                         out=(_z((B, Td, 80 * r)), _z((B, Td, 1025 * r)), _z((B,), torch.int32),
                                              _z((B, 2), torch.int32)), work=w), ())


def _frame_dtw(lib, path):
    B, Fa, Fb, K = 2, 569, 569, 32   # the smallest square shape at K = 32 whose coefficients do not fit LDS
    assert lib.frame_dtw_workspace_bytes(B, Fa, Fb, K) > 0 and lib.frame_dtw_workspace_bytes(B, Fa - 1, Fb - 1, K) == 0
    a, b = _rand(14, B, Fa, K).to(DEV), _rand(15, B, Fb, K).to(DEV)
    na, nb = _i32(569, 300), _i32(500, 569)
    if not path:
        return (lib.frame_dtw_workspace_bytes(B, Fa, Fb, K), torch.uint8,
                lambda w: lib.frame_dtw(a, b, na, nb, cost=_z((B,)), steps=_z((B,), torch.int32), work=w), ())
    P = Fa + Fb - 1
    return (lib.frame_dtw_path_workspace_bytes(B, Fa, Fb, K), torch.uint8,
            lambda w: lib.frame_dtw_path(a, b, na, nb, cost=_z((B,)), steps=_z((B,), torch.int32), path_a=_z((B, P), torch.int32),
                                         path_b=_z((B, P), torch.int32), work=w), ())


def _alignment_path(lib):
    B, Td, Tt = 2, 9, 257   # the narrowest row one wave does not hold
    assert lib.alignment_path_workspace_bytes(B, Td, Tt) > 0 and lib.alignment_path_workspace_bytes(B, Td, Tt - 1) == 0
    al = torch.softmax(_rand(16, B, Td, Tt) * 3.0, dim=-1).to(DEV)
    return (lib.alignment_path_workspace_bytes(B, Td, Tt), torch.uint8,
            lambda w: lib.alignment_path(al, _i32(257, 100), _i32(9, 5), path=_z((B, Td), torch.int32), dur=_z((B, Tt), torch.int32),
                                         counts=_z((B, len(lib.PATH_COUNTS)), torch.int32), mass=_z((B,)), workspace=w), ())


CASES = {
    'griffinlim': lambda lib: _griffinlim(lib, 'plain'),
    'griffinlim_rows': lambda lib: _griffinlim(lib, 'rows'),
    'griffinlim_fast': lambda lib: _griffinlim(lib, 'fast'),
    'wave_finish': _wave_finish,
    'wave_loudness': _wave_loudness,
    'wave_limit': _wave_limit,
    'wave_join': _wave_join,
    'phase_estimate_F5': lambda lib: _phase_estimate(lib, 5),
    'phase_estimate_F33': lambda lib: _phase_estimate(lib, 33),
    'frames_cepstats': _frames_cepstats,
    'f0_viterbi': _f0_viterbi,
    'tensor_stats': _tensor_stats,
    'param_ema': _param_ema,
    'audio_features': _audio_features,
    'frame_dtw': lambda lib: _frame_dtw(lib, False),
    'frame_dtw_path': lambda lib: _frame_dtw(lib, True),
    'alignment_path': _alignment_path,
}
ROUNDED_BASE = ('wave_finish', 'wave_join', 'frames_cepstats')


@pytest.mark.parametrize('name', sorted(CASES))
def test_stated_bytes_are_enough(built_lib, name):
    nbytes, dtype, call, offsets = CASES[name](built_lib)
    assert (len(offsets) > 0) == (name in ROUNDED_BASE)
    assert nbytes > 0 and nbytes % torch.empty((), dtype=dtype).element_size() == 0
    ref = call(None)
    torch.cuda.synchronize()
    for offset in (0,) + tuple(offsets):
        slot = Slot(nbytes, offset)
        for seed, pattern in enumerate(('qnan', 'noise')):
            slot.fill(pattern, seed)
            work = slot.view(dtype)
            assert work.numel() * work.element_size() == nbytes and work.data_ptr() % 256 == offset
            got = call(work)
            torch.cuda.synchronize()
            _same(got, ref, '%s, workspace at +%d filled with %s' % (name, offset, pattern))
            slot.check()
