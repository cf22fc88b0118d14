"""GPU: Griffin-Lim (audio.py:77-97) -- the HIP FFT / overlap-add path against the NumPy restatement of the
librosa algorithm (oracle/griffinlim_numpy.py; PARITY UNPINNED: librosa is absent from this image).

Tolerances (fp32 FFTs vs fp64): one synthesis + analysis pass and the n_iter = 0 / 1 waveforms rel-L2 <= 2e-5; after several rounds
the phase projection is ill-conditioned at near-zero bins, so for n_iter = 50 the test compares the quantity Griffin-Lim
minimises (spectral convergence, audio.py:90-92) instead of samples: within 2 % of the oracle's, and far below the start.

The waveform, Griffin-Lim's workspace and the de-normalised magnitudes are the tests' own buffers, carved from a guarded arena and
filled with NaN before every call (tests/poison.py): afterwards every output element is written and the guard bands are intact."""
import numpy as np
import pytest
import torch

from oracle import griffinlim_numpy as gl
from tests.poison import Guarded
from tests.util import rel_l2

pytestmark = pytest.mark.gpu


def _griffinlim(lib, m, p, n_iter):
    """lib.griffinlim into a poisoned waveform buffer with a poisoned workspace, between guard bands"""
    B, _, F = m.shape
    G = Guarded({'wave': ((B, 300 * (F - 1)), torch.float32, 'qnan'),
                 'work': ((lib.griffinlim_workspace_floats(B, F),), torch.float32, 'qnan')})
    w = lib.griffinlim(m, p, n_iter, out=G['wave'], work=G['work'])
    torch.cuda.synchronize()
    G.check('wave')
    assert bool(torch.isfinite(w).all())
    return w


def _case(F, seed):
    rng = np.random.default_rng(seed)
    # a magnitude matrix that IS the STFT of a signal (so Griffin-Lim can converge), plus noise-floor bins
    y = np.cumsum(rng.standard_normal(300 * (F - 1))) * 0.01 + np.sin(np.arange(300 * (F - 1)) * 0.05)
    mag = np.abs(gl.stft(y)) + 1e-3
    ph = 2 * np.pi * rng.random(mag.shape)
    return mag, ph


@pytest.mark.parametrize('F', [8, 41])
def test_istft_and_one_round_match_oracle(built_lib, F):
    mag, ph = _case(F, 3)
    m = torch.tensor(np.stack([mag, 0.5 * mag]), dtype=torch.float32, device='cuda')
    p = torch.tensor(np.stack([ph, ph[:, ::-1].copy()]), dtype=torch.float32, device='cuda')
    for n_iter in (0, 1, 3):
        w = _griffinlim(built_lib, m, p, n_iter).cpu().numpy()
        for b, (mg, pp) in enumerate(((mag, ph), (0.5 * mag, ph[:, ::-1]))):
            ref = gl.griffinlim(mg.astype(np.float32).astype(np.float64), pp.astype(np.float32).astype(np.float64), n_iter)
            assert w[b].shape == ref.shape == (300 * (F - 1),)
            e = rel_l2(w[b], ref)
            print('  F=%d n_iter=%d batch %d: waveform rel-L2 %.2e' % (F, n_iter, b, e))
            assert e < (2e-5 if n_iter <= 1 else 1e-3)


def test_fifty_rounds_converge_like_the_oracle(built_lib):
    F = 24
    mag, ph = _case(F, 11)
    mag32, ph32 = mag.astype(np.float32), ph.astype(np.float32)
    w = _griffinlim(built_lib, torch.tensor(mag32[None], device='cuda'), torch.tensor(ph32[None], device='cuda'), 50).cpu().numpy()[0]
    ref = gl.griffinlim(mag32.astype(np.float64), ph32.astype(np.float64), 50)
    sc_hip, sc_ref = gl.spectral_convergence(w.astype(np.float64), mag), gl.spectral_convergence(ref, mag)
    sc0 = gl.spectral_convergence(gl.griffinlim(mag32.astype(np.float64), ph32.astype(np.float64), 0), mag)
    print('  spectral convergence after 50 rounds: hip %.4f oracle %.4f (random phase: %.4f); waveform rel-L2 %.2e'
          % (sc_hip, sc_ref, sc0, rel_l2(w, ref)))
    assert sc_hip < 0.5 * sc0 and abs(sc_hip - sc_ref) <= 0.02 * sc_ref + 1e-3


def test_output_to_waveform_pipeline(built_lib):
    """test.py:64 end to end on the device: normalised r-frame output -> de-normalise -> frames -> exp -> Griffin-Lim."""
    from tacotron_amd.audio import denormalize, reshape_frames
    from tacotron_amd.griffinlim import invert_spectrogram
    rng = np.random.default_rng(5)
    B, Td, r = 2, 12, 2
    out = rng.standard_normal((B, Td, 1025 * r)).astype(np.float32) * 0.3
    mean = rng.standard_normal(1025 * r).astype(np.float32) * 0.1 - 2.0
    std = (0.5 + rng.random(1025 * r)).astype(np.float32)
    F = (Td // 4) * 4 * r
    ph = (2 * np.pi * rng.random((B, 1025, F))).astype(np.float32)
    G = Guarded({'mag_t': ((B, 1025, F), torch.float32, 'qnan'), 'wave': ((B, 300 * (F - 1)), torch.float32, 'qnan'),
                 'work': ((built_lib.griffinlim_workspace_floats(B, F),), torch.float32, 'qnan'),
                 'spec': ((B, F, 1025), torch.float32, 'qnan')})
    w = invert_spectrogram(torch.tensor(out, device='cuda'), mean, std, r, n_iter=2, phase0=torch.tensor(ph, device='cuda'),
                           mag_t=G['mag_t'], wave=G['wave'], work=G['work'])
    torch.cuda.synchronize()
    G.check('mag_t', 'wave')
    w = w.cpu().numpy()
    # taco_denorm_unframe with both outputs into poisoned buffers: spec fully written, and mag_t = exp(spec) transposed
    G.refill('mag_t')
    spec_d, mag_d = built_lib.denorm_unframe(torch.tensor(out, device='cuda'), torch.tensor(mean, device='cuda'),
                                             torch.tensor(std, device='cuda'), r, want_spec=True, want_mag_t=True,
                                             spec=G['spec'], mag_t=G['mag_t'])
    torch.cuda.synchronize()
    G.check('spec', 'mag_t')
    for b in range(B):
        spec = reshape_frames(denormalize(out[b].astype(np.float64), mean.astype(np.float64), std.astype(np.float64)), r, forward=False)
        ref = gl.griffinlim(np.exp(spec.T), ph[b].astype(np.float64), 2)     # audio.invert_spectrogram: griffinlim(np.exp(spec.T))
        assert rel_l2(w[b], ref) < 1e-3
        assert rel_l2(spec_d[b].cpu().numpy(), spec) < 1e-6 and rel_l2(mag_d[b].cpu().numpy(), np.exp(spec.T)) < 1e-5
