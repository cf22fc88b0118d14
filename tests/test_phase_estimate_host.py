"""The single-pass phase estimate on the host: what the restatement (tests/phase_estimate_ref.py, the rules of include/taco_hip.h
taco_phase_estimate) does to a stationary sinusoid, to lobes, to bins without an owner and at the wrap of its accumulators; the
convergence claims of DESIGN.md 4b on the four inputs of tests/fgl_ref.py, in fp64 rounds on fp32-rounded inputs; and the argument
errors of invert_spectrogram / check_options that need no device."""
import numpy as np
import pytest

from oracle import griffinlim_numpy as gl
from tests import fgl_ref
from tests import phase_estimate_ref as pr

K = pr.K


def _tone(k_frac, F=6, amp=1.0):
    """|STFT| (K, F) fp32 of a stationary sinusoid at the fractional bin k_frac"""
    n = np.arange(300 * (F - 1))
    return np.abs(gl.stft(amp * np.sin(2 * np.pi * k_frac * n / 2048.0))).astype(np.float32)


@pytest.mark.parametrize('k_frac', [100.0, 100.25, 100.5, 317.8, 900.4])
def test_a_stationary_sinusoid_advances_by_hop_times_frequency(k_frac):
    mag = _tone(k_frac)
    col = mag[:, 3]
    own, adv = pr.frame_tables(col)
    k = int(np.argmax(col))
    assert own[k] == k and abs(k - k_frac) <= 0.5 + 1e-9
    # the bar is the parabola's bias: through three bins of the linear magnitudes of a Hann lobe it is below 0.1 bin even without
    # zero padding, worst near a quarter bin off the centre; the 1200-sample window in 2048 points has a main lobe of 6.8 bins and
    # stays well inside that.  300 / 2048 turns per bin
    want = 300.0 * k_frac / 2048.0
    got = (adv[k].astype(np.float64) / 2.0 ** 32)
    d = (got - want + 0.5) % 1.0 - 0.5
    assert abs(d) <= 0.1 * 300.0 / 2048.0, (k_frac, got, want % 1.0)
    acc = pr.frame_update(np.zeros(K, dtype=np.uint32), col)
    assert acc[k] == adv[k]
    # exactly: Q16 offset, then integers
    a, b, c = col[k - 1], col[k], col[k + 1]
    p = np.float32(np.float32(0.5) * (a - c)) / np.float32((a - np.float32(2) * b) + c)
    q = int(np.rint(np.clip(p, np.float32(-0.5), np.float32(0.5)) * np.float32(65536)))
    assert int(adv[k]) == ((300 * (k * 65536 + q)) << 5) % 2 ** 32


def test_lobe_bins_equal_the_peak_and_unowned_bins_keep_theirs():
    m = np.full(K, 0.1, dtype=np.float32)
    m[200:207] = (0.2, 0.5, 0.9, 1.0, 0.8, 0.4, 0.15)    # one lobe, peak at 203
    m[900:903] = (0.3, 0.6, 0.3)                         # and one at 901
    m[1010:] = (0.1 + 0.01 * np.arange(1, 16)).astype(np.float32)   # rises into bin 1024: no owner
    own, adv = pr.frame_tables(m)
    assert (own[199:899] == 203).all(), 'the bins that rise into the peak, the peak, and the bins that fall from it'
    assert (own[899:1009] == 901).all() and own[1024] == 901, 'the last bin does not rise: it takes the peak on its left'
    assert (own[:199] == -1).all(), 'bins left of the first peak that do not rise have no owner'
    assert (own[1009:1024] == -1).all(), 'bins that rise into bin K - 1 have no owner'
    rng = np.random.default_rng(0)
    acc = rng.integers(0, 2 ** 32, size=K, dtype=np.uint64).astype(np.uint32)
    new = pr.frame_update(acc, m)
    assert (new[199:899] == new[203]).all() and new[203] == np.uint32((int(acc[203]) + int(adv[203])) % 2 ** 32)
    assert (new[899:1009] == new[901]).all() and new[1024] == new[901]
    assert new[901] == np.uint32((int(acc[901]) + int(adv[901])) % 2 ** 32)
    assert np.array_equal(new[:199], acc[:199]) and np.array_equal(new[1009:1024], acc[1009:1024])
    # a frame without peaks carries every accumulator; so does the absolute value of a negative frame what the positive one does
    assert np.array_equal(pr.frame_update(acc, np.zeros(K, dtype=np.float32)), acc)
    assert np.array_equal(pr.frame_update(acc, -m), new)


def test_accumulators_wrap():
    m = np.full(K, 0.1, dtype=np.float32)
    m[1000:1003] = (0.3, 0.6, 0.3)
    _, adv = pr.frame_tables(m)
    assert int(adv[1001]) == (300 * 1001 * 65536 * 32) % 2 ** 32 and 300 * 1001 * 65536 * 32 > 2 ** 32
    acc = np.zeros(K, dtype=np.uint32)
    seen = []
    for _ in range(40):
        acc = pr.frame_update(acc, m)
        seen.append(int(acc[1001]))
    assert seen == [(int(adv[1001]) * (i + 1)) % 2 ** 32 for i in range(40)]
    assert any(b < a for a, b in zip(seen, seen[1:])), 'never wrapped'
    ph = pr.phase_of(acc)
    assert ph.dtype == np.float32 and (ph >= 0).all() and (ph < np.float32(2 * np.pi) + 1e-6).all()
    # step 6: half a turn per odd bin
    zero = pr.phase_of(np.zeros(K, dtype=np.uint32))
    assert (zero[0::2] == 0).all() and np.allclose(zero[1::2], np.pi, atol=1e-6)


def test_rows_and_lengths():
    mag = fgl_ref.case(24, 11)[0].astype(np.float32)
    dirty = mag.copy()
    dirty[:, 9:] = np.nan
    full = pr.phase_estimate_row(mag)
    cut = pr.phase_estimate(np.stack([dirty, mag]), [9, 0])
    assert np.array_equal(cut[0, :, :9].view(np.int32), full[:, :9].view(np.int32)) and (cut[0, :, 9:].view(np.int32) == 0).all()
    assert (cut[1].view(np.int32) == 0).all()
    assert np.array_equal(pr.phase_estimate(mag[None], [3], 4)[0].view(np.int32), pr.phase_estimate_row(mag, 12).view(np.int32))


_CONV = {}


def _conv(name, n_iter, momentum):
    """(estimate, random) spectral convergence of the returned waveform; every fp64 run made once"""
    key = (name, n_iter, momentum)
    if key not in _CONV:
        fn, F, seed = {c[0]: c[1:] for c in fgl_ref.CASES}[name]
        mag, ph = fgl_ref.fp32_inputs(fn, F, seed)
        est = pr.phase_estimate_row(mag)
        _CONV[key] = tuple(float(fgl_ref.griffinlim_fast(mag, p, n_iter, momentum)[1][-1]) for p in (est, ph))
    return _CONV[key]


@pytest.mark.parametrize('name', [c[0] for c in fgl_ref.CASES])
def test_ten_momentum_rounds_end_below_random_phases(name):
    est, rand = _conv(name, 10, 0.99)
    print('  %s: 10 rounds, momentum 0.99: estimate %.4f, random %.4f' % (name, est, rand))
    assert est < rand


@pytest.mark.parametrize('name', [c[0] for c in fgl_ref.CASES])
def test_no_rounds_at_all(name):
    est, rand = _conv(name, 0, 0.0)
    print('  %s: 0 rounds: estimate %.4f, random %.4f (%.2f of it)' % (name, est, rand, est / rand))
    if name == 'case(24, 11)':
        assert est <= rand
    else:
        assert est <= 0.5 * rand


def test_argument_errors_that_need_no_device(built_lib):
    import torch
    from tacotron_amd import test as drv
    from tacotron_amd.griffinlim import invert_spectrogram
    out = torch.zeros(1, 8, 2050)
    mean, std = np.zeros(2050, dtype=np.float32), np.ones(2050, dtype=np.float32)
    with pytest.raises(ValueError, match='phase_init'):
        invert_spectrogram(out, mean, std, 2, phase_init='peaks')
    with pytest.raises(ValueError, match='phase_init'):
        invert_spectrogram(out, mean, std, 2, phase_init=True)
    with pytest.raises(ValueError, match='excludes phase0'):
        invert_spectrogram(out, mean, std, 2, phase_init='estimate', phase0=torch.zeros(1, 1025, 16))
    drv.check_options(gl_init=None)
    drv.check_options(gl_init='random', vocode=False)
    drv.check_options(n_iter=0, gl_init='estimate')
    drv.check_options(n_iter=10, stop=True, vocode_lengths=True, gl_momentum=0.99, rate=0.8, pitch=2.0, gl_init='estimate')
    with pytest.raises(ValueError, match='gl-init'):
        drv.check_options(gl_init='peaks')
    with pytest.raises(ValueError, match='gl-init'):
        drv.check_options(gl_init='estimate', vocode=False)
    a = drv.parse_args(['--gl-init', 'estimate', '--gl-iters', '0'])
    assert a.gl_init == 'estimate' and a.gl_iters == 0
    assert drv.parse_args([]).gl_init == 'random'
    with pytest.raises(SystemExit):
        drv.parse_args(['--gl-init', 'peaks'])


def test_wrapper_checks_come_before_the_device(built_lib):
    import torch
    lib = built_lib
    m = torch.zeros(2, 1025, 8)
    with pytest.raises(ValueError, match='phase_estimate: mag_t'):
        lib.phase_estimate(torch.zeros(2, 1024, 8))
    with pytest.raises(ValueError, match='phase_estimate: frames'):
        lib.phase_estimate(m, torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match='frames_per_unit'):
        lib.phase_estimate(m, None, 0)
    with pytest.raises(ValueError, match='phase_estimate: out'):
        lib.phase_estimate(m, out=torch.zeros(2, 1025, 9))
    with pytest.raises(ValueError, match='overlap'):
        lib.phase_estimate(m, out=m)
    with pytest.raises(ValueError, match='must be on the GPU'):
        lib.phase_estimate(m)
    with pytest.raises(ValueError):
        lib.phase_estimate_workspace_bytes(0, 8)
    assert lib.phase_estimate_workspace_bytes(2, 8) >= 2 * 8 * 1025 * 6
    assert {'taco_phase_estimate', 'taco_phase_estimate_workspace_bytes'} <= set(lib.EXPORTS)
