"""What estimating the initial phases costs and what it buys: taco_phase_estimate at B = 32, 1025 bins and F = 360 and 720 frames on
`speechy`-shaped rows (tests/fgl_ref.py: harmonics of a vibrato pitch under a syllable envelope), against
  - one Griffin-Lim round at the same shape in the same run -- the bar: an estimate that costs more than the round it saves has not
    paid for itself -- from taco_griffinlim_fast behind the estimate at 0, 10, 30 and 50 rounds (momentum 0.99): round_ms is the
    slope (50 rounds - 0 rounds) / 50;
  - copying the magnitudes back to the host and running the NumPy restatement (tests/phase_estimate_ref.py): what a user has without
    the entry point.  It runs --host-reps times, not --reps x --calls.
Its two launches are timed separately from the kernels' own durations as torch.profiler records them over --calls calls (the owner
kernel, B x ceil(F / 16) workgroups; the chain kernel, one workgroup per row walking F dependent frames).  The rows run side by side,
so chain_us_per_frame, the chain kernel's duration over F, is what a STEP of that chain costs -- next to 0.28 us per step of
taco_alignment_path and 0.38 us per frame of taco_f0_viterbi (profiles/).  Where the profiler gives no kernel records the split is null
and `split_error` says why.

At F = 360 it also reads the device's spectral convergence per round (taco_griffinlim_fast's conv, 50 rounds, momentum 0.99 and 0)
from the estimate and from the device's seed phases: the mean and the worst row of the 32, per round.

The device forms are timed with device events around --calls calls (--gl-calls for the Griffin-Lim forms) after warm-up, enqueued
behind a kernel that holds the stream for --hold-ms so that they are all queued when the clock starts, and ALTERNATE --reps (>= 5)
times in the one process; reported per call: the median over the repetitions and their spread (max - min).

    python tools/phase_estimate_timing.py [--reps 5] [--calls 200] [--out DIR]

Prints one JSON line; with --out also writes it to DIR/phase_estimate_timing.json.  No pass mark: exit status 0 unless a call fails."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tacotron_amd import lib  # noqa: E402
from tests import fgl_ref  # noqa: E402
from tests import phase_estimate_ref as pr  # noqa: E402

B, C = 32, 1025
FRAMES = (360, 720)
ROUNDS = (0, 10, 30, 50)
KERNELS = ('phase_owner_kernel', 'phase_chain_kernel')
OTHER_CHAINS = {'taco_alignment_path_us_per_step': 0.28, 'taco_f0_viterbi_us_per_frame': 0.38}   # profiles/*_timing.json


def med_spread(v):
    return {'median': float(np.median(v)), 'spread': float(np.max(v) - np.min(v)), 'all': [float(x) for x in v]}


def time_calls(fn, calls, hold_ms):
    """ms per call of fn() between one pair of device events, the calls queued behind a stream-holding kernel"""
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if hold_ms > 0:
        lib.debug_spin(1, 64, 0, int(hold_ms * 1000))
    s.record()
    for _ in range(calls):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / calls


def kernel_split(fn, calls):
    """mean device duration in ms of each of the call's two kernels over `calls` calls, from torch.profiler"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    out = {}
    for name in KERNELS:
        hits = [ev for ev in prof.key_averages() if name in ev.key]
        if not hits:
            raise RuntimeError('the profiler recorded no %s' % name)
        total = sum(getattr(ev, 'device_time_total', None) or getattr(ev, 'cuda_time_total', 0.0) for ev in hits)
        out[name] = total / sum(ev.count for ev in hits) / 1e3
    return out


def speechy_rows(F):
    """(B, C, F) fp32: 32 seeds of fgl_ref.speechy at 360 frames; 720 frames are two of them end to end"""
    rows = np.stack([fgl_ref.speechy(FRAMES[0], 1 + b)[0].astype(np.float32) for b in range(B)])
    return rows if F == FRAMES[0] else np.concatenate([rows, rows[::-1]], axis=2)[:, :, :F]


def conv_curves(m, est, seed):
    """device conv per round at 50 rounds, from the estimate and from the seed phases: mean and worst row"""
    out = {}
    for momentum in (0.99, 0.0):
        for name, ph in (('estimate', est), ('seed', None)):
            _, c = lib.griffinlim_fast(m, None, phase0=ph, seed=seed, n_iter=50, momentum=momentum, want_conv=True)
            c = c.cpu().numpy().astype(np.float64)
            out['momentum_%g_%s' % (momentum, name)] = {'mean': [float(x) for x in c.mean(axis=0)], 'worst': [float(x) for x in c.max(axis=0)]}
    return out


def one_shape(a, F, dev):
    mag = speechy_rows(F)
    m = torch.from_numpy(mag).to(dev)
    est = torch.empty(B, C, F, device=dev)
    ws = torch.empty(lib.phase_estimate_workspace_bytes(B, F), dtype=torch.uint8, device=dev)
    wave = torch.empty(B, 300 * (F - 1), device=dev)
    work = torch.empty(lib.griffinlim_fast_workspace_floats(B, F), device=dev)
    estimate = lambda: lib.phase_estimate(m, None, 1, out=est, workspace=ws)   # noqa: E731
    estimate()
    forms = {'phase_estimate': (estimate, a.calls)}
    for n in ROUNDS:
        forms['griffinlim_fast_%d_rounds' % n] = ((lambda n=n: lib.griffinlim_fast(m, None, phase0=est, n_iter=n, momentum=0.99, out=wave,
                                                                                   work=work)), a.gl_calls)
    ts = {k: [] for k in forms}
    for _ in range(a.warmup):
        for fn, calls in forms.values():
            time_calls(fn, calls, 0.0)
    for _ in range(a.reps):
        for k, (fn, calls) in forms.items():
            ts[k].append(time_calls(fn, calls, a.hold_ms))
    res = {'F': F, 'mag_bytes': 4 * B * C * F, 'workspace_bytes': int(ws.numel()), 'unit': 'ms per call'}
    for k, v in ts.items():
        res[k] = med_spread(v)
    key = 'phase_estimate'
    res['round_ms'] = (res['griffinlim_fast_50_rounds']['median'] - res['griffinlim_fast_0_rounds']['median']) / 50.0
    res['estimate_over_round'] = res[key]['median'] / res['round_ms']
    res['estimate_over_0_rounds'] = res[key]['median'] / res['griffinlim_fast_0_rounds']['median']
    try:
        split = kernel_split(estimate, a.calls)
        res[key]['owner_ms'], res[key]['chain_ms'] = split[KERNELS[0]], split[KERNELS[1]]
        res[key]['chain_us_per_frame'] = 1e3 * split[KERNELS[1]] / F
    except Exception as e:   # noqa: BLE001  (no kernel records on this installation: the call's own time stands)
        res[key]['owner_ms'] = res[key]['chain_ms'] = res[key]['chain_us_per_frame'] = None
        res[key]['split_error'] = '%s: %s' % (type(e).__name__, e)
    res[key]['call_us_per_frame'] = 1e3 * res[key]['median'] / F
    res[key]['other_chains'] = OTHER_CHAINS

    def host():
        return pr.phase_estimate(m.cpu().numpy())

    want = host()
    hs = []
    for _ in range(a.host_reps):
        t0 = time.perf_counter()
        host()
        hs.append(1e3 * (time.perf_counter() - t0))
    res['host_numpy'] = med_spread(hs)
    res['host_over_kernel'] = res['host_numpy']['median'] / res[key]['median']
    estimate()
    torch.cuda.synchronize()
    res[key]['equals_host'] = bool(np.array_equal(est.cpu().numpy().view(np.int32), want.view(np.int32)))
    if F == FRAMES[0]:
        res['conv_per_round'] = conv_curves(m, est, 0)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--gl-calls', type=int, default=10)
    ap.add_argument('--hold-ms', type=float, default=20.0)
    ap.add_argument('--host-reps', type=int, default=2)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'phase_estimate_timing needs a GPU'
    assert a.reps >= 5 and a.calls >= 200, 'at least 5 alternations of at least 200 calls'
    dev = torch.device('cuda', torch.cuda.current_device())
    res = {'tool': 'phase_estimate_timing', 'B': B, 'C': C, 'reps': a.reps, 'warmup': a.warmup, 'calls': a.calls, 'gl_calls': a.gl_calls,
           'hold_ms': a.hold_ms, 'host_reps': a.host_reps, 'version': lib.version(), 'device': torch.cuda.get_device_name(dev),
           'input': 'tests/fgl_ref.speechy, seeds 1 .. 32', 'lengths': [one_shape(a, F, dev) for F in FRAMES]}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, 'phase_estimate_timing.json'), 'w') as f:
            f.write(line + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
