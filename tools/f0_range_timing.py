"""What the intonation range costs: taco_f0_range_curve at B = 32 rows of F = 360, 720 and 8192 frames, with smooth W = 0 and W = 2, with
and without a base curve, on seeded pitch tracks (a slow sinusoid of log2(period) in the tracker's range, 70 % of the frames voiced,
scale 1.5 in every row so that no row takes the neutral copy), against
  - taco_f0_stats on the same `period` in the same run: the same read plus the same reduction, the natural yardstick;
  - the host path it replaces: `period` copied back, the NumPy restatement (tests/f0_range_ref.curve, float32), the curve uploaded.
    It runs --host-reps times, not --reps x --calls;
  - at F = 360 and 720 the calls on either side of it at C = 1025, taco_frames_f0 and taco_frames_pitch_curve, and the Griffin-Lim
    call the chain ends in (taco_griffinlim, 50 rounds, --gl-calls calls per repetition): `share_of_griffinlim` is the curve's
    median over that call's.  (At F = 8192 the magnitudes of 32 rows are 1 GiB: the curve and the statistics alone.)

The device forms are timed with device events around --calls (>= 200) calls after warm-up, enqueued behind a kernel that holds the
stream for --hold-ms so that they are all queued when the clock starts, and ALTERNATE --reps (>= 5) times in the one process;
reported per call: the median over the repetitions and their spread (max - min).

    python tools/f0_range_timing.py [--reps 7] [--calls 200] [--out DIR]

Prints one JSON line; with --out also writes it to DIR/f0_range_timing.json.  No pass mark: exit status 0 unless a call fails."""
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
from tests import f0_range_cases as rc  # noqa: E402
from tests import f0_range_ref as rr  # noqa: E402

B, C = 32, 1025
FRAMES = (360, 720, 8192)
CHAIN_FRAMES = (360, 720)
SCALE = 1.5


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


def one_shape(a, F, dev):
    period_h = rc.rows(F, None, ['random'] * B, seed=1000 + F)
    base_h = rc.bases(B, F, seed=F)
    scale_h = (rc.q(SCALE),) * B
    period, base = torch.from_numpy(period_h).to(dev), torch.from_numpy(base_h).to(dev)
    scale = torch.tensor(scale_h, dtype=torch.int32).to(dev)
    step, stats = torch.empty(B, F, dtype=torch.int32, device=dev), torch.empty(B, 3, device=dev)
    forms = {'f0_stats': (lambda: lib.f0_stats(period, out=stats), a.calls)}
    for W in (0, 2):
        for name, bq in (('', None), ('_base', base)):
            forms['f0_range_curve_W%d%s' % (W, name)] = (lambda W=W, bq=bq: lib.f0_range_curve(period, None, 1, scale, bq, W, rr.LIMIT, out=step),
                                                         a.calls)
    if F in CHAIN_FRAMES:
        g = torch.Generator(device=dev).manual_seed(3)
        x = torch.exp(torch.randn(B, C, F, generator=g, device=dev) * 2.0)
        moved = torch.empty_like(x)
        weight, gain, lag_min, lag_max = lib.f0_tables()
        f0_kw = dict(weight=torch.from_numpy(weight).to(dev), gain=torch.from_numpy(gain).to(dev), lag_min=lag_min, lag_max=lag_max)
        track = (torch.empty(B, F, device=dev), torch.empty(B, F, device=dev))
        lib.f0_range_curve(period, None, 1, scale, None, rr.SMOOTH, rr.LIMIT, out=step)
        curve = step.clone()
        phase0 = torch.rand(B, C, F, generator=g, device=dev) * (2.0 * np.pi)
        wave, work = torch.empty(B, 300 * (F - 1), device=dev), torch.empty(lib.griffinlim_workspace_floats(B, F), device=dev)
        forms['frames_f0'] = (lambda: lib.frames_f0(x, **f0_kw, out=track), a.calls)
        forms['frames_pitch_curve'] = (lambda: lib.frames_pitch_curve(x, None, curve, out=moved), a.calls)
        forms['griffinlim_50'] = (lambda: lib.griffinlim(x, phase0, 50, out=wave, work=work), a.gl_calls)
    ts = {k: [] for k in forms}
    for _ in range(a.warmup):
        for fn, calls in forms.values():
            time_calls(fn, min(calls, 20), 0.0)
    for _ in range(a.reps):
        for k, (fn, calls) in forms.items():
            ts[k].append(time_calls(fn, calls, a.hold_ms))
    res = {'F': F, 'period_bytes': 4 * B * F, 'voiced_share': float((period_h > 0).mean()), 'unit': 'ms per call'}
    for k, v in ts.items():
        res[k] = med_spread(v)
    for k in [k for k in ts if k.startswith('f0_range_curve')]:
        res[k]['over_f0_stats'] = res[k]['median'] / res['f0_stats']['median']
        if 'griffinlim_50' in res:
            res[k]['share_of_griffinlim'] = res[k]['median'] / res['griffinlim_50']['median']

    def host():   # what a user has without the entry point
        p = period.cpu().numpy()
        s = rr.curve(p, None, 1, scale_h, base_h, rr.SMOOTH, rr.LIMIT, dtype=np.float32)[0]
        torch.from_numpy(s).to(dev)
        torch.cuda.synchronize()
        return s
    want = host()
    hs = []
    for _ in range(a.host_reps):
        t0 = time.perf_counter()
        host()
        hs.append(1e3 * (time.perf_counter() - t0))
    res['host_numpy_W2_base'] = med_spread(hs)
    res['host_over_kernel_W2_base'] = res['host_numpy_W2_base']['median'] / res['f0_range_curve_W2_base']['median']
    lib.f0_range_curve(period, None, 1, scale, base, rr.SMOOTH, rr.LIMIT, out=step)
    torch.cuda.synchronize()
    res['worst_step_difference_from_host_float32'] = float(np.abs(step.cpu().numpy().astype(np.int64) - want).max())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--gl-calls', type=int, default=3)
    ap.add_argument('--hold-ms', type=float, default=20.0)
    ap.add_argument('--host-reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'f0_range_timing needs a GPU'
    assert a.reps >= 5 and a.calls >= 200, 'at least 5 alternations of at least 200 calls'
    dev = torch.device('cuda', torch.cuda.current_device())
    res = {'tool': 'f0_range_timing', 'B': B, 'C': C, 'scale': SCALE, 'limit': rr.LIMIT, 'reps': a.reps, 'warmup': a.warmup, 'calls': a.calls,
           'gl_calls': a.gl_calls, 'hold_ms': a.hold_ms, 'host_reps': a.host_reps, 'version': lib.version(),
           'device': torch.cuda.get_device_name(dev), 'lengths': [one_shape(a, F, dev) for F in FRAMES]}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, 'f0_range_timing.json'), 'w') as f:
            f.write(line + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
