"""What the F0 tracker costs: taco_frames_f0 alone at the Nancy bin count (B = 32, C = 1025) for F = 360 and F = 720 frames with the
16 kHz tables of lib.f0_tables (lags 40 .. 266: 229 rows of the autocorrelation), with and without the acf output, against
  - taco_frames_stretch at rate 1 on the same tensor: a copy of the same input bytes, the floor for a kernel that reads mag_t once
    (the tracker writes far less than the copy: two floats per frame, or 231 with acf, against 1025);
  - the same computation as torch ops on the device -- square, weight, one matmul with the cosine basis of the 229 lags, the
    normalisation, the candidate masks, two reductions, a gather and the parabola: what a user has without the entry point (the
    largest difference of its acf from the kernel's and the share of frames whose period agrees within 1e-3 samples are reported).

All forms are timed with device events around --calls (>= 200) calls after warm-up, enqueued behind a kernel that holds the stream for
--hold-ms so that they are all queued when the clock starts, and ALTERNATE --reps (>= 5) times in the one process; reported per call:
the median over the repetitions and their spread (max - min).  47 / 94 MB of input fit the 256 MiB Infinity Cache, so gb_per_s (the
input bytes over the median) is not an HBM rate.  mflop_per_frame is the cosine product alone: 2 L C.

    python tools/frames_f0_timing.py [--reps 7] [--calls 200] [--out DIR]

Prints one JSON line; with --out also writes it to DIR/frames_f0_timing.json.  No pass mark: exit status 0 unless a call fails."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tacotron_amd import lib  # noqa: E402

B, C = 32, 1025
FRAMES = (360, 720)


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


def torch_form(x, weight, gain, lag_min, lag_max, ratio, threshold, dev):
    """the definition of include/taco_hip.h as torch ops; returns the closure that computes (period, strength, acf)"""
    N = 2 * (C - 1)
    k = torch.arange(C, dtype=torch.float64)
    n = torch.arange(lag_min - 1, lag_max + 2, dtype=torch.float64)
    cs = torch.cos(2.0 * math.pi * torch.outer(n, k) / N).to(torch.float32).to(dev)   # (L, C)
    u = torch.full((C,), 2.0)
    u[0] = u[-1] = 1.0
    uw = (u * torch.from_numpy(weight))[None, :, None].to(dev)
    g = torch.from_numpy(gain)[None, :, None].to(dev)
    lags = torch.arange(lag_min, lag_max + 1, dtype=torch.float32, device=dev)[None, :, None]
    ninf = torch.tensor(float('-inf'), device=dev)

    def run():
        p = uw * (x * x)
        r0 = p.sum(dim=1, keepdim=True)
        y = torch.matmul(cs, p) / r0 * g
        ym, y0, yp = y[:, :-2], y[:, 1:-1], y[:, 2:]
        cand = (y0 > ym) & (y0 >= yp)
        top = torch.where(cand, y0, ninf).amax(dim=1, keepdim=True)
        ok = cand & (y0 >= ratio * top)
        at = torch.where(ok, lags, torch.full_like(lags, 1e9)).argmin(dim=1, keepdim=True)
        a_m, a_0, a_p = ym.gather(1, at), y0.gather(1, at), yp.gather(1, at)
        d = (a_m - (a_0 + a_0)) + a_p
        delta = torch.where(d == 0, torch.zeros_like(d), (0.5 * (a_m - a_p) / d).clamp(-0.5, 0.5))
        voiced = ok.any(dim=1, keepdim=True) & (a_0 >= threshold)
        zero = torch.zeros_like(a_0)
        return (torch.where(voiced, at.to(torch.float32) + lag_min + delta, zero)[:, 0], torch.where(voiced, a_0, zero)[:, 0], y)

    return run


def one_length(a, F, dev):
    g = torch.Generator(device='cpu').manual_seed(3)
    x = torch.exp(torch.randn(B, C, F, generator=g) * 2.0).to(dev)
    weight, gain, lag_min, lag_max = lib.f0_tables()
    L = lag_max - lag_min + 3
    w_d, g_d = torch.from_numpy(weight).to(dev), torch.from_numpy(gain).to(dev)
    period, strength = torch.empty(B, F, device=dev), torch.empty(B, F, device=dev)
    acf = torch.empty(B, L, F, device=dev)
    copy_out = torch.empty_like(x)
    n = torch.empty(B, dtype=torch.int32, device=dev)
    kw = dict(weight=w_d, gain=g_d, lag_min=lag_min, lag_max=lag_max, ratio=lib.F0_RATIO, threshold=0.0)
    forms = {'frames_f0': lambda: lib.frames_f0(x, **kw, out=(period, strength)),
             'frames_f0_acf': lambda: lib.frames_f0(x, **kw, want_acf=True, out=(period, strength, acf)),
             'frames_stretch_rate_1': lambda: lib.frames_stretch(x, None, None, Fo=F, out=copy_out, frames_out=n),
             'torch_ops': torch_form(x, weight, gain, lag_min, lag_max, lib.F0_RATIO, 0.0, dev)}
    ref = forms['torch_ops']()
    forms['frames_f0_acf']()
    diff = float((acf - ref[2]).abs().max())
    agree = float(((period - ref[0]).abs() < 1e-3).float().mean())
    del ref
    ts = {k: [] for k in forms}
    for _ in range(a.warmup):
        for fn in forms.values():
            time_calls(fn, a.calls, 0.0)
    for _ in range(a.reps):
        for k, fn in forms.items():
            ts[k].append(time_calls(fn, a.calls, a.hold_ms))
    nbytes = 4 * B * C * F
    res = {'F': F, 'lags': L, 'input_bytes': nbytes, 'unit': 'ms per call', 'mflop_per_frame': 2.0 * L * C / 1e6,
           'torch_max_acf_diff': diff, 'torch_period_agreement': agree}
    for k, v in ts.items():
        res[k] = med_spread(v)
        res[k]['gb_per_s'] = nbytes / (res[k]['median'] * 1e-3) / 1e9
    floor = res['frames_stretch_rate_1']['median']
    res['f0_over_copy_floor'] = {k: res[k]['median'] / floor for k in ('frames_f0', 'frames_f0_acf')}
    res['torch_over_kernel'] = res['torch_ops']['median'] / res['frames_f0_acf']['median']
    res['tflops_of_the_product'] = 2.0 * L * C * B * F / (res['frames_f0']['median'] * 1e-3) / 1e12
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--hold-ms', type=float, default=20.0)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'frames_f0_timing needs a GPU'
    assert a.reps >= 5 and a.calls >= 200, 'at least 5 alternations of at least 200 calls'
    dev = torch.device('cuda', torch.cuda.current_device())
    res = {'tool': 'frames_f0_timing', 'B': B, 'C': C, 'reps': a.reps, 'warmup': a.warmup, 'calls': a.calls, 'hold_ms': a.hold_ms,
           'version': lib.version(), 'device': torch.cuda.get_device_name(dev), 'lengths': [one_length(a, F, dev) for F in FRAMES]}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, 'frames_f0_timing.json'), 'w') as f:
            f.write(line + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
