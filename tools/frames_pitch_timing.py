"""What the pitch shift costs: taco_frames_pitch alone at the Nancy bin count (B = 32, C = 1025) for F = 360 and F = 720 frames at +4,
0 and -4 semitones (0 is the copy path), against
  - taco_frames_stretch at rate 1 on the same tensor: a copy of the same bytes, the floor for a kernel that reads mag_t once and
    writes out once;
  - the same shift as torch ops on the device -- log, two matmuls with the cosine basis, two index_select along the bin axis, lerp,
    exp: what a user has without the entry point (its largest relative difference from the kernel's output is reported);
  - for proportion, the 50-round Griffin-Lim call the shifted matrix goes to.

All forms are timed with device events around --calls (>= 200) calls after warm-up, enqueued behind a kernel that holds the stream for
--hold-ms so that they are all queued when the clock starts, and ALTERNATE --reps (>= 5) times in the one process; reported per call:
the median over the repetitions and their spread (max - min).  The bytes the shift must move are B C F floats in and as many out;
gb_per_s is that over the median.  47 / 94 MB in and as much out fit the 256 MiB Infinity Cache, so the rates are not HBM rates.

    python tools/frames_pitch_timing.py [--reps 7] [--calls 200] [--gl-reps 3] [--out DIR]

Prints one JSON line; with --out also writes it to DIR/frames_pitch_timing.json.  No pass mark: exit status 0 unless a call fails."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tacotron_amd import lib  # noqa: E402

B, C = 32, 1025
FRAMES = (360, 720)
SEMITONES = (4.0, 0.0, -4.0)
LIFTER = 32


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


def torch_form(x, step, Q, dev):
    """the definition of include/taco_hip.h as torch ops; returns the closure that computes it"""
    N = 2 * (C - 1)
    k = torch.arange(C, dtype=torch.float64)
    n = torch.arange(Q + 1, dtype=torch.float64)
    cs = torch.cos(2.0 * math.pi * torch.outer(n, k) / N)                    # (Q + 1, C)
    wt = torch.full((C,), 2.0, dtype=torch.float64)
    wt[0] = wt[-1] = 1.0
    to_cep = (cs * wt[None, :] / N).to(torch.float32).to(dev)               # c = to_cep @ L
    back = cs.t().clone()
    back[:, 1:] *= 2.0
    to_env = back.to(torch.float32).to(dev)                                 # E = to_env @ c
    p = torch.arange(C, dtype=torch.int64) * step
    i, frac = p >> 16, p & 0xFFFF
    inner = i < C - 1
    top = (i == C - 1) & (frac == 0)
    i0 = torch.where(inner | top, i, torch.zeros_like(i)).to(dev)
    i1 = torch.where(inner, i + 1, torch.where(top, i, torch.zeros_like(i))).to(dev)
    w = (frac.to(torch.float32) * (2.0 ** -16))[None, :, None].to(dev)
    keep = (inner | top).to(torch.float32)[None, :, None].to(dev)

    def run():
        L = torch.log(torch.clamp(x, min=1e-8))
        E = torch.matmul(to_env, torch.matmul(to_cep, L))
        Rr = L - E
        Rp = torch.lerp(torch.index_select(Rr, 1, i0), torch.index_select(Rr, 1, i1), w) * keep
        return torch.exp(E + Rp)

    return run


def one_length(a, F, dev):
    g = torch.Generator(device='cpu').manual_seed(3)
    x = torch.exp(torch.randn(B, C, F, generator=g) * 2.0).to(dev)
    out = torch.empty_like(x)
    copy_out = torch.empty_like(x)
    n = torch.empty(B, dtype=torch.int32, device=dev)
    steps = {s: torch.full((B,), lib.pitch_step(s), dtype=torch.int32, device=dev) for s in SEMITONES}
    forms = {'frames_pitch_%+g' % s: (lambda q=steps[s]: lib.frames_pitch(x, None, q, lifter=LIFTER, out=out)) for s in SEMITONES}
    forms['frames_stretch_rate_1'] = lambda: lib.frames_stretch(x, None, None, Fo=F, out=copy_out, frames_out=n)
    forms['torch_ops_+4'] = torch_form(x, lib.pitch_step(4.0), LIFTER, dev)
    ref = forms['torch_ops_+4']()
    got = forms['frames_pitch_+4']()
    diff = float(((got - ref).abs() / ref).max())
    copied = bool(torch.equal(forms['frames_pitch_+0']().view(torch.int32), x.view(torch.int32)))
    del ref
    ts = {k: [] for k in forms}
    for _ in range(a.warmup):
        for fn in forms.values():
            time_calls(fn, a.calls, 0.0)
    for _ in range(a.reps):
        for k, fn in forms.items():
            ts[k].append(time_calls(fn, a.calls, a.hold_ms))
    nbytes = 2 * 4 * B * C * F
    res = {'F': F, 'lifter': LIFTER, 'bytes_to_move': nbytes, 'unit': 'ms per call', 'torch_max_rel_diff': diff,
           'zero_semitones_is_a_copy': copied}
    for k, v in ts.items():
        res[k] = med_spread(v)
        res[k]['gb_per_s'] = nbytes / (res[k]['median'] * 1e-3) / 1e9
    floor = res['frames_stretch_rate_1']['median']
    res['pitch_over_copy_floor'] = {('%+g' % s): res['frames_pitch_%+g' % s]['median'] / floor for s in SEMITONES}
    res['torch_over_kernel'] = res['torch_ops_+4']['median'] / res['frames_pitch_+4']['median']
    # the Griffin-Lim call the shifted matrix goes to: 50 rounds over all F frames of every row
    forms['frames_pitch_+4']()
    n.fill_(F)
    work = torch.empty(lib.griffinlim_rows_workspace_floats(B, F), dtype=torch.float32, device=dev)
    wave = torch.empty(B, 300 * (F - 1), dtype=torch.float32, device=dev)
    gl = []
    for rep in range(1 + a.gl_reps):   # (the first one is the warm-up)
        t = time_calls(lambda: lib.griffinlim_rows(out, n, seed=0, n_iter=50, out=wave, work=work), 1, 0.0)
        if rep:
            gl.append(t)
    res['griffinlim_rows_50_rounds'] = med_spread(gl)
    res['pitch_share_of_griffinlim'] = res['frames_pitch_+4']['median'] / res['griffinlim_rows_50_rounds']['median']
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--hold-ms', type=float, default=20.0)
    ap.add_argument('--gl-reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'frames_pitch_timing needs a GPU'
    assert a.reps >= 5 and a.calls >= 200, 'at least 5 alternations of at least 200 calls'
    dev = torch.device('cuda', torch.cuda.current_device())
    res = {'tool': 'frames_pitch_timing', 'B': B, 'C': C, 'reps': a.reps, 'warmup': a.warmup, 'calls': a.calls, 'hold_ms': a.hold_ms,
           'version': lib.version(), 'device': torch.cuda.get_device_name(dev), 'lengths': [one_length(a, F, dev) for F in FRAMES]}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, 'frames_pitch_timing.json'), 'w') as f:
            f.write(line + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
