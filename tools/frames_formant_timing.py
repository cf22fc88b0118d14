"""What the formant shift costs: taco_frames_formant alone at the Nancy bin count (B = 32, C = 1025, lifter 32) for F = 360 and
F = 720 frames at +4 and -4 semitones, on one run against
  - taco_frames_sharpen (beta 0.4) and taco_frames_pitch (+-4 semitones) on the same bytes: the kernels whose shape it shares.  The
    expectation to confirm or refute: a cost near the sharpen kernel's -- the same two MFMA stages, two reads per element, one
    logarithm and one exponential, and an output stage that keeps y in registers where the sharpen kernel keeps it in LDS;
  - taco_frames_stretch at rate 1 on the same tensor: a copy of the same bytes, the floor for a kernel that reads mag_t once and
    writes out once;
  - the same computation as torch ops on the device -- log, two matmuls with the cosine basis, a gather and a lerp along the bin
    axis, exp, two sums of squares -- what a user has without the entry point (its largest relative difference from the kernel's
    output is reported);
  - for proportion, the 50-round Griffin-Lim call the shifted matrix goes to.

All forms are timed with device events around --calls (>= 200) calls after warm-up, enqueued behind a kernel that holds the stream for
--hold-ms so that they are all queued when the clock starts, and ALTERNATE --reps (>= 5) times in the one process; reported per call:
the median over the repetitions and their spread (max - min).  47 / 94 MB in and as much out fit the 256 MiB Infinity Cache, so the
rates are not HBM rates.

    python tools/frames_formant_timing.py [--reps 7] [--calls 200] [--gl-reps 3] [--out DIR]

Prints one JSON line; with --out also writes it to DIR/frames_formant_timing.json.  No pass mark: exit status 0 unless a call fails."""
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
SEMITONES = (4.0, -4.0)
LIFTER = 32
BETA = 0.4


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


def torch_form(x, step_q, Q, dev):
    """the definition of include/taco_hip.h as torch ops -> a closure"""
    N = 2 * (C - 1)
    k = torch.arange(C, dtype=torch.float64)
    n = torch.arange(Q + 1, dtype=torch.float64)
    cs = torch.cos(2.0 * math.pi * torch.outer(n, k) / N)                    # (Q + 1, C)
    wt = torch.full((C,), 2.0, dtype=torch.float64)
    wt[0] = wt[-1] = 1.0
    to_cep = (cs * wt[None, :] / N).to(torch.float32).to(dev)               # c = to_cep @ L
    back = (2.0 * cs.t()).clone()
    back[:, 0] = 1.0
    to_env = back.to(torch.float32).to(dev)                                 # E = to_env @ c
    p = torch.arange(C, dtype=torch.int64) * int(step_q)
    i, w = p >> 16, ((p & 0xFFFF).double() / 65536.0).to(torch.float32)
    inner = i < C - 1
    i0 = torch.where(inner, i, torch.full_like(i, C - 1)).to(dev)
    i1 = torch.where(inner, i + 1, torch.full_like(i, C - 1)).to(dev)
    w = torch.where(inner, w, torch.zeros_like(w)).to(dev)[None, :, None]

    def formant():
        E = torch.matmul(to_env, torch.matmul(to_cep, torch.log(torch.clamp(x, min=1e-8))))
        e0 = E.index_select(1, i0)
        y = x * torch.exp(e0 + w * (E.index_select(1, i1) - e0) - E)
        g = torch.sqrt((x * x).sum(dim=1, keepdim=True) / (y * y).sum(dim=1, keepdim=True))
        return y * g

    return formant


def one_length(a, F, dev):
    g = torch.Generator(device='cpu').manual_seed(3)
    x = torch.exp(torch.randn(B, C, F, generator=g) * 2.0).to(dev)
    out, sharp_out, pitch_out, copy_out = (torch.empty_like(x) for _ in range(4))
    n = torch.empty(B, dtype=torch.int32, device=dev)
    fsteps = {s: torch.full((B,), lib.formant_step(s), dtype=torch.int32, device=dev) for s in SEMITONES}
    psteps = {s: torch.full((B,), lib.pitch_step(s), dtype=torch.int32, device=dev) for s in SEMITONES}
    forms = {'frames_formant_%+g' % s: (lambda q=fsteps[s]: lib.frames_formant(x, None, q, lifter=LIFTER, out=out)) for s in SEMITONES}
    forms['frames_sharpen'] = lambda: lib.frames_sharpen(x, BETA, LIFTER, out=sharp_out)
    forms.update({'frames_pitch_%+g' % s: (lambda q=psteps[s]: lib.frames_pitch(x, None, q, lifter=LIFTER, out=pitch_out)) for s in SEMITONES})
    forms['frames_stretch_rate_1'] = lambda: lib.frames_stretch(x, None, None, Fo=F, out=copy_out, frames_out=n)
    diffs = {}
    for s in SEMITONES:
        forms['torch_ops_formant_%+g' % s] = torch_form(x, lib.formant_step(s), LIFTER, dev)
        ref = forms['torch_ops_formant_%+g' % s]()
        diffs['%+g' % s] = float(((forms['frames_formant_%+g' % s]() - ref).abs() / ref).max())
        del ref
    ts = {k: [] for k in forms}
    for _ in range(a.warmup):
        for fn in forms.values():
            time_calls(fn, a.calls, 0.0)
    for _ in range(a.reps):
        for k, fn in forms.items():
            ts[k].append(time_calls(fn, a.calls, a.hold_ms))
    nbytes = 2 * 4 * B * C * F
    res = {'F': F, 'lifter': LIFTER, 'beta': BETA, 'bytes_to_move': nbytes, 'unit': 'ms per call', 'torch_max_rel_diff': diffs}
    for k, v in ts.items():
        res[k] = med_spread(v)
        res[k]['gb_per_s'] = nbytes / (res[k]['median'] * 1e-3) / 1e9
    floor = res['frames_stretch_rate_1']['median']
    formant = max(res['frames_formant_%+g' % s]['median'] for s in SEMITONES)
    pitch = min(res['frames_pitch_%+g' % s]['median'] for s in SEMITONES)
    res['formant_over_sharpen'] = formant / res['frames_sharpen']['median']
    res['formant_over_pitch'] = formant / pitch
    res['formant_over_copy_floor'] = formant / floor
    res['torch_over_kernel'] = {'%+g' % s: res['torch_ops_formant_%+g' % s]['median'] / res['frames_formant_%+g' % s]['median'] for s in SEMITONES}
    # the Griffin-Lim call the shifted matrix goes to: 50 rounds over all F frames of every row
    forms['frames_formant_%+g' % SEMITONES[0]]()
    n.fill_(F)
    work = torch.empty(lib.griffinlim_rows_workspace_floats(B, F), dtype=torch.float32, device=dev)
    wave = torch.empty(B, 300 * (F - 1), dtype=torch.float32, device=dev)
    gl = []
    for rep in range(1 + a.gl_reps):   # (the first one is the warm-up)
        t = time_calls(lambda: lib.griffinlim_rows(out, n, seed=0, n_iter=50, out=wave, work=work), 1, 0.0)
        if rep:
            gl.append(t)
    res['griffinlim_rows_50_rounds'] = med_spread(gl)
    res['formant_share_of_griffinlim'] = formant / res['griffinlim_rows_50_rounds']['median']
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
    assert torch.cuda.is_available(), 'frames_formant_timing needs a GPU'
    assert a.reps >= 5 and a.calls >= 200, 'at least 5 alternations of at least 200 calls'
    dev = torch.device('cuda', torch.cuda.current_device())
    res = {'tool': 'frames_formant_timing', 'B': B, 'C': C, 'reps': a.reps, 'warmup': a.warmup, 'calls': a.calls, 'hold_ms': a.hold_ms,
           'version': lib.version(), 'device': torch.cuda.get_device_name(dev), 'lengths': [one_length(a, F, dev) for F in FRAMES]}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, 'frames_formant_timing.json'), 'w') as f:
            f.write(line + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
