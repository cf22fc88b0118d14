"""Time of the weight-averaging pass (taco_param_ema, as Tacotron.apply_gradients enqueues it with Config.ema_decay set) on the
buffers of an S1-shaped model: B = 32, Tt = 200, Td = 180, r = 2, n = 6,926,609 parameters, after a few train steps.

  - the call with and without its statistics, alone (one call between two events carries the launch latency of an idle queue) and per
    call of a burst of 10 (steady);
  - a device copy of n floats out of the same parameter buffer in the same run, alone and per copy of a burst of 10.  The call reads
    8 n bytes and writes 4 n, the copy reads 4 n and writes 4 n: 1.5 x the bytes;
  - the same update as torch ops: ema.lerp_(params, w) and the two norms (|params - ema|, |params|);
  - the train step of two models in the same process, one with ema_decay = 0.999 and one without, and the averaging model's step
    with the statistics asked for (a log step), all alternating.

Device events around each variant, the variants alternating inside each repetition; per variant the median, the minimum, the 10th and
90th percentile and the maximum over --reps.

    python tools/param_ema_timing.py [--reps 30] [--warmup 5] [--out DIR]

Prints one JSON line; with --out also writes it to DIR/param_ema_timing.json.  No pass mark: the exit status is 0 unless a call fails
or the average disagrees with torch's lerp by more than a few units in the last place."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tacotron_amd import lib  # noqa: E402
from tacotron_amd.config import Config  # noqa: E402
from tacotron_amd.data import synthetic_batch  # noqa: E402
from tacotron_amd.model import Tacotron  # noqa: E402

B, TT, TD, R, V, BURST, DECAY = 32, 200, 180, 2, 60, 10, 0.999


def alternate(fns, reps, warmup):
    """{name: {median, min, p10, p90, max} in ms}: each repetition runs every callable once, in order, each between its own pair of
    device events"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            e.synchronize()
            ts[k].append(s.elapsed_time(e))
    return {k: {'median': float(np.median(v)), 'min': float(np.min(v)), 'p10': float(np.percentile(v, 10)),
                'p90': float(np.percentile(v, 90)), 'max': float(np.max(v))} for k, v in ts.items()}


def per_call(stat, n):
    return {k: v / n for k, v in stat.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'param_ema_timing needs a GPU'

    def model(decay):
        c = Config()
        c.r, c.vocab_size, c.max_decode_iter, c.ema_decay = R, V, TD, decay
        return Tacotron(c, synthetic_batch(B, TT, TD, R, V), train=True, seed=0)

    plain, avg = model(0.0), model(DECAY)
    for _ in range(5):
        plain.step(1e-3)
        avg.step(1e-3)
    avg.step(1e-3, ema_stats=True)
    plain.step(1e-3)
    torch.cuda.synchronize()
    plain.check()
    avg.check()
    n = avg.params.numel
    params, ema = avg.params.flat, avg.ema
    w = lib.ema_weight(DECAY, 10 ** 6)
    stats = torch.zeros(3, dtype=torch.float64, device=avg.device)
    work = torch.empty(lib.param_ema_workspace_bytes(n), dtype=torch.uint8, device=avg.device)
    dst = torch.empty(n, device=avg.device)
    ema_t = ema.clone()
    # the call against torch's lerp on the same inputs (lerp may fuse; a few units in the last place)
    mine = ema.clone()
    lib.param_ema(mine, params, w)
    theirs = ema.clone().lerp_(params, float(w))
    gap = (mine - theirs).abs().max().item()
    scale = ema.abs().max().item()
    agrees = gap <= 4 * 2.0 ** -24 * scale

    def burst(fn):
        def run():
            for _ in range(BURST):
                fn()
        return run

    call = lambda: lib.param_ema(ema, params, w)
    call_stats = lambda: lib.param_ema(ema, params, w, None, stats, work)
    copy = lambda: dst.copy_(params)

    def torch_ops():
        ema_t.lerp_(params, float(w))
        return torch.linalg.vector_norm(params - ema_t), torch.linalg.vector_norm(params)

    ev = alternate({'call': call, 'call_stats': call_stats, 'copy': copy, 'torch_lerp_and_norms': torch_ops,
                    'call_x%d' % BURST: burst(call), 'call_stats_x%d' % BURST: burst(call_stats), 'copy_x%d' % BURST: burst(copy),
                    'torch_x%d' % BURST: burst(torch_ops)}, a.reps, a.warmup)
    for k in ('call', 'call_stats', 'copy', 'torch'):
        ev[k + '_steady'] = per_call(ev.pop('%s_x%d' % (k, BURST)), BURST)
    ev.update(alternate({'train_step': lambda: plain.step(1e-3), 'train_step_ema': lambda: avg.step(1e-3),
                         'train_step_ema_stats': lambda: avg.step(1e-3, ema_stats=True)}, a.reps, a.warmup))
    torch.cuda.synchronize()
    plain.check()
    avg.check()
    med = {k: v['median'] for k, v in ev.items()}
    res = {'tool': 'param_ema_timing', 'B': B, 'Tt': TT, 'Td': TD, 'r': R, 'n': n, 'decay': DECAY, 'version': lib.version(),
           'reps': a.reps, 'warmup': a.warmup, 'burst': BURST, 'device': torch.cuda.get_device_name(0),
           'unit': 'ms (variants alternate inside each repetition; *_steady: per call of a burst of %d)' % BURST,
           'events': ev, 'max_abs_gap_to_torch_lerp': gap, 'agrees_with_torch_lerp': bool(agrees),
           'checks': {'bytes_call': 12.0 * n, 'bytes_copy': 8.0 * n,
                      'call_steady_gb_per_s': 12.0 * n / (med['call_steady'] * 1e-3) / 1e9,
                      'call_stats_steady_gb_per_s': 12.0 * n / (med['call_stats_steady'] * 1e-3) / 1e9,
                      'copy_steady_gb_per_s': 8.0 * n / (med['copy_steady'] * 1e-3) / 1e9,
                      'call_over_copy_steady': med['call_steady'] / med['copy_steady'],
                      'call_stats_over_copy_steady': med['call_stats_steady'] / med['copy_steady'],
                      'call_over_copy_single': med['call'] / med['copy'],
                      'call_stats_over_copy_single': med['call_stats'] / med['copy'],
                      'torch_over_call_stats_steady': med['torch_steady'] / med['call_stats_steady'],
                      'ema_step_over_plain_step': med['train_step_ema'] / med['train_step'],
                      'ema_step_minus_plain_step_ms': med['train_step_ema'] - med['train_step'],
                      'ema_stats_step_minus_plain_step_ms': med['train_step_ema_stats'] - med['train_step']}}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, 'param_ema_timing.json'), 'w') as f:
            f.write(line + '\n')
    return 0 if agrees else 1


if __name__ == '__main__':
    sys.exit(main())
