"""Time of the training monitor's device pass (taco_tensor_stats, as Tacotron.step(monitor=True) calls it) on an S1-shaped model:
B = 32, Tt = 200, Td = 180, r = 2, after a few train steps so that every buffer holds what a run would show.

  - the calls on the model's buffers: parameters, gradients, Adam m and v, the workspace's histogram sites and the two output tensors
    (Tacotron.monitor_stats: one call per buffer), all of them and buffer by buffer;
  - a device copy of the same number of bytes, buffer by buffer (one contiguous copy each).  The copy moves twice the bytes the call
    reads (it also writes them), so a multiple above 1 is an open item, not a failure;
  - the same statistics as torch ops: per segment isfinite / sum / sum of squares / min / max / count of zeros / histc of log2 |x|
    -- what the call replaces, about ten launches per segment;
  - the train step at a monitor step and at a plain step, alternating in the same run.

Device events around each variant, the variants alternating inside each repetition, the median over --reps.  The calls are also timed
per call of a burst of 10 (a single call carries the launch latency of an idle queue).

    python tools/tensor_stats_timing.py [--reps 20] [--warmup 3] [--out DIR]

Prints one JSON line; with --out also writes it to DIR/tensor_stats_timing.json.  No pass mark: the exit status is 0 unless a call
fails or the device's finite counts and extremes disagree with torch's."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')

import torch  # noqa: E402

from tacotron_amd import lib  # noqa: E402
from tacotron_amd.config import Config  # noqa: E402
from tacotron_amd.data import synthetic_batch  # noqa: E402
from tacotron_amd.model import MONITOR_FORWARD, MONITOR_UPDATE, Tacotron  # noqa: E402
from tools.griffinlim_timing import alternate  # noqa: E402

B, TT, TD, R, V, BURST = 32, 200, 180, 2, 60, 10


def torch_stats(x, edges_log2):
    """the statistics of one slice as torch ops -> (finite, min, max) as device scalars (the rest is computed and dropped)"""
    fin = torch.isfinite(x)
    v = torch.where(fin, x, torch.zeros_like(x))
    n = fin.sum()
    s, s2 = v.double().sum(), (v.double() * v.double()).sum()
    zeros = (x == 0).sum()
    mn = torch.where(fin, x, torch.full_like(x, float('inf'))).min()
    mx = torch.where(fin, x, torch.full_like(x, float('-inf'))).max()
    h = torch.histc(torch.log2(v.abs().clamp_min(2.0 ** -126)), bins=len(edges_log2) - 1, min=edges_log2[0], max=edges_log2[-1])
    return n, mn, mx, s, s2, zeros, h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--torch-reps', type=int, default=3, help='repetitions of the torch-ops loop (thousands of launches each)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'tensor_stats_timing needs a GPU'
    c = Config()
    c.r, c.vocab_size, c.max_decode_iter = R, V, TD
    m = Tacotron(c, synthetic_batch(B, TT, TD, R, V), train=True, seed=0)
    for _ in range(3):
        m.step(1e-3)
    m.step(1e-3, monitor=True)
    torch.cuda.synchronize()
    m.check()
    sites, bufs, order = m.monitor_sites(), m._monitor['bufs'], MONITOR_FORWARD + MONITOR_UPDATE
    floats = {k: sum(s for _, _, s in sites[k]) for k in order}
    dst = torch.empty(max(floats.values()), device=m.device)

    def call_all():
        m.monitor_stats()

    def call_burst():
        for _ in range(BURST):
            m.monitor_stats()

    def copy_all():
        for k in order:
            dst[:floats[k]].copy_(bufs[k].view(-1)[:floats[k]])

    res = {'tool': 'tensor_stats_timing', 'B': B, 'Tt': TT, 'Td': TD, 'r': R, 'version': lib.version(), 'reps': a.reps, 'warmup': a.warmup,
           'segments': {k: len(sites[k]) for k in order}, 'work_items': {k: m._monitor['plans'][k].n_items for k in order},
           'floats': floats, 'chunk': lib.STATS_CHUNK, 'bins': int(m.monitor_result.hist.shape[1]),
           'unit': 'ms (median; variants alternate inside each repetition)'}
    fns = {'calls_all_buffers': call_all, 'calls_all_buffers_x%d' % BURST: call_burst, 'copy_all_buffers': copy_all}
    for k in order:
        fns['call_' + k] = (lambda k=k: m.monitor_stats((k,)))
        fns['copy_' + k] = (lambda k=k: dst[:floats[k]].copy_(bufs[k].view(-1)[:floats[k]]))
    ev = alternate(fns, a.reps, a.warmup)
    ev['calls_all_buffers_steady'] = ev.pop('calls_all_buffers_x%d' % BURST) / BURST
    res['events'] = ev
    # the same statistics as torch ops, and the device's results against them
    edges_log2 = [float(lib.STATS_E_LO), float(lib.STATS_E_HI + 1)]
    edges_log2 = [edges_log2[0] + i / 4.0 for i in range(int((edges_log2[1] - edges_log2[0]) * 4) + 1)]
    got = {}

    def torch_all():
        for k in order:
            flat = bufs[k].view(-1)
            got[k] = [torch_stats(flat[o:o + s], edges_log2)[:3] for _, o, s in sites[k]]

    res['events'].update(alternate({'torch_ops_all_buffers': torch_all}, a.torch_reps, 1))
    m.monitor_stats()
    torch.cuda.synchronize()
    counts, moments = m.monitor_result.counts.cpu(), m.monitor_result.moments.cpu()
    same, row = True, 0
    for k in order:
        for n, mn, mx in got[k]:
            same = same and int(n) == int(counts[row, 1]) and float(mn) == float(moments[row, 2]) and float(mx) == float(moments[row, 3])
            row += 1
    res['device_equals_torch'] = bool(same)
    # the train step with and without the monitor
    res['events'].update(alternate({'train_step': lambda: m.step(1e-3), 'train_step_monitor': lambda: m.step(1e-3, monitor=True)},
                                   a.reps, a.warmup))
    m.check()
    ev = res['events']
    nbytes = 4.0 * sum(floats.values())
    res['checks'] = {'bytes_read': nbytes, 'steady_gb_per_s_read': nbytes / (ev['calls_all_buffers_steady'] * 1e-3) / 1e9,
                     'copy_gb_per_s_read_plus_written': 2.0 * nbytes / (ev['copy_all_buffers'] * 1e-3) / 1e9,
                     'calls_over_copy_of_the_same_bytes': ev['calls_all_buffers_steady'] / ev['copy_all_buffers'],
                     'calls_over_copy_by_buffer': {k: ev['call_' + k] / ev['copy_' + k] for k in order},
                     'torch_ops_over_calls': ev['torch_ops_all_buffers'] / ev['calls_all_buffers'],
                     'monitor_step_over_plain_step': ev['train_step_monitor'] / ev['train_step'],
                     'monitor_step_minus_plain_step_ms': ev['train_step_monitor'] - ev['train_step']}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, 'tensor_stats_timing.json'), 'w') as f:
            f.write(line + '\n')
    return 0 if same else 1


if __name__ == '__main__':
    sys.exit(main())
