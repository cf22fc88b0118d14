"""Time of the per-utterance alignment scores on the device (taco_alignment_scores, as `train --align-log` calls it at a log step)
against the host path it replaces: the (B, Td, Tt) alignment tensor copied back over PCIe, then the scores in NumPy
(tests/align_ref.py, the restatement the GPU tests compare against).

The shape is S1, the flagship training batch: B = 32, Td = 180, Tt = 200 (4.6 MB of alignments), the fp32 softmax of seeded logits
with a peak that walks each row's text.  The device call is timed with device events, alone and per call of 20 back to back (one
call is microseconds: the single-call figure carries the launch latency of an idle queue); the host path has no device events and is
timed by the host clock around a synchronised call, and so is the device call with its 256 result values copied back, for a like
comparison.  The variants alternate inside each repetition and the median over --reps is reported.

    python tools/alignment_scores_timing.py [--reps 20] [--warmup 3] [--out DIR]

Prints one JSON line; with --out also writes it to DIR/alignment_scores_timing.json.  No pass mark: the exit status is 0 unless a call
fails or the two paths disagree."""
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
from tests import align_ref  # noqa: E402
from tools.griffinlim_timing import alternate  # noqa: E402
from tools.wave_join_timing import wall  # noqa: E402

B, TD, TT, BURST = 32, 180, 200, 20


def s1_alignments(seed=0):
    rng = np.random.default_rng(seed)
    tl = rng.integers(60, TT + 1, size=B).astype(np.int32)
    logits = rng.standard_normal((B, TD, TT)).astype(np.float32)
    t = np.arange(TD)
    for b in range(B):
        logits[b, t, np.clip(t * int(tl[b]) // 150 + rng.integers(-2, 3, size=TD), 0, TT - 1)] += np.float32(6.0)
    e = np.exp(logits - logits.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True, dtype=np.float32)).astype(np.float32), tl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'alignment_scores_timing needs a GPU'
    dev = torch.device('cuda', torch.cuda.current_device())
    al_h, tl_h = s1_alignments()
    al, tl = torch.tensor(al_h, device=dev), torch.tensor(tl_h, device=dev)
    counts = torch.empty(B, len(lib.ALIGN_COUNTS), dtype=torch.int32, device=dev)
    means = torch.empty(B, len(lib.ALIGN_MEANS), device=dev)
    host = {}

    def device_call():
        lib.alignment_scores(al, tl, None, lib.MAX_JUMP, counts, means)

    def device_burst():
        for _ in range(BURST):
            device_call()

    def device_path():   # what the driver does at a log step: the call, then 8 values per row to the host
        device_call()
        host['device'] = (counts.cpu().numpy(), means.cpu().numpy())

    def host_copy():
        host['al'] = al.cpu().numpy()

    def host_path():   # what it replaces: the alignment tensor to the host, then the scores in NumPy
        host_copy()
        host['host'] = align_ref.scores(host['al'], tl_h, None, lib.MAX_JUMP)

    res = {'tool': 'alignment_scores_timing', 'B': B, 'Td': TD, 'Tt': TT, 'max_jump': lib.MAX_JUMP, 'reps': a.reps, 'warmup': a.warmup,
           'version': lib.version(), 'unit': 'ms per call (median; variants alternate inside each repetition)'}
    res['events'] = alternate({'taco_alignment_scores': device_call, 'taco_alignment_scores_x%d' % BURST: device_burst}, a.reps, a.warmup)
    res['events']['taco_alignment_scores_steady'] = res['events'].pop('taco_alignment_scores_x%d' % BURST) / BURST
    res['wall'] = wall({'device_call': device_call, 'device_call_and_copy_back': device_path, 'host_copy_of_the_alignments': host_copy,
                        'host_copy_and_numpy_scores': host_path}, a.reps, a.warmup)
    (dc, dm), (hc, hm) = host['device'], host['host']
    same = bool(np.array_equal(dc, hc) and np.abs(dm.astype(np.float64) - hm).max() <= align_ref.means_bound(TD, TT))
    res['device_equals_host'] = same
    nbytes = 4.0 * B * TD * TT
    res['checks'] = {'bytes_read': nbytes, 'steady_gb_per_s': nbytes / (res['events']['taco_alignment_scores_steady'] * 1e-3) / 1e9,
                     'host_path_over_device_path': res['wall']['host_copy_and_numpy_scores'] / res['wall']['device_call_and_copy_back'],
                     'bytes_back_host_path': nbytes, 'bytes_back_device_path': 4.0 * B * 8}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, 'alignment_scores_timing.json'), 'w') as f:
            f.write(line + '\n')
    return 0 if same else 1


if __name__ == '__main__':
    sys.exit(main())
