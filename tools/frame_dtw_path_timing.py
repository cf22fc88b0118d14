"""What the warping path costs on the device (taco_frame_dtw_path against taco_frame_dtw, the yardstick, timed in the same run) and
what the aligned F0 scores cost (taco_path_f0_scores), against the host path they replace: both frame tensors and both period
tracks copied back over PCIe, then the walk with its direction table and the scores in NumPy (tests/path_ref.py, the restatement
the GPU tests compare against bit for bit).

The cases are those of tools/frame_dtw_timing.py: one S1-shaped batch, B = 32, Fa = Fb = 360 frames of C = 80 mel bands, K = 13
DCT coefficients, every row at full length, and the S2 envelope Fa = Fb = 1000.  The device calls are timed with device events,
alone and per call of 10 back to back; the variants alternate inside each repetition and the median is reported.  The path call's
time over the cost-only call's is the cost of the direction stores plus the backtrack.  The backtrack alone is separated on ONE
row of 360 x 360 whose walk is the same 719 diagonals in both variants and whose path is not: a sequence against itself (the
diagonal: 360 cells) and a pair built so that the only free path runs along the table's edge (718 cells); the difference over 358
is one step of the backtrack -- one dependent load -- and the diagonal row's time over the cost-only row's bounds the stores.
`taco_frame_dtw_over_parent` compares the yardstick itself with profiles/frame_dtw_timing.json as the parent commit recorded it: the
cost-only kernel's instructions did not change with the path form, so this ratio is run-to-run spread and nothing else.

    python tools/frame_dtw_path_timing.py [--reps 20] [--host-reps 3] [--warmup 3] [--out DIR]

Prints one JSON line; with --out also writes it to DIR/frame_dtw_path_timing.json.  No pass mark: the exit status is 0 unless a call
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
from tests import path_cases, path_ref  # noqa: E402
from tools.frame_dtw_timing import frames  # noqa: E402
from tools.griffinlim_timing import alternate  # noqa: E402
from tools.wave_join_timing import wall  # noqa: E402

B, C, K, BURST, GROSS = 32, 80, 13, 10, 1.2


def edge_pair(F):
    """(a, b) (1, F, C): a = [0, x, x, ..], b = [0, .., 0, x] with x a frame the cepstra see (a cosine over the channels; a constant
    one has no coefficient behind c0) -- the free cells are row 0 up to column F - 2 and column F - 1 from row 1 on, every other
    cell costs |x|, so the path has 2 F - 2 cells"""
    x = np.cos(np.pi * (np.arange(C) + 0.5) / C).astype(np.float32)
    a, b = np.tile(x, (1, F, 1)), np.zeros((1, F, C), dtype=np.float32)
    a[0, 0], b[0, F - 1] = 0.0, x
    return a, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--host-reps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'frame_dtw_path_timing needs a GPU'
    dev = torch.device('cuda', torch.cuda.current_device())
    rng = np.random.default_rng(0)
    basis_h = lib.dct_basis(C, 1, K)
    basis = torch.tensor(basis_h, device=dev)

    def tensors(a_h, b_h):
        n, Fa, Fb = a_h.shape[0], a_h.shape[1], b_h.shape[1]
        return {'a_h': a_h, 'b_h': b_h, 'a': torch.tensor(a_h, device=dev), 'b': torch.tensor(b_h, device=dev),
                'cost': torch.empty(n, device=dev), 'steps': torch.empty(n, dtype=torch.int32, device=dev),
                'path_a': torch.empty(n, Fa + Fb - 1, dtype=torch.int32, device=dev),
                'path_b': torch.empty(n, Fa + Fb - 1, dtype=torch.int32, device=dev),
                'work0': torch.empty(lib.frame_dtw_workspace_bytes(n, Fa, Fb, K), dtype=torch.uint8, device=dev),
                'work': torch.empty(lib.frame_dtw_path_workspace_bytes(n, Fa, Fb, K), dtype=torch.uint8, device=dev)}

    t = {F: tensors(frames(rng, F), frames(rng, F)) for F in (360, 1000)}
    one = frames(rng, 360)[:1]
    t['diag'] = tensors(one, one.copy())
    t['edge'] = tensors(*edge_pair(360))
    per_h = {'a': path_cases.periods(rng, B, 360), 'b': path_cases.periods(rng, B, 360)}
    per = {k: torch.tensor(v, device=dev) for k, v in per_h.items()}
    counts, means = torch.empty(B, 5, dtype=torch.int32, device=dev), torch.empty(B, 2, device=dev)

    def cost_call(k):
        x = t[k]
        return lambda: lib.frame_dtw(x['a'], x['b'], None, None, basis, x['cost'], x['steps'], x['work0'])

    def path_call(k):
        x = t[k]
        return lambda: lib.frame_dtw_path(x['a'], x['b'], None, None, basis, x['cost'], x['steps'], x['path_a'], x['path_b'], x['work'])

    def scores_call():
        x = t[360]
        lib.path_f0_scores(per['a'], per['b'], x['path_a'], x['path_b'], x['steps'], GROSS, counts, means)

    def burst(fn):
        def run():
            for _ in range(BURST):
                fn()
        return run

    host = {}

    def device_path():   # what the driver does per batch: the two calls, then 8 values per row to the host
        path_call(360)()
        scores_call()
        host['device'] = (counts.cpu().numpy(), means.cpu().numpy(), t[360]['steps'].cpu().numpy())

    def host_copy():
        host['in'] = (t[360]['a'].cpu().numpy(), t[360]['b'].cpu().numpy(), per['a'].cpu().numpy(), per['b'].cpu().numpy())

    def host_path():     # what it replaces: frames and periods to the host, the walk with its table and the scores in NumPy
        host_copy()
        fa, fb, pa, pb = host['in']
        _, steps, path_a, path_b = path_ref.dtw32_path(fa, fb, None, None, basis_h)
        host['host'] = path_ref.path_scores(pa, pb, path_a, path_b, steps, GROSS) + (steps, path_a, path_b)

    res = {'tool': 'frame_dtw_path_timing', 'B': B, 'C': C, 'K': K, 'reps': a.reps, 'host_reps': a.host_reps, 'warmup': a.warmup,
           'version': lib.version(), 'unit': 'ms per call (median; variants alternate inside each repetition)',
           'backtrack': 'one lane, one dependent load per step (the tiled form is not built)',
           'workspace_bytes_per_row': {'360': lib.frame_dtw_path_workspace_bytes(1, 360, 360, K),
                                       '1000': lib.frame_dtw_path_workspace_bytes(1, 1000, 1000, K)}}
    fns = {}
    for k in (360, 1000):
        fns['taco_frame_dtw_%d' % k], fns['taco_frame_dtw_path_%d' % k] = cost_call(k), path_call(k)
        fns['taco_frame_dtw_%d_x%d' % (k, BURST)], fns['taco_frame_dtw_path_%d_x%d' % (k, BURST)] = burst(cost_call(k)), burst(path_call(k))
    for k in ('diag', 'edge'):
        fns['one_row_cost_%s_x%d' % (k, BURST)], fns['one_row_path_%s_x%d' % (k, BURST)] = burst(cost_call(k)), burst(path_call(k))
    path_call(360)()     # (the scores read this call's path)
    fns['taco_path_f0_scores_360'], fns['taco_path_f0_scores_360_x%d' % BURST] = scores_call, burst(scores_call)
    ev = alternate(fns, a.reps, a.warmup)
    for k in [k for k in ev if k.endswith('_x%d' % BURST)]:
        ev[k[:-len('_x%d' % BURST)] + '_steady'] = ev.pop(k) / BURST
    res['events'] = ev
    res['wall'] = wall({'device_calls_and_copy_back': device_path, 'host_copy_of_frames_and_periods': host_copy}, a.reps, a.warmup)
    res['wall'].update(wall({'host_copy_and_numpy_path_and_scores': host_path}, a.host_reps, 1))
    (dc, dm, dn), (hc, hm, hn, hpa, hpb) = host['device'], host['host']
    same = bool(np.array_equal(dc, hc) and np.array_equal(dn, hn) and np.array_equal(t[360]['path_a'].cpu().numpy(), hpa)
                and np.array_equal(t[360]['path_b'].cpu().numpy(), hpb)
                and np.abs(dm.astype(np.float64) - hm).max() <= path_ref.PATH_SCORES_ATOL)
    res['device_equals_host'] = same
    steps = {k: int(t[k]['steps'][0]) for k in ('diag', 'edge')}
    per_step = 1e3 * (ev['one_row_path_edge_steady'] - ev['one_row_path_diag_steady']) / (steps['edge'] - steps['diag'])
    mean_steps = {k: float(t[k]['steps'].double().mean()) for k in (360, 1000)}
    parent = None
    try:
        with open(os.path.join(ROOT, 'profiles', 'frame_dtw_timing.json')) as f:
            parent = json.load(f)['events']
    except (OSError, ValueError, KeyError):
        pass
    res['checks'] = {
        'path_over_cost_360': ev['taco_frame_dtw_path_360_steady'] / ev['taco_frame_dtw_360_steady'],
        'path_over_cost_1000': ev['taco_frame_dtw_path_1000_steady'] / ev['taco_frame_dtw_1000_steady'],
        'one_row_steps': steps,
        'backtrack_us_per_step': per_step,
        'one_row_stores_and_360_steps_us': 1e3 * (ev['one_row_path_diag_steady'] - ev['one_row_cost_diag_steady']),
        'mean_steps': mean_steps,
        'backtrack_share_of_the_added_time_360': per_step * mean_steps[360]
        / (1e3 * (ev['taco_frame_dtw_path_360_steady'] - ev['taco_frame_dtw_360_steady'])),
        'backtrack_share_of_the_path_call_360': per_step * mean_steps[360] / (1e3 * ev['taco_frame_dtw_path_360_steady']),
        'taco_frame_dtw_over_parent': None if parent is None else {
            '360': ev['taco_frame_dtw_360_steady'] / parent['taco_frame_dtw_360_steady'],
            '1000': ev['taco_frame_dtw_1000_steady'] / parent['taco_frame_dtw_1000_steady']},
        'host_path_over_device_path': res['wall']['host_copy_and_numpy_path_and_scores'] / res['wall']['device_calls_and_copy_back'],
        'bytes_back_host_path': 2 * 4.0 * B * 360 * C + 2 * 4.0 * B * 360, 'bytes_back_device_path': 32.0 * B}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, 'frame_dtw_path_timing.json'), 'w') as f:
            f.write(line + '\n')
    return 0 if same else 1


if __name__ == '__main__':
    sys.exit(main())
