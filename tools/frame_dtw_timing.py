"""Time of the dynamic-time-warping distance on the device (taco_frame_dtw, as tacotron_amd.evaluate calls it once per batch) against
the host path it replaces: the two (B, F, 80) frame tensors copied back over PCIe, then the same recurrence in NumPy, vectorised by
anti-diagonal (tests/dtw_ref.py, the float32 restatement the GPU tests compare against bit for bit).

The case is one S1-shaped batch: B = 32, Fa = Fb = 360 chronological frames of C = 80 mel bands, K = 13 DCT coefficients, every
row at full length (the worst case of the walk: 719 anti-diagonals).  The S2 envelope, Fa = Fb = 1000, is timed on the device as
well, and taco_frames_active next to it.  The device calls are timed with device events, alone and per call of 10 back to back (the
single-call figure carries the launch latency of an idle queue); the host path has no device events and is timed by the host clock
around a synchronised call, and so is the device call with its 2 B result values copied back, for a like comparison.  The variants
alternate inside each repetition and the median is reported; the NumPy walk takes seconds, so it gets --host-reps of its own.
`us_per_diagonal` is the steady time of the 360 x 360 call over its 719 diagonals: what a barrier-free path for diagonals no longer
than a wave (not built) would have to beat on the 2 x 63 short diagonals at the table's corners.

    python tools/frame_dtw_timing.py [--reps 20] [--host-reps 3] [--warmup 3] [--out DIR]

Prints one JSON line; with --out also writes it to DIR/frame_dtw_timing.json.  No pass mark: the exit status is 0 unless a call
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
from tests import dtw_ref  # noqa: E402
from tools.griffinlim_timing import alternate  # noqa: E402
from tools.wave_join_timing import wall  # noqa: E402

B, C, K, BURST = 32, 80, 13, 10


def frames(rng, F):
    """smooth log-mel-like frames: a random walk over the frames around -5"""
    return (np.cumsum(rng.standard_normal((B, F, C)) * 0.3, axis=1) - 5.0).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--host-reps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'frame_dtw_timing needs a GPU'
    dev = torch.device('cuda', torch.cuda.current_device())
    rng = np.random.default_rng(0)
    basis_h = lib.dct_basis(C, 1, K)
    basis = torch.tensor(basis_h, device=dev)
    host, calls = {}, {}
    t = {}
    for F in (360, 1000):
        a_h, b_h = frames(rng, F), frames(rng, F)
        t[F] = {'a_h': a_h, 'b_h': b_h, 'a': torch.tensor(a_h, device=dev), 'b': torch.tensor(b_h, device=dev),
                'cost': torch.empty(B, device=dev), 'steps': torch.empty(B, dtype=torch.int32, device=dev),
                'n': torch.empty(B, dtype=torch.int32, device=dev),
                'work': torch.empty(lib.frame_dtw_workspace_bytes(B, F, F, K), dtype=torch.uint8, device=dev)}

    def device_call(F):
        x = t[F]
        return lambda: lib.frame_dtw(x['a'], x['b'], None, None, basis, x['cost'], x['steps'], x['work'])

    def burst(fn):
        def run():
            for _ in range(BURST):
                fn()
        return run

    def active_call():
        lib.frames_active(t[360]['b'], -18.0, t[360]['n'])

    def device_path():   # what the driver does per batch: the call, then 2 values per row to the host
        device_call(360)()
        host['device'] = (t[360]['cost'].cpu().numpy(), t[360]['steps'].cpu().numpy())

    def host_copy():
        host['a'], host['b'] = t[360]['a'].cpu().numpy(), t[360]['b'].cpu().numpy()

    def host_path():   # what it replaces: both frame tensors to the host, then the warp in NumPy
        host_copy()
        host['host'] = dtw_ref.dtw32(host['a'], host['b'], None, None, basis_h)

    res = {'tool': 'frame_dtw_timing', 'B': B, 'C': C, 'K': K, 'reps': a.reps, 'host_reps': a.host_reps, 'warmup': a.warmup,
           'version': lib.version(), 'unit': 'ms per call (median; variants alternate inside each repetition)',
           'barrier_free_short_diagonals': 'not built'}
    ev = alternate({'taco_frame_dtw_360': device_call(360), 'taco_frame_dtw_360_x%d' % BURST: burst(device_call(360)),
                    'taco_frame_dtw_1000': device_call(1000), 'taco_frame_dtw_1000_x%d' % BURST: burst(device_call(1000)),
                    'taco_frames_active_360': active_call, 'taco_frames_active_360_x%d' % BURST: burst(active_call)}, a.reps, a.warmup)
    for k in ('taco_frame_dtw_360', 'taco_frame_dtw_1000', 'taco_frames_active_360'):
        ev[k + '_steady'] = ev.pop('%s_x%d' % (k, BURST)) / BURST
    res['events'] = ev
    res['wall'] = wall({'device_call': device_call(360), 'device_call_and_copy_back': device_path,
                        'host_copy_of_the_frames': host_copy}, a.reps, a.warmup)
    res['wall'].update(wall({'host_copy_and_numpy_dtw': host_path}, a.host_reps, 1))
    (dc, dn), (hc, hn) = host['device'], host['host']
    same = bool(np.array_equal(dc.view(np.uint32), hc.view(np.uint32)) and np.array_equal(dn, hn))
    res['device_equals_host'] = same
    res['checks'] = {'us_per_diagonal_360': 1e3 * ev['taco_frame_dtw_360_steady'] / 719,
                     'us_per_diagonal_1000': 1e3 * ev['taco_frame_dtw_1000_steady'] / 1999,
                     'cells_per_us_360': B * 360 * 360 / (1e3 * ev['taco_frame_dtw_360_steady']),
                     'host_path_over_device_path': res['wall']['host_copy_and_numpy_dtw'] / res['wall']['device_call_and_copy_back'],
                     'bytes_back_host_path': 2 * 4.0 * B * 360 * C, 'bytes_back_device_path': 8.0 * B}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, 'frame_dtw_timing.json'), 'w') as f:
            f.write(line + '\n')
    return 0 if same else 1


if __name__ == '__main__':
    sys.exit(main())
