"""Wall time of joining the finished pieces of long prompts on the device (taco_wave_join, PCM16 only, as the driver's --long calls
it) against the host path it replaces: the N finished fp32 rows copied back over PCIe, then the join in NumPy (tests/join_ref.py, the
restatement the GPU tests compare against: offsets, ramps, peak, PCM16).

The shape: 8 prompts of 4 pieces at the flagship inference length L = 300 (360 - 1) = 107,700 samples; every piece keeps 60,000 to
107,700 samples; 300 / 150 / 0 ms pauses and 5 ms ramps at 16 kHz (the driver's defaults); Lj is the binding's default (worst case).
Both paths are timed by the host clock around a synchronised call, because the host path has no device events; the device call is
also timed with device events, alone and per call of 20 back to back (one call is tens of microseconds: the single-call figure carries
the launch latency of an idle queue).  The variants alternate inside each repetition and the median over --reps is reported.

    python tools/wave_join_timing.py [--reps 20] [--warmup 3] [--out DIR]

Prints one JSON line; with --out also writes it to DIR/wave_join_timing.json.  No pass mark: the exit status is 0 unless a call fails
or the two paths disagree."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tacotron_amd import data, lib  # noqa: E402
from tacotron_amd.griffinlim import join_gaps, join_samples  # noqa: E402
from tests import join_ref  # noqa: E402
from tools.griffinlim_timing import alternate  # noqa: E402

P, K, F, BURST = 8, 4, 360, 20


def wall(fns, reps, warmup):
    """{name: median ms by the host clock}: each repetition runs every callable once, in order, the device idle before and after"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[k].append(1e3 * (time.perf_counter() - t0))
    return {k: float(np.median(v)) for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'wave_join_timing needs a GPU'
    dev = torch.device('cuda', torch.cuda.current_device())
    N, L = P * K, 300 * (F - 1)
    rng = np.random.default_rng(5)
    lens = rng.integers(60000, L + 1, size=N)
    x = torch.tensor((0.4 * rng.standard_normal((N, L))).astype(np.float32), device=dev)
    bounds = torch.tensor(np.stack([np.zeros(N, np.int64), lens], axis=1), dtype=torch.int32, device=dev)
    first = [K * p for p in range(P + 1)]
    kinds = [(data.SENTENCE, data.CLAUSE, data.WORD, data.END)[i % K] for i in range(N)]
    gap, fade = join_gaps(kinds), join_samples(5.0)
    Lj = -(-(K * L + max(sum(gap[first[p]:first[p + 1] - 1]) for p in range(P))) // 8) * 8
    pcm = torch.empty(P, Lj, dtype=torch.int16, device=dev)
    offsets = torch.empty(N, dtype=torch.int32, device=dev)
    total = torch.empty(P, dtype=torch.int32, device=dev)
    peak = torch.empty(P, device=dev)
    work = torch.empty(lib.wave_join_workspace_bytes(N, P, Lj), dtype=torch.uint8, device=dev)
    host = {}

    def device_join():
        lib.wave_join(x, bounds, first, gap, fade=fade, Lj=Lj, want_out=False, pcm=pcm, offsets=offsets, total=total, peak=peak, work=work)

    def device_burst():
        for _ in range(BURST):
            device_join()

    def device_path():   # what the driver does: the join, then pcm, total and offsets to the host
        device_join()
        host['device'] = (pcm.cpu().numpy(), total.cpu().numpy(), offsets.cpu().numpy())

    def host_copy():
        host['rows'] = (x.cpu().numpy(), bounds.cpu().numpy())

    def host_path():   # what it replaces: the N fp32 rows and their bounds to the host, then the join in NumPy
        host_copy()
        host['host'] = join_ref.join(host['rows'][0], host['rows'][1], first, gap, fade, Lj)

    res = {'tool': 'wave_join_timing', 'P': P, 'pieces_per_prompt': K, 'N': N, 'L': L, 'Lj': Lj, 'fade': fade, 'gap': gap[:K],
           'reps': a.reps, 'warmup': a.warmup, 'version': lib.version(),
           'unit': 'ms per call (median; variants alternate inside each repetition)'}
    res['events'] = alternate({'taco_wave_join': device_join, 'taco_wave_join_x%d' % BURST: device_burst}, a.reps, a.warmup)
    res['events']['taco_wave_join_steady'] = res['events'].pop('taco_wave_join_x%d' % BURST) / BURST
    res['wall'] = wall({'device_join': device_join, 'device_join_and_copy_back': device_path, 'host_copy_of_the_rows': host_copy,
                        'host_copy_and_numpy_join': host_path}, a.reps, a.warmup)
    d, h = host['device'], host['host']
    same = bool(np.array_equal(d[0], h[1]) and np.array_equal(d[1], h[3]) and np.array_equal(d[2], h[2]))
    res['device_equals_host'] = same
    kept = float(lens.sum())
    # bytes the device call has to move: the kept samples read, the joined fp32 rows written and read again, int16 written
    nbytes = 4.0 * kept + (4.0 + 4.0 + 2.0) * P * Lj
    res['checks'] = {'bytes_moved': nbytes, 'steady_gb_per_s': nbytes / (res['events']['taco_wave_join_steady'] * 1e-3) / 1e9,
                     'host_path_over_device_path': res['wall']['host_copy_and_numpy_join'] / res['wall']['device_join_and_copy_back'],
                     'bytes_back_host_path': 4.0 * N * L, 'bytes_back_device_path': 2.0 * P * Lj}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, 'wave_join_timing.json'), 'w') as f:
            f.write(line + '\n')
    return 0 if same else 1


if __name__ == '__main__':
    sys.exit(main())
