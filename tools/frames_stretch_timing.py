"""What the speaking-rate stretch costs: taco_frames_stretch alone at the Nancy shape (B = 32, C = 1025, F = 360) for rates 0.5, 1.0
and 2.0, against the same stretch as torch ops on the device -- two index_select along the frame axis plus the arithmetic, what a user
has without the entry point -- and, for proportion, the Griffin-Lim call it feeds at the stretched length.

Both forms are timed with device events around --calls (>= 200) calls after warm-up, enqueued behind a kernel that holds the stream
for --hold-ms so that they are all queued when the clock starts, and ALTERNATE --reps (>= 5) times in the one process; reported per
call: the median over the repetitions and their spread (max - min).  The bytes the stretch must move come from the shapes: every
source frame read once (B C F floats: a gather fetches whole lines, also where a fast rate skips frames) and every output frame
written once (B C Fo floats); gb_per_s is that over the median.  The working set (47 MB in, 24 to 94 MB out) fits the 256 MiB
Infinity Cache, so the rate is not an HBM rate.  The torch form's result is compared with the kernel's, bit for bit.

    python tools/frames_stretch_timing.py [--reps 7] [--calls 200] [--gl-reps 3] [--out DIR]

Prints one JSON line; with --out also writes it to DIR/frames_stretch_timing.json.  No pass mark: exit status 0 unless a call fails."""
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

B, C, F = 32, 1025, 360
RATES = (0.5, 1.0, 2.0)


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


def one_rate(a, x, rate, dev):
    step = lib.stretch_step(rate)
    Fo = lib.stretch_capacity(F, step)
    steps = torch.full((B,), step, dtype=torch.int32, device=dev)
    out = torch.empty(B, C, Fo, dtype=torch.float32, device=dev)
    n = torch.empty(B, dtype=torch.int32, device=dev)
    p = torch.arange(Fo, dtype=torch.int64, device=dev) * step
    i0, frac = p >> 16, p & 0xFFFF
    i1 = torch.clamp(i0 + 1, max=F - 1)
    w = frac.to(torch.float32) * (2.0 ** -16)

    def kernel():
        return lib.frames_stretch(x, None, steps, out=out, frames_out=n)

    def torch_ops():
        lo, hi = torch.index_select(x, 2, i0), torch.index_select(x, 2, i1)
        return lo + w * (hi - lo)

    same = bool(torch.equal(kernel()[0].view(torch.int32), torch_ops().view(torch.int32)))
    forms = {'frames_stretch': kernel, 'torch_index_select': torch_ops}
    ts = {k: [] for k in forms}
    for _ in range(a.warmup):
        for fn in forms.values():
            time_calls(fn, a.calls, 0.0)
    for _ in range(a.reps):
        for k, fn in forms.items():
            ts[k].append(time_calls(fn, a.calls, a.hold_ms))
    nbytes = 4 * B * C * (F + Fo)
    res = {'rate': rate, 'step_q': step, 'Fo': Fo, 'bytes_to_move': nbytes,
           'torch_bits_equal': same, 'unit': 'ms per call'}
    for k, v in ts.items():
        res[k] = med_spread(v)
        res[k]['gb_per_s'] = nbytes / (res[k]['median'] * 1e-3) / 1e9
    res['torch_over_kernel'] = res['torch_index_select']['median'] / res['frames_stretch']['median']
    # the Griffin-Lim call the stretched matrix goes to: 50 rounds over the device's frames_out
    work = torch.empty(lib.griffinlim_rows_workspace_floats(B, Fo), dtype=torch.float32, device=dev)
    wave = torch.empty(B, 300 * (Fo - 1), dtype=torch.float32, device=dev)
    gl = []
    for rep in range(1 + a.gl_reps):   # (the first one is the warm-up)
        t = time_calls(lambda: lib.griffinlim_rows(out, n, seed=0, n_iter=50, out=wave, work=work), 1, 0.0)
        if rep:
            gl.append(t)
    res['griffinlim_rows_50_rounds'] = med_spread(gl)
    res['stretch_share_of_griffinlim'] = res['frames_stretch']['median'] / res['griffinlim_rows_50_rounds']['median']
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
    assert torch.cuda.is_available(), 'frames_stretch_timing needs a GPU'
    assert a.reps >= 5 and a.calls >= 200, 'at least 5 alternations of at least 200 calls'
    dev = torch.device('cuda', torch.cuda.current_device())
    g = torch.Generator(device='cpu').manual_seed(3)
    x = torch.exp(torch.randn(B, C, F, generator=g) * 2.0).to(dev)
    res = {'tool': 'frames_stretch_timing', 'B': B, 'C': C, 'F': F, 'reps': a.reps, 'warmup': a.warmup, 'calls': a.calls,
           'hold_ms': a.hold_ms, 'version': lib.version(), 'device': torch.cuda.get_device_name(dev),
           'other_forms': 'profiles/frames_stretch_store_forms.txt (two forms with 16-byte stores, measured and deleted); LDS staging of the source: not built', 'rates': [one_rate(a, x, rate, dev) for rate in RATES]}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, 'frames_stretch_timing.json'), 'w') as f:
            f.write(line + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
