"""What prosody inside an utterance costs: the three curve entry points at the Nancy shape (B = 32, C = 1025, F = 360 and 720), each
next to its constant sibling at the same bytes.

  taco_frames_stretch_curve with every duration 131072 (rate 0.5)  beside  taco_frames_stretch at step 32768 -- the same map, the
      same bits (checked), so what differs is the map launch and the gather reading its positions instead of forming them.  The two
      launches are not separable through the C ABI, so the map is timed as the call at C = 1 (the map launch plus a one-bin gather)
      and the gather as the difference to the whole call;
  taco_frames_pitch_curve with every step 55109 (+3 semitones)     beside  taco_frames_pitch at that row step -- the same bits (checked);
  taco_path_curve (B x 72 | 144 steps x r = 5 frames, Tt = 140);
  the torch-ops form of the stretch curve a user would otherwise write: cumsum, searchsorted, two index_select, lerp (one curve
      for the whole batch -- index_select has no per-row form; the kernel takes a curve per row).

Method of tools/frames_stretch_timing.py: device events around --calls (>= 200) calls after warm-up, enqueued behind a kernel that
holds the stream for --hold-ms, the forms ALTERNATING --reps (>= 5) times in the one process; reported per call: the median over the
repetitions and their spread (max - min).  A ratio is "above the spread" when the difference of the medians exceeds the larger of the
two spreads.

    python tools/frames_curve_timing.py [--reps 7] [--calls 200] [--out DIR]

Prints one JSON line; with --out also writes it to DIR/frames_curve_timing.json.  No pass mark: exit status 0 unless a call fails."""
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

B, C, R, TT = 32, 1025, 5, 140
FRAMES = (360, 720)
RATE, SEMITONES = 0.5, 3.0


def med_spread(v):
    return {'median': float(np.median(v)), 'spread': float(np.max(v) - np.min(v)), 'all': [float(x) for x in v]}


def time_calls(fn, calls, hold_ms):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if hold_ms > 0:
        lib.debug_spin(1, 64, 0, int(hold_ms * 1000))
    s.record()
    for _ in range(calls):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / calls


def alternate(a, forms):
    ts = {k: [] for k in forms}
    for _ in range(a.warmup):
        for fn in forms.values():
            time_calls(fn, a.calls, 0.0)
    for _ in range(a.reps):
        for k, fn in forms.items():
            ts[k].append(time_calls(fn, a.calls, a.hold_ms))
    return {k: med_spread(v) for k, v in ts.items()}


def ratio(res, num, den):
    """(median ratio, whether the difference of the medians exceeds the larger spread of the two)"""
    x, y = res[num], res[den]
    return {'ratio': x['median'] / y['median'], 'above_spread': bool(abs(x['median'] - y['median']) > max(x['spread'], y['spread']))}


def one_shape(a, F, dev):
    g = torch.Generator(device='cpu').manual_seed(3)
    x = torch.exp(torch.randn(B, C, F, generator=g) * 2.0).to(dev)
    dur, step = lib.stretch_dur(RATE), lib.stretch_step(RATE)
    Fo = lib.stretch_curve_capacity(F, dur)
    assert Fo == lib.stretch_capacity(F, step)
    durs = torch.full((B, F), dur, dtype=torch.int32, device=dev)
    steps = torch.full((B,), step, dtype=torch.int32, device=dev)
    out, out2 = (torch.empty(B, C, Fo, dtype=torch.float32, device=dev) for _ in range(2))
    n, n2 = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(2))
    src = torch.empty(B, Fo, dtype=torch.int32, device=dev)
    x1, out1 = x[:, :1, :].contiguous(), torch.empty(B, 1, Fo, dtype=torch.float32, device=dev)
    d1 = durs[0].to(torch.int64)

    def curve():
        return lib.frames_stretch_curve(x, None, durs, out=out, frames_out=n, src=src)

    def constant():
        return lib.frames_stretch(x, None, steps, out=out2, frames_out=n2)

    def map_one_bin():
        return lib.frames_stretch_curve(x1, None, durs, out=out1, frames_out=n, src=src)

    def torch_ops():
        D = torch.cumsum(d1, 0) - d1
        q = torch.arange(Fo, dtype=torch.int64, device=dev) << 16
        i = torch.searchsorted(D, q, right=True) - 1
        w = (((q - D[i]) << 16) // d1[i]).to(torch.float32) * (2.0 ** -16)
        lo, hi = torch.index_select(x, 2, i), torch.index_select(x, 2, torch.clamp(i + 1, max=F - 1))
        return torch.lerp(lo, hi, w)

    same = bool(torch.equal(curve()[0].view(torch.int32), constant()[0].view(torch.int32)) and torch.equal(n, n2))
    torch_diff = float((torch_ops() - out).abs().max())
    res = alternate(a, {'frames_stretch_curve': curve, 'frames_stretch': constant, 'map_and_one_bin': map_one_bin, 'torch_ops': torch_ops})
    nbytes = 4 * B * C * (F + Fo)
    for k in ('frames_stretch_curve', 'frames_stretch', 'torch_ops'):
        res[k]['gb_per_s'] = nbytes / (res[k]['median'] * 1e-3) / 1e9
    stretch = {'dur_q': dur, 'step_q': step, 'Fo': Fo, 'bytes_to_move': nbytes, 'curve_bits_equal_constant': same,
               'torch_max_abs_difference': torch_diff, 'unit': 'ms per call', **res,
               'gather_by_difference': res['frames_stretch_curve']['median'] - res['map_and_one_bin']['median'],
               'curve_over_constant': ratio(res, 'frames_stretch_curve', 'frames_stretch'),
               'torch_over_curve': ratio(res, 'torch_ops', 'frames_stretch_curve')}

    pstep = lib.pitch_step(SEMITONES)
    psteps = torch.full((B, F), pstep, dtype=torch.int32, device=dev)
    prow = torch.full((B,), pstep, dtype=torch.int32, device=dev)
    po, po2 = (torch.empty(B, C, F, dtype=torch.float32, device=dev) for _ in range(2))

    def pcurve():
        return lib.frames_pitch_curve(x, None, psteps, out=po)

    def pconst():
        return lib.frames_pitch(x, None, prow, out=po2)

    psame = bool(torch.equal(pcurve().view(torch.int32), pconst().view(torch.int32)))
    res = alternate(a, {'frames_pitch_curve': pcurve, 'frames_pitch': pconst})
    pitch = {'step_q': pstep, 'lifter': 32, 'curve_bits_equal_constant': psame, 'unit': 'ms per call', **res,
             'curve_over_constant': ratio(res, 'frames_pitch_curve', 'frames_pitch')}

    Td = F // R
    path = (torch.arange(Td, device=dev) * TT // Td).to(torch.int32).repeat(B, 1).contiguous()
    values = torch.randint(16384, 262145, (B, TT), generator=g).to(torch.int32).to(dev)
    cv = torch.empty(B, Td * R, dtype=torch.int32, device=dev)
    res = alternate(a, {'path_curve': lambda: lib.path_curve(path, values, R, 65536, curve=cv)})
    return {'F': F, 'stretch': stretch, 'pitch': pitch, 'path': {'Td': Td, 'r': R, 'Tt': TT, 'unit': 'ms per call', **res}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--hold-ms', type=float, default=20.0)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'frames_curve_timing needs a GPU'
    assert a.reps >= 5 and a.calls >= 200, 'at least 5 alternations of at least 200 calls'
    dev = torch.device('cuda', torch.cuda.current_device())
    res = {'tool': 'frames_curve_timing', 'B': B, 'C': C, 'rate': RATE, 'semitones': SEMITONES, 'reps': a.reps, 'warmup': a.warmup,
           'calls': a.calls, 'hold_ms': a.hold_ms, 'version': lib.version(), 'device': torch.cuda.get_device_name(dev),
           'shapes': [one_shape(a, F, dev) for F in FRAMES]}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, 'frames_curve_timing.json'), 'w') as f:
            f.write(line + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
