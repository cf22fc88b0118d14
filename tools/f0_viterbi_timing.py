"""What smoothing a pitch track costs: taco_f0_viterbi at the Nancy lag count (B = 32, L = 229: lags 40 .. 266 with their neighbours)
for F = 360 and F = 720 frames and K = 4 and K = 15 candidates per frame, on the acf of seeded magnitude frames, against
  - taco_frames_f0 with its acf output on the same shape (C = 1025): the call that has to run in front of it;
  - copying acf back to the host and running the NumPy restatement vectorised over the rows (tests/f0_viterbi_ref.py: candidates and
    best_path over (B, L, F) at once): what a user has without the entry point.  It runs --host-reps times, not --reps x --calls.
Its two launches are timed separately from the kernels' own durations as torch.profiler records them over --calls calls (the
candidate kernel, B x ceil(F / 32) workgroups; the path kernel, one wave per row walking a chain of F dependent steps).  The rows run
side by side, so us_per_frame, the path kernel's duration over F, is what a STEP of that chain costs.  Where the profiler gives no
kernel records the split is null and `split_error` says why.

The device forms are timed with device events around --calls (>= 200) calls after warm-up, enqueued behind a kernel that holds the
stream for --hold-ms so that they are all queued when the clock starts, and ALTERNATE --reps (>= 5) times in the one process;
reported per call: the median over the repetitions and their spread (max - min).

    python tools/f0_viterbi_timing.py [--reps 7] [--calls 200] [--out DIR]

Prints one JSON line; with --out also writes it to DIR/f0_viterbi_timing.json.  No pass mark: exit status 0 unless a call fails."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tacotron_amd import lib  # noqa: E402
from tests import f0_viterbi_ref as vr  # noqa: E402

B, C = 32, 1025
FRAMES = (360, 720)
CANDIDATES = (4, 15)
KERNELS = ('f0_candidates_kernel', 'f0_path_kernel')


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


def kernel_split(fn, calls):
    """mean device duration in ms of each of the call's two kernels over `calls` calls, from torch.profiler"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    out = {}
    for name in KERNELS:
        hits = [ev for ev in prof.key_averages() if name in ev.key]
        if not hits:
            raise RuntimeError('the profiler recorded no %s' % name)
        total = sum(getattr(ev, 'device_time_total', None) or getattr(ev, 'cuda_time_total', 0.0) for ev in hits)
        out[name] = total / sum(ev.count for ev in hits) / 1e3
    return out


def host_form(acf, bias, lg, K, threshold, jump, switch):
    """the device-to-host copy of acf and the restatement over all rows at once; returns the closure"""
    def run():
        y = acf.cpu().numpy()
        idx, v = vr.candidates(y, bias, K)
        return vr.best_path(idx, v, lg, threshold, jump, switch)
    return run


def one_shape(a, F, dev):
    g = torch.Generator(device='cpu').manual_seed(3)
    x = torch.exp(torch.randn(B, C, F, generator=g) * 2.0).to(dev)
    weight, gain, lag_min, lag_max = lib.f0_tables()
    bias, lg, jump, switch = lib.f0_viterbi_tables()
    L = lag_max - lag_min + 3
    w_d, g_d, b_d, l_d = (torch.from_numpy(t).to(dev) for t in (weight, gain, bias, lg))
    raw = (torch.empty(B, F, device=dev), torch.empty(B, F, device=dev), torch.empty(B, L, F, device=dev))
    f0_kw = dict(weight=w_d, gain=g_d, lag_min=lag_min, lag_max=lag_max, ratio=lib.F0_RATIO, threshold=lib.F0_THRESHOLD)
    lib.frames_f0(x, **f0_kw, want_acf=True, out=raw)
    acf = raw[2]
    out = (torch.empty(B, F, device=dev), torch.empty(B, F, device=dev), torch.empty(B, 4, dtype=torch.int32, device=dev),
           torch.empty(B, device=dev))
    forms = {'frames_f0_acf': lambda: lib.frames_f0(x, **f0_kw, want_acf=True, out=raw)}
    for K in CANDIDATES:
        ws = torch.empty(lib.f0_viterbi_workspace_bytes(B, L, F, K), dtype=torch.uint8, device=dev)
        forms['f0_viterbi_K%d' % K] = (lambda K=K, ws=ws: lib.f0_viterbi(acf, None, 1, lag_min, lag_max, b_d, l_d, K, lib.F0_THRESHOLD, jump,
                                                                         switch, out, ws))
    ts = {k: [] for k in forms}
    for _ in range(a.warmup):
        for fn in forms.values():
            time_calls(fn, a.calls, 0.0)
    for _ in range(a.reps):
        for k, fn in forms.items():
            ts[k].append(time_calls(fn, a.calls, a.hold_ms))
    res = {'F': F, 'lags': L, 'acf_bytes': 4 * B * L * F, 'unit': 'ms per call'}
    for k, v in ts.items():
        res[k] = med_spread(v)
    for K in CANDIDATES:
        key = 'f0_viterbi_K%d' % K
        forms[key]()
        torch.cuda.synchronize()
        counts = out[2].cpu().numpy()
        res[key]['voiced_share'] = float(counts[:, 1].sum() / counts[:, 0].sum())
        res[key]['moved_share'] = float(counts[:, 2].sum() / counts[:, 0].sum())
        try:
            split = kernel_split(forms[key], a.calls)
            res[key]['candidates_ms'], res[key]['path_ms'] = split[KERNELS[0]], split[KERNELS[1]]
            res[key]['path_us_per_frame'] = 1e3 * split[KERNELS[1]] / F
        except Exception as e:   # noqa: BLE001  (no kernel records on this installation: the call's own time stands)
            res[key]['candidates_ms'] = res[key]['path_ms'] = res[key]['path_us_per_frame'] = None
            res[key]['split_error'] = '%s: %s' % (type(e).__name__, e)
        res[key]['call_us_per_frame'] = 1e3 * res[key]['median'] / F
        res[key]['over_frames_f0_acf'] = res[key]['median'] / res['frames_f0_acf']['median']
        host = host_form(acf, bias, lg, K, lib.F0_THRESHOLD, jump, switch)
        want = host()
        hs = []
        for _ in range(a.host_reps):
            t0 = time.perf_counter()
            host()
            hs.append(1e3 * (time.perf_counter() - t0))
        res['host_numpy_K%d' % K] = med_spread(hs)
        res['host_over_kernel_K%d' % K] = res['host_numpy_K%d' % K]['median'] / res[key]['median']
        res[key]['score_equals_host'] = bool(np.array_equal(out[3].cpu().numpy().view(np.uint32), want[1].view(np.uint32)))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--hold-ms', type=float, default=20.0)
    ap.add_argument('--host-reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'f0_viterbi_timing needs a GPU'
    assert a.reps >= 5 and a.calls >= 200, 'at least 5 alternations of at least 200 calls'
    dev = torch.device('cuda', torch.cuda.current_device())
    res = {'tool': 'f0_viterbi_timing', 'B': B, 'C': C, 'reps': a.reps, 'warmup': a.warmup, 'calls': a.calls, 'hold_ms': a.hold_ms,
           'host_reps': a.host_reps, 'version': lib.version(), 'device': torch.cuda.get_device_name(dev),
           'lengths': [one_shape(a, F, dev) for F in FRAMES]}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, 'f0_viterbi_timing.json'), 'w') as f:
            f.write(line + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
