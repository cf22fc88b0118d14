"""Wall time of one Griffin-Lim call at the flagship inference shape: F = 360 frames (Td = 180, r = 2), 50 rounds, B = 1 and 32.

taco_griffinlim against taco_griffinlim_rows with every row at 360, 184 and 96 frames (the lengths of
profiles/infer_stop_timing.json times r) and with a mixed batch (lengths spread evenly over 96 .. 360).  Every variant is timed
with device events around one call; the variants ALTERNATE inside each repetition and the median over --reps repetitions is
reported.  taco_griffinlim is in the rotation twice: the difference of its two medians is the run's own spread.
--parent-lib PATH adds the taco_griffinlim of another build of the library (the parent commit's), loaded with plain ctypes, twice
in the same rotation; the checks then compare against it.  Separately: today's host phase draw + upload (host clock around
torch.rand on the CPU, the copy and a synchronise) against a taco_griffinlim_rows call with n_iter = 0 that is given phases and
one that draws them on the device (phase0 = NULL).

    python tools/griffinlim_timing.py [--reps 20] [--warmup 3] [--parent-lib PATH] [--out DIR]

Prints one JSON line; with --out also writes it to DIR/griffinlim_rows_timing.json.  Exit status 1 when a check fails:
  - rows at full length, and this build's taco_griffinlim, are not slower than the parent's taco_griffinlim (mean of its two
    medians) by more than twice the relative difference of the parent's two medians, at least 3 % (with --parent-lib);
  - rows at 96 of 360 frames are strictly faster than this build's full-length taco_griffinlim."""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tacotron_amd import lib  # noqa: E402

F, N_ITER, LENGTHS = 360, 50, (360, 184, 96)


def alternate(fns, reps, warmup):
    """{name: median ms}: each repetition runs every callable once, in order, each between its own pair of device events"""
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
    return {k: float(np.median(v)) for k, v in ts.items()}


def parent_griffinlim(path):
    """taco_griffinlim and its workspace size from another build of the library (no tacotron_amd.lib: it lacks the new symbols)"""
    p = C.CDLL(path)
    p.taco_griffinlim_workspace_bytes.restype = C.c_int64
    p.taco_griffinlim_workspace_bytes.argtypes = [C.c_int, C.c_int]
    p.taco_griffinlim.restype = C.c_int
    p.taco_griffinlim.argtypes = [C.c_void_p] * 4 + [C.c_int] * 3 + [C.c_void_p]
    p.taco_version.restype = C.c_int
    return p


def host_phase_draw_ms(B, reps, warmup, dev):
    """what griffinlim.invert_spectrogram does without `lengths`: torch.rand on the CPU, scaled, copied to the device"""
    ts = []
    for i in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g = torch.Generator(device='cpu').manual_seed(i)
        ph = (2.0 * math.pi * torch.rand((B, 1025, F), generator=g)).to(dev)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
        del ph
    return float(np.median(ts[warmup:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--parent-lib', default=None, help='libtaco_hip.so of the parent commit')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'griffinlim_timing needs a GPU'
    dev = torch.device('cuda', torch.cuda.current_device())
    parent = parent_griffinlim(a.parent_lib) if a.parent_lib else None
    res = {'tool': 'griffinlim_timing', 'F': F, 'n_iter': N_ITER, 'reps': a.reps, 'warmup': a.warmup,
           'unit': 'ms per call (median; variants alternate inside each repetition)',
           'parent_lib': bool(parent), 'parent_version': parent.taco_version() if parent else None, 'version': lib.version(),
           'rows': [], 'phases': [], 'checks': []}
    ok = True
    for B in (1, 32):
        g = torch.Generator(device='cpu').manual_seed(B)
        mag = (torch.rand((B, 1025, F), generator=g) + 1e-3).to(dev)
        ph = (2.0 * math.pi * torch.rand((B, 1025, F), generator=g)).to(dev)
        wave = torch.empty(B, 300 * (F - 1), device=dev)
        work = torch.empty(lib.griffinlim_workspace_floats(B, F), device=dev)
        work_rows = torch.empty(lib.griffinlim_rows_workspace_floats(B, F), device=dev)
        frames = {n: torch.full((B,), n, dtype=torch.int32, device=dev) for n in LENGTHS}
        mixed = torch.tensor(np.round(np.linspace(LENGTHS[-1], LENGTHS[0], B)).astype(np.int32), device=dev) if B > 1 else None

        def plain():
            lib.griffinlim(mag, ph, N_ITER, out=wave, work=work)

        def rows(fr, n_iter=N_ITER, phase0=ph):
            return lambda: lib.griffinlim_rows(mag, fr, phase0=phase0, seed=1, n_iter=n_iter, out=wave, work=work_rows)

        fns = {'taco_griffinlim_a': plain}
        if parent:
            pwork = torch.empty(parent.taco_griffinlim_workspace_bytes(B, F) // 4, device=dev)

            def old():
                rc = parent.taco_griffinlim(lib.ptr(mag), lib.ptr(ph), lib.ptr(wave), lib.ptr(pwork), B, F, N_ITER, lib.stream_ptr())
                assert rc == 0, 'parent taco_griffinlim: rc %d' % rc
            fns['parent_taco_griffinlim_a'] = old
        for n in LENGTHS:
            fns['rows_%d' % n] = rows(frames[n])
        if mixed is not None:
            fns['rows_mixed'] = rows(mixed)
        fns['taco_griffinlim_b'] = plain
        if parent:
            fns['parent_taco_griffinlim_b'] = old
        row = {'B': B}
        row.update(alternate(fns, a.reps, a.warmup))
        if mixed is not None:
            row['mixed_frames_mean'] = float(mixed.float().mean())
        res['rows'].append(row)
        full = 0.5 * (row['taco_griffinlim_a'] + row['taco_griffinlim_b'])
        chk = {'B': B, 'rows_96_over_full': row['rows_96'] / full, 'rows_184_over_full': row['rows_184'] / full,
               'rows_96_faster_than_full': row['rows_96'] < full}
        ok = ok and chk['rows_96_faster_than_full']
        if parent:
            pa, pb = row['parent_taco_griffinlim_a'], row['parent_taco_griffinlim_b']
            base = 0.5 * (pa + pb)
            tol = max(0.03, 2.0 * abs(pa - pb) / min(pa, pb))
            chk.update({'parent_spread': abs(pa - pb) / min(pa, pb), 'tolerance': tol,
                        'rows_360_over_parent': row['rows_360'] / base, 'taco_griffinlim_over_parent': full / base})
            chk['rows_360_within'] = row['rows_360'] <= base * (1.0 + tol)
            chk['taco_griffinlim_within'] = full <= base * (1.0 + tol)
            ok = ok and chk['rows_360_within'] and chk['taco_griffinlim_within']
        res['checks'].append(chk)
        # initial phases: host draw + upload against the device's own, around a call that does nothing else but one istft
        p = alternate({'rows_n_iter0_phase0_given': rows(frames[F], 0), 'rows_n_iter0_phase0_null': rows(frames[F], 0, None)},
                      a.reps, a.warmup)
        p.update({'B': B, 'host_draw_and_upload': host_phase_draw_ms(B, max(3, a.reps // 4), 1, dev),
                  'phase_bytes': B * 1025 * F * 4})
        res['phases'].append(p)
    res['ok'] = bool(ok)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, 'griffinlim_rows_timing.json'), 'w') as f:
            f.write(line + '\n')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
