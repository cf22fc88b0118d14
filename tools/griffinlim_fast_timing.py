"""Wall time of fast Griffin-Lim (taco_griffinlim_fast) at the flagship inference shape: F = 360 frames (Td = 180, r = 2), B = 1 and 32.

In the manner of tools/griffinlim_timing.py: every variant is timed with device events around one call; the variants ALTERNATE
inside each repetition and the median over --reps repetitions is reported.  The rotation:
  taco_griffinlim, 50 rounds, of this build -- twice (the difference of the two medians is the run's own spread);
  with --parent-lib PATH the taco_griffinlim of another build of the library (the parent commit's, loaded with plain ctypes), twice;
  taco_griffinlim_fast with momentum 0 / 50 rounds, 0.99 / 50 rounds, 0.99 / 30 rounds, and 0.99 / 30 rounds with the readout.
Recorded next to the medians: what a momentum round costs over a plain one, what the readout costs, fast_30 / plain_50, and (with
--parent-lib) whether taco_griffinlim and taco_griffinlim_rows of this build give the bits of the parent's on one fixed input.

    python tools/griffinlim_fast_timing.py [--reps 20] [--warmup 3] [--parent-lib PATH] [--out DIR]

Prints one JSON line; with --out also writes it to DIR/griffinlim_fast_timing.json.  Exit status 1 when a check fails:
  - same_bits_as_parent is false for either entry point (with --parent-lib);
  - this build's taco_griffinlim, or the momentum-0 fast call, is slower than the parent's taco_griffinlim (mean of its two medians)
    by more than twice the relative difference of the parent's two medians, at least 3 % (with --parent-lib);
  - momentum 0.99 / 30 rounds is not strictly faster than this build's plain 50 rounds at B = 32."""
import argparse
import ctypes as C
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')

import torch  # noqa: E402

from tacotron_amd import lib  # noqa: E402
from tools.griffinlim_timing import alternate  # noqa: E402

F, N_PLAIN, N_FAST, MOMENTUM = 360, 50, 30, 0.99


def parent_library(path):
    """the two older entry points of another build of the library (no tacotron_amd.lib: it lacks the new symbols)"""
    p = C.CDLL(path)
    for name in ('taco_griffinlim_workspace_bytes', 'taco_griffinlim_rows_workspace_bytes'):
        getattr(p, name).restype, getattr(p, name).argtypes = C.c_int64, [C.c_int, C.c_int]
    p.taco_griffinlim.restype, p.taco_griffinlim.argtypes = lib.EXPORTS['taco_griffinlim']
    p.taco_griffinlim_rows.restype, p.taco_griffinlim_rows.argtypes = lib.EXPORTS['taco_griffinlim_rows']
    p.taco_version.restype = C.c_int
    return p


def same_bits_as_parent(parent, dev):
    """taco_griffinlim and taco_griffinlim_rows of both builds on one fixed input (B = 3, F = 41, 3 rounds; rows 41, 24, 3 frames)"""
    B, Fs, n_iter = 3, 41, 3
    g = torch.Generator(device='cpu').manual_seed(41)
    mag = (torch.rand((B, 1025, Fs), generator=g) + 1e-3).to(dev)
    ph = (2.0 * math.pi * torch.rand((B, 1025, Fs), generator=g)).to(dev)
    frames = torch.tensor([41, 24, 3], dtype=torch.int32, device=dev)
    out = {}
    mine = lib.griffinlim(mag, ph, n_iter)
    theirs = torch.full_like(mine, float('nan'))
    work = torch.empty(parent.taco_griffinlim_workspace_bytes(B, Fs) // 4, device=dev)
    rc = parent.taco_griffinlim(lib.ptr(mag), lib.ptr(ph), lib.ptr(theirs), lib.ptr(work), B, Fs, n_iter, lib.stream_ptr())
    assert rc == 0, 'parent taco_griffinlim: rc %d' % rc
    torch.cuda.synchronize()
    out['taco_griffinlim'] = bool(torch.equal(mine.view(torch.int32), theirs.view(torch.int32)))
    for name, p0 in (('taco_griffinlim_rows', ph), ('taco_griffinlim_rows_device_phases', None)):
        mine = lib.griffinlim_rows(mag, frames, phase0=p0, seed=5, n_iter=n_iter)
        theirs = torch.full_like(mine, float('nan'))
        work = torch.empty(parent.taco_griffinlim_rows_workspace_bytes(B, Fs) // 4, device=dev)
        rc = parent.taco_griffinlim_rows(lib.ptr(mag), lib.ptr(p0), 5, lib.ptr(frames), 1, lib.ptr(theirs), lib.ptr(work), B, Fs, n_iter,
                                         lib.stream_ptr())
        assert rc == 0, 'parent taco_griffinlim_rows: rc %d' % rc
        torch.cuda.synchronize()
        out[name] = bool(torch.equal(mine.view(torch.int32), theirs.view(torch.int32)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--parent-lib', default=None, help='libtaco_hip.so of the parent commit')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'griffinlim_fast_timing needs a GPU'
    dev = torch.device('cuda', torch.cuda.current_device())
    parent = parent_library(a.parent_lib) if a.parent_lib else None
    res = {'tool': 'griffinlim_fast_timing', 'F': F, 'n_plain': N_PLAIN, 'n_fast': N_FAST, 'momentum': MOMENTUM, 'reps': a.reps,
           'warmup': a.warmup, 'unit': 'ms per call (median; variants alternate inside each repetition)',
           'parent_lib': bool(parent), 'parent_version': parent.taco_version() if parent else None, 'version': lib.version(),
           'same_bits_as_parent': None, 'rows': [], 'checks': []}
    ok = True
    if parent:
        same = same_bits_as_parent(parent, dev)
        res['same_bits_as_parent'] = all(same.values())
        res['same_bits_detail'] = same
        ok = ok and res['same_bits_as_parent']
    for B in (1, 32):
        g = torch.Generator(device='cpu').manual_seed(B)
        mag = (torch.rand((B, 1025, F), generator=g) + 1e-3).to(dev)
        ph = (2.0 * math.pi * torch.rand((B, 1025, F), generator=g)).to(dev)
        wave = torch.empty(B, 300 * (F - 1), device=dev)
        work = torch.empty(lib.griffinlim_workspace_floats(B, F), device=dev)
        work_fast = torch.empty(lib.griffinlim_fast_workspace_floats(B, F), device=dev)
        conv = torch.empty(B, N_FAST + 1, device=dev)

        def plain():
            lib.griffinlim(mag, ph, N_PLAIN, out=wave, work=work)

        def fast(momentum, n_iter, cv=None):
            return lambda: lib.griffinlim_fast(mag, None, phase0=ph, n_iter=n_iter, momentum=momentum, out=wave, conv=cv, work=work_fast)

        fns = {'taco_griffinlim_a': plain}
        if parent:
            pwork = torch.empty(parent.taco_griffinlim_workspace_bytes(B, F) // 4, device=dev)

            def old():
                rc = parent.taco_griffinlim(lib.ptr(mag), lib.ptr(ph), lib.ptr(wave), lib.ptr(pwork), B, F, N_PLAIN, lib.stream_ptr())
                assert rc == 0, 'parent taco_griffinlim: rc %d' % rc
            fns['parent_taco_griffinlim_a'] = old
        fns['fast_m0_50'] = fast(0.0, N_PLAIN)
        fns['fast_m099_50'] = fast(MOMENTUM, N_PLAIN)
        fns['fast_m099_30'] = fast(MOMENTUM, N_FAST)
        fns['fast_m099_30_conv'] = fast(MOMENTUM, N_FAST, conv)
        fns['taco_griffinlim_b'] = plain
        if parent:
            fns['parent_taco_griffinlim_b'] = old
        row = {'B': B}
        row.update(alternate(fns, a.reps, a.warmup))
        res['rows'].append(row)
        full = 0.5 * (row['taco_griffinlim_a'] + row['taco_griffinlim_b'])
        chk = {'B': B,
               'momentum_round_over_plain_round': row['fast_m099_50'] / row['fast_m0_50'],
               'momentum_round_extra_ms': (row['fast_m099_50'] - row['fast_m0_50']) / N_PLAIN,
               'conv_cost_ms': row['fast_m099_30_conv'] - row['fast_m099_30'],
               'conv_over_without': row['fast_m099_30_conv'] / row['fast_m099_30'],
               'fast_30_over_plain_50': row['fast_m099_30'] / full,
               'fast_30_conv_over_plain_50': row['fast_m099_30_conv'] / full,
               'fast_30_faster_than_plain_50': row['fast_m099_30'] < full}
        if B == 32:
            ok = ok and chk['fast_30_faster_than_plain_50']
        if parent:
            pa, pb = row['parent_taco_griffinlim_a'], row['parent_taco_griffinlim_b']
            base = 0.5 * (pa + pb)
            tol = max(0.03, 2.0 * abs(pa - pb) / min(pa, pb))
            chk.update({'parent_spread': abs(pa - pb) / min(pa, pb), 'tolerance': tol,
                        'taco_griffinlim_over_parent': full / base, 'fast_m0_50_over_parent': row['fast_m0_50'] / base})
            chk['taco_griffinlim_within'] = full <= base * (1.0 + tol)
            chk['fast_m0_50_within'] = row['fast_m0_50'] <= base * (1.0 + tol)
            ok = ok and chk['taco_griffinlim_within'] and chk['fast_m0_50_within']
        res['checks'].append(chk)
    res['ok'] = bool(ok)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, 'griffinlim_fast_timing.json'), 'w') as f:
            f.write(line + '\n')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
