"""Time of the best monotone attention path on the device (taco_alignment_path, as `test --timings` and `evaluate --durations` call
it behind a decode) against
  - taco_alignment_scores on the same tensor: the cost of reading the same bytes once, without a chain of dependent steps;
  - the host path it replaces: the (B, Td, Tt) alignment tensor copied back over PCIe, then the recurrence in NumPy, a step's cells
    taken together (tests/align_path_ref.py best_path_fast, held to the plain-loop restatement by the host tests).

The shape is S1, the flagship training batch: B = 32, Td = 180, Tt = 200 (4.6 MB of alignments), the inputs of
tools/alignment_scores_timing.py, at max_jump 4 (the default) and 1.  The call is a latency chain of Td dependent steps per row, so
the figure to read is the time per decoder step, call / 180.  Both forms of the kernel are timed: the single-wave form takes this
shape; the general form (LDS rows, a barrier per step, the direction table in the workspace) is given the same rows laid out with
Tt = 260 -- the same text lengths, so the same cells -- which is past the single-wave form's 256 characters.  The device calls are
timed with device events, alone and per call of 20 back to back; the host path by the host clock around a synchronised call, and so
is the device call with its results copied back, for a like comparison.  The variants alternate inside each repetition and the
median over --reps is reported.

    python tools/alignment_path_timing.py [--reps 20] [--warmup 3] [--out DIR]

Prints one JSON line; with --out also writes it to DIR/alignment_path_timing.json.  No pass mark: the exit status is 0 unless a call
fails or the paths disagree."""
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
from tests import align_path_ref  # noqa: E402
from tools.alignment_scores_timing import B, BURST, TD, TT, s1_alignments  # noqa: E402
from tools.griffinlim_timing import alternate  # noqa: E402
from tools.wave_join_timing import wall  # noqa: E402

WIDE = 260   # the general form's layout of the same rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'alignment_path_timing needs a GPU'
    dev = torch.device('cuda', torch.cuda.current_device())
    al_h, tl_h = s1_alignments()
    wide_h = np.zeros((B, TD, WIDE), dtype=np.float32)
    wide_h[:, :, :TT] = al_h
    al, wide, tl = torch.tensor(al_h, device=dev), torch.tensor(wide_h, device=dev), torch.tensor(tl_h, device=dev)
    assert lib.alignment_path_workspace_bytes(B, TD, TT) == 0 and lib.alignment_path_workspace_bytes(B, TD, WIDE) == B * TD * WIDE
    out = lib.alignment_path(al, tl)                                   # (path, dur, counts, mass), reused by every call below
    wout = lib.alignment_path(wide, tl)
    work = torch.empty(B * TD * WIDE, dtype=torch.uint8, device=dev)
    counts = torch.empty(B, len(lib.ALIGN_COUNTS), dtype=torch.int32, device=dev)
    means = torch.empty(B, len(lib.ALIGN_MEANS), device=dev)
    host = {}

    def wave(J):
        return lambda: lib.alignment_path(al, tl, None, J, *out)

    def general(J):
        return lambda: lib.alignment_path(wide, tl, None, J, *wout, work)

    def scores():
        lib.alignment_scores(al, tl, None, lib.MAX_JUMP, counts, means)

    def burst(call):
        def run():
            for _ in range(BURST):
                call()
        return run

    def device_path():   # what the drivers do: the call, then dur, counts and mass to the host
        wave(lib.PATH_JUMP)()
        host['device'] = tuple(x.cpu().numpy() for x in out[1:])

    def host_copy():
        host['al'] = al.cpu().numpy()

    def host_path():   # what it replaces: the alignment tensor to the host, then the recurrence in NumPy
        host_copy()
        host['host'] = align_path_ref.best_paths(host['al'], tl_h, None, lib.PATH_JUMP, one=align_path_ref.best_path_fast)

    res = {'tool': 'alignment_path_timing', 'B': B, 'Td': TD, 'Tt': TT, 'general_form_Tt': WIDE, 'reps': a.reps, 'warmup': a.warmup,
           'version': lib.version(), 'unit': 'ms per call (median; variants alternate inside each repetition)'}
    calls = {'taco_alignment_scores': scores}
    for J in (lib.PATH_JUMP, 1):
        calls['wave_form_J%d' % J], calls['general_form_J%d' % J] = wave(J), general(J)
    variants = dict(calls)
    variants.update({k + '_x%d' % BURST: burst(f) for k, f in calls.items()})
    ev = alternate(variants, a.reps, a.warmup)
    for k in calls:
        ev[k + '_steady'] = ev.pop(k + '_x%d' % BURST) / BURST
    res['events'] = ev
    res['wall'] = wall({'device_call': wave(lib.PATH_JUMP), 'device_call_and_copy_back': device_path,
                        'host_copy_of_the_alignments': host_copy, 'host_copy_and_numpy_recurrence': host_path}, a.reps, a.warmup)
    general(lib.PATH_JUMP)()
    wave(lib.PATH_JUMP)()
    torch.cuda.synchronize()
    got, gen, want = tuple(x.cpu().numpy() for x in out), tuple(x.cpu().numpy() for x in wout), host['host']
    same = all(np.array_equal(g, w) for g, w in zip(got[:3], want[:3])) and got[3].tobytes() == want[3].tobytes()
    forms = (np.array_equal(gen[0], got[0]) and np.array_equal(gen[1][:, :TT], got[1]) and np.array_equal(gen[2], got[2])
             and gen[3].tobytes() == got[3].tobytes())
    res['device_equals_host'], res['forms_agree'] = bool(same), bool(forms)
    nbytes = 4.0 * B * TD * TT
    J = lib.PATH_JUMP
    res['checks'] = {'bytes_read': nbytes,
                     'us_per_decoder_step': {k: 1e3 * ev[k + '_steady'] / TD for k in calls if k != 'taco_alignment_scores'},
                     'wave_form_over_scores_call': ev['wave_form_J%d_steady' % J] / ev['taco_alignment_scores_steady'],
                     'general_form_over_wave_form': ev['general_form_J%d_steady' % J] / ev['wave_form_J%d_steady' % J],
                     'host_path_over_device_path': res['wall']['host_copy_and_numpy_recurrence'] / res['wall']['device_call_and_copy_back'],
                     'bytes_back_host_path': nbytes, 'bytes_back_device_path': 4.0 * B * (TT + 3 + 1)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, 'alignment_path_timing.json'), 'w') as f:
            f.write(line + '\n')
    return 0 if same and forms else 1


if __name__ == '__main__':
    sys.exit(main())
