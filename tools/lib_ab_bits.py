"""Does a rewritten kernel still compute the same bits?  The companion of tools/kernel_asm_diff.py for when a kernel's text does
change: two builds of the library run the same entry points over the tests' own case lists, and every output is compared by the
sha256 of its bytes.  Needs a GPU.

  python tools/lib_ab_bits.py <parent .so> <this .so> [--out FILE] [--timeout SECONDS]

For each library one fresh child process is started with TACO_LIB naming it (the library is chosen when tacotron_amd.lib is
imported, so each build gets a process of its own), under its own time limit; the tool stops at the first child that exits nonzero
or runs out of time.  A child prints one line per case and output, `<entry point>/<case>/<output> <sha256>`:
  frames_pitch     over tests.pitch_cases.all_cases()                     out
  frames_sharpen   over tests.sharpen_ref.all_cases()                     out
  frames_cepstats  over the same cases                                     sums, count
  frames_f0        over tests.f0_cases.all_cases(), with the acf           period, strength, acf
(frames_pitch_curve is held bitwise to frames_pitch by tests/test_gpu_frames_curve.py.)  Outputs are fresh buffers; the entry points
define every element of them.  The parent prints `same` or `DIFF` per line, then a tally, and exits 0 only when every line is `same`.
A kernel whose assembly changed must be reachable from an entry point listed here: add it with its test module's case list."""
import argparse
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child():
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    from tacotron_amd import lib
    from tests import f0_cases, pitch_cases, sharpen_ref

    dev = torch.device('cuda', torch.cuda.current_device())
    print('lib_ab_bits: this child runs %s' % lib.LIB_PATH, file=sys.stderr)

    def put(a, dtype=None):
        return None if a is None else torch.as_tensor(np.asarray(a), dtype=dtype).to(dev)

    def emit(name, t):
        print('%s %s' % (name, hashlib.sha256(t.cpu().contiguous().numpy().tobytes()).hexdigest()), flush=True)

    for name, x, frames, steps, per_unit, Q in pitch_cases.all_cases():
        out = lib.frames_pitch(put(x), put(frames, torch.int32), put(steps, torch.int32), per_unit, Q)
        emit('frames_pitch/%s/out' % name, out)
    for name, x, frames, per_unit, beta, Q in sharpen_ref.all_cases():
        x, frames = put(x), put(frames, torch.int32)
        emit('frames_sharpen/%s/out' % name, lib.frames_sharpen(x, beta, Q, frames, per_unit))
        sums, count = lib.frames_cepstats(x, Q, frames, per_unit)
        emit('frames_cepstats/%s/sums' % name, sums)
        emit('frames_cepstats/%s/count' % name, count)
    for c in f0_cases.all_cases():
        got = lib.frames_f0(put(c.x), put(c.frames, torch.int32), c.per_unit, c.weight, c.gain, c.lag_min, c.lag_max, c.ratio,
                            c.threshold, want_acf=True)
        for what, t in zip(('period', 'strength', 'acf'), got):
            emit('frames_f0/%s/%s' % (c.name, what), t)
    return 0


def run_child(so, timeout):
    """[(name, sha256)] of one library, from a fresh process; exits the tool where the child fails"""
    env = dict(os.environ, TACO_LIB=os.path.abspath(so))
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), '--child'], env=env, timeout=timeout, stdout=subprocess.PIPE,
                           text=True)
    except subprocess.TimeoutExpired:
        sys.exit('lib_ab_bits: %s: no result within %d s' % (so, timeout))
    if p.returncode != 0:
        sys.exit('lib_ab_bits: %s: the child exited with status %d' % (so, p.returncode))
    return [tuple(l.split()) for l in p.stdout.splitlines() if l.count(' ') == 1 and '/' in l]


def main():
    ap = argparse.ArgumentParser(usage='python tools/lib_ab_bits.py <parent .so> <this .so> [--out FILE] [--timeout SECONDS]')
    ap.add_argument('libs', nargs='*')
    ap.add_argument('--out', default=None)
    ap.add_argument('--timeout', type=int, default=240, help='per child')
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child()
    if len(a.libs) != 2 or not all(os.path.exists(so) for so in a.libs):
        sys.exit(__doc__)
    parent, here = (dict(run_child(so, a.timeout)) for so in a.libs)
    lines, ndiff = [], 0
    for name in list(parent) + [n for n in here if n not in parent]:
        same = parent.get(name) is not None and parent.get(name) == here.get(name)
        ndiff += not same
        lines.append('%-5s %s %s' % ('same', name, here[name]) if same else
                     'DIFF  %s parent %s here %s' % (name, parent.get(name), here.get(name)))
    lines.append('# %d outputs: %d same, %d DIFF' % (len(lines), len(lines) - ndiff, ndiff))
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text)
    return 0 if lines[:-1] and ndiff == 0 else 1


if __name__ == '__main__':
    sys.exit(main())
