"""Is a move a move?  Compares the device assembly of every kernel of two source trees, text against text.  CPU only.

  python tools/kernel_asm_diff.py <parent tree> <this tree>      (each the root of a checkout; prints to stdout)

For each tree and each unit of that tree's list (csrc/UNITS, or build.sh's COMMON where the tree has no such file, plus decoder and
decoder3) the device assembly is emitted with the flags of that tree's build.sh plus `-S --cuda-device-only` (D3FLAGS for
decoder3.hip).  A kernel's text runs from the `.text` / `.section .text.<symbol>` directive in front of its label to its
`.end_amdhsa_kernel`, i.e. the code and the kernel descriptor (registers, LDS, scratch).  Comments and blank lines are dropped, and
the local labels lose what depends on the kernel's position in its file: the function index of `.LBB<n>_<m>`, `.Lfunc_begin<n>`,
`.Lfunc_end<n>`, and the number of `.Ltmp<n>`, which is renumbered by first appearance inside the kernel.  Kernels are matched by
mangled name, whatever unit they are in; a name that two units of one tree define (internal linkage) carries its unit's name.
One line per kernel: `same`, `DIFF`, `only in parent` or `only here`; the exit status is 0 only when every kernel is `same`.
The tool looks at nothing but equality of text and knows no instruction."""
import concurrent.futures
import os
import re
import shlex
import subprocess
import sys
import tempfile


def tree_units(tree):
    """(csrc directory, [(unit, flags)]) of a tree, from its own build.sh and list of units."""
    csrc = os.path.join(tree, 'tacotron_amd', 'csrc')
    sh = open(os.path.join(csrc, 'build.sh')).read()
    var = lambda name: re.search(r'^%s="([^"]*)"' % name, sh, re.M)
    flags, d3 = shlex.split(var('FLAGS').group(1)), shlex.split(var('D3FLAGS').group(1))
    if os.path.exists(os.path.join(csrc, 'UNITS')):
        units = open(os.path.join(csrc, 'UNITS')).read().split()
    else:
        units = var('COMMON').group(1).split()
    return csrc, [(u, flags) for u in units + ['decoder']] + [('decoder3', flags + d3)]


def emit(csrc, unit, flags, out):
    subprocess.run(['hipcc'] + flags + ['-S', '--cuda-device-only', unit + '.hip', '-o', out], cwd=csrc, check=True,
                   stderr=subprocess.DEVNULL)
    return open(out).read().split('\n')


def kernels_of(lines):
    """{mangled name: normalised text} of one assembly file."""
    out = {}
    text_at, begin_of, name = 0, {}, None
    for end, l in enumerate(lines):
        s = l.strip()
        if s == '.text' or re.match(r'\.section\s+\.text', s):
            text_at = end
        elif re.match(r'[A-Za-z_$][\w$.]*:', l):
            begin_of[l.split(':')[0]] = text_at   # a global label: its text begins at the section directive in front of it
        elif s.startswith('.amdhsa_kernel '):
            name = s.split()[1]
        if s != '.end_amdhsa_kernel':
            continue
        begin = begin_of[name]
        tmp = {}
        body = []
        for t in lines[begin:end + 1]:
            t = t.split(';')[0].rstrip()
            if not t.strip():
                continue
            t = re.sub(r'\.LBB\d+_', '.LBB_', t)
            t = re.sub(r'\.Lfunc_(begin|end)\d+', r'.Lfunc_\1', t)
            t = re.sub(r'\.Ltmp(\d+)', lambda m: '.Ltmp#%d' % tmp.setdefault(m.group(1), len(tmp)), t)
            body.append(t)
        out[name] = '\n'.join(body)
    return out


def tree_kernels(tree, tmpdir, tag, pool):
    csrc, units = tree_units(tree)
    jobs = [(u, pool.submit(emit, csrc, u, f, os.path.join(tmpdir, '%s_%s.s' % (tag, u)))) for u, f in units]
    per_unit = [(u, kernels_of(j.result())) for u, j in jobs]
    count = {}
    for _, ks in per_unit:
        for name in ks:
            count[name] = count.get(name, 0) + 1
    return {(name if count[name] == 1 else '%s [%s]' % (name, u)): text for u, ks in per_unit for name, text in ks.items()}


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as tmpdir, concurrent.futures.ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as pool:
        parent = tree_kernels(sys.argv[1], tmpdir, 'parent', pool)
        here = tree_kernels(sys.argv[2], tmpdir, 'here', pool)
    tally = {}
    for name in sorted(set(parent) | set(here)):
        if name not in here:
            verdict = 'only in parent'
        elif name not in parent:
            verdict = 'only here'
        else:
            verdict = 'same' if parent[name] == here[name] else 'DIFF'
        tally[verdict] = tally.get(verdict, 0) + 1
        print('%-14s %s' % (verdict, name))
    print('# %d kernels: %s' % (sum(tally.values()), ', '.join('%d %s' % (n, v) for v, n in sorted(tally.items()))))
    sys.exit(0 if set(tally) <= {'same'} else 1)


if __name__ == '__main__':
    main()
