"""The runtime switches of libtaco_hip.so, held together on the host (no GPU call): the declared table
(tacotron_amd/csrc/switches.def), its one reader (switches.h, compiled here with the host C++ compiler and run against a
Python restatement of the five parse rules), every name the tests, tools and drivers use, and INTEGRATION.md §4."""
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'tacotron_amd', 'csrc')

# (name, kind, default, read): derived from the sources before the table existed; a change of the table is a change of this literal
TABLE = (
    [(n, 'PRESENT', 0, 'LIVE') for n in (
        'DEC_NO_LRES', 'DEC_FAKEW', 'DEC_FAKEX', 'DEC_NOPF', 'DEC_NOLIVE', 'DEC_V3_AGENT', 'GEMM2_TRACE', 'SPK_UNFUSED', 'QUIET',
        'BWD_PREP_EARLY', 'NO_PRENET_FUSE', 'PN_TRACE', 'DEC_TRACE', 'NO_BANK_GATHER', 'NO_SIDE_TN')] +
    [(n, 'NONZERO', 0, 'LIVE') for n in ('DETERMINISTIC', 'TN2', 'NO_POOL_FUSE', 'NO_OVERLAP')] +
    [(n, 'UNLESS0', 1, 'LIVE') for n in (
        'GEMM2_BF16X', 'TN_MERGE_TAPS', 'GEMM2_XCD', 'GEMM2_BANK_XCD', 'GEMM2_BSPLIT', 'XPROJ_BWD_KSPLIT')] +
    [('BF16X_MAX_CHAIN', 'INT', 2048, 'LIVE'), ('GEMM2_MIN_TILES', 'INT', 160, 'LIVE'), ('TN_XCD', 'INT', 1, 'LIVE'),
     ('TAIL_EVENTS', 'INT', 1, 'LIVE'), ('DEC_V3', 'INT', -1, 'LIVE'), ('KSPLIT', 'INT', 0, 'LIVE'), ('DEC_CLUSTER', 'INT', 0, 'LIVE'),
     ('TN_BLOCKS', 'INT', 0, 'ONCE'), ('TN_BM', 'INT', 0, 'ONCE'), ('TN_BIG_TILES', 'INT', 128, 'ONCE'), ('GEMM2_BI_NS', 'INT', 3, 'ONCE'),
     ('GEMM2_VARIANT', 'TEXT', 0, 'LIVE'), ('DEC_ALLOW_XCD_LOCAL', 'TEXT', 0, 'LIVE')])
PYTHON_SIDE = {'TACO_LIB', 'TACO_FORCE_DIST', 'TACO_COMM_PRIORITY', 'TACO_CORPUS_HBM_GB'}   # read by tacotron_amd/*.py, not by the library
NAME = re.compile(r'TACO_[A-Z0-9_]+')


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def declared():
    """switches.def -> [(name, kind, default, read, effect)], one per line that is neither blank nor a comment."""
    rows = []
    for line in read('tacotron_amd', 'csrc', 'switches.def').splitlines():
        if not line.strip() or line.lstrip().startswith('//'):
            continue
        m = re.fullmatch(r'\w+\((\w+),\s*(\w+),\s*(-?\d+),\s*(\w+),\s*"([^"]+)"\)', line.strip())
        assert m, 'switches.def: not a table line: %r' % line
        rows.append((m.group(1), m.group(2), int(m.group(3)), m.group(4), m.group(5)))
    return rows


def csrc_files():
    return sorted(glob.glob(os.path.join(CSRC, '*')))


# the compile-time names: each is selected by build.sh (the probe and previous-decoder libraries) or by a tool
COMPILE_TIME = {'TACO_DEC_PROBES', 'TACO_NO_RS', 'TACO_NO_POLL128', 'TACO_NO_SHADOW', 'TACO_NO_GROUPED_FANDQ', 'TACO_NO_UNIPOLL',
                'TACO_NO_TANH_SPLIT', 'TACO_PN_TRACE', 'TACO_GRU_TRACE'}


def compile_time_names():
    """Every identifier that csrc/ tests in a preprocessor condition, whatever its prefix."""
    names = set()
    for path in csrc_files():
        if path.endswith(('.hip', '.h')):
            for line in open(path):
                m = re.match(r'\s*#\s*(if|ifdef|ifndef|elif)\b(.*)', line)
                if m:
                    names.update(re.findall(r'\b[A-Za-z_]\w*', m.group(2).split('//')[0]))
    return names - {'defined'}


def test_table_is_the_pinned_one():
    rows = declared()
    names = [r[0] for r in rows]
    assert len(names) == len(set(names)) == 38
    # PRESENT / NONZERO / UNLESS0 / TEXT defaults are informative: what an unset variable means (off, off, on, null)
    assert sorted(r[:4] for r in rows) == sorted(TABLE)


def test_switches_h_is_the_only_reader_and_every_switch_is_used():
    others = ''
    for path in csrc_files():
        if os.path.basename(path) != 'switches.h' and os.path.isfile(path):
            text = open(path).read()
            assert 'getenv' not in text, '%s reads the environment by itself' % os.path.basename(path)
            if os.path.basename(path) != 'switches.def':
                others += text
    assert 'getenv' in read('tacotron_amd', 'csrc', 'switches.h')
    used = set(re.findall(r'\bSW_([A-Z0-9_]+)\b', others))
    assert not [n for n, _, _, _ in TABLE if n not in used]
    assert used <= {n for n, _, _, _ in TABLE}


HARNESS = r'''
#include <cstdio>
#include <utility>
#include "switches.h"
template <Switch S> void show() {
  if constexpr (kSwitches[S].kind == SWK_INT) printf("%s %d\n", kSwitches[S].env, sw_int<S>());
  else if constexpr (kSwitches[S].kind == SWK_TEXT) printf("%s %s\n", kSwitches[S].env, sw_text<S>() ? sw_text<S>() : "(null)");
  else printf("%s %d\n", kSwitches[S].env, (int)sw_on<S>());
}
template <int... I> void all(std::integer_sequence<int, I...>) { (show<(Switch)I>(), ...); }
int main() { all(std::make_integer_sequence<int, SW_COUNT>()); }
'''


def atoi(s):
    m = re.match(r'\s*([+-]?\d+)', s)
    return int(m.group(1)) if m else 0


def expected(kind, default, e):
    """The five rules, e = the variable's value or None."""
    if kind == 'PRESENT':
        return '%d' % (e is not None)
    if kind == 'NONZERO':
        return '%d' % (e is not None and atoi(e) != 0)
    if kind == 'UNLESS0':
        return '%d' % (not (e is not None and atoi(e) == 0))
    if kind == 'INT':
        return '%d' % (atoi(e) if e is not None else default)
    assert kind == 'TEXT'
    return '(null)' if e is None else e


def host_compile(src, out):
    """switches.h includes nothing from HIP: a plain host compile; hipcc (host-only, as C++) where there is no host compiler."""
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    cmd = [cxx] if cxx else [shutil.which('hipcc') or '/opt/rocm/bin/hipcc', '-x', 'c++']
    return subprocess.run(cmd + ['-std=c++17', '-I', CSRC, '-o', out, src], stderr=subprocess.PIPE, universal_newlines=True)


@pytest.fixture(scope='module')
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp('switches')
    src, exe = str(d / 'harness.cpp'), str(d / 'harness')
    with open(src, 'w') as f:
        f.write(HARNESS)
    done = host_compile(src, exe)
    assert done.returncode == 0, done.stderr

    def run(env):
        base = {k: v for k, v in os.environ.items() if not k.startswith('TACO_')}
        out = subprocess.check_output([exe], env=dict(base, **env)).decode()
        return [tuple(line.split(' ', 1)) for line in out.split('\n')[:-1]]
    return run


@pytest.mark.parametrize('value', [None, '', '0', '1', '2', 'x', '-1'])
def test_parse_rules(harness, value):
    """Every switch set to the same value, one fresh process per value (so the ONCE entries are read for the first time)."""
    env = {} if value is None else {'TACO_' + n: value for n, _, _, _ in TABLE}
    got = dict(harness(env))
    want = {'TACO_' + n: expected(kind, default, value) for n, kind, default, _ in TABLE}
    assert got == want


def test_each_switch_reads_its_own_name(harness):
    """One variable set at a time, to a value its kind tells from unset ("0": PRESENT on, UNLESS0 off, TEXT "0"; NONZERO "1"; INT "7"):
    that switch alone leaves its unset value."""
    unset = {'TACO_' + n: expected(kind, default, None) for n, kind, default, _ in TABLE}
    for n, kind, default, _ in TABLE:
        v = {'NONZERO': '1', 'INT': '7'}.get(kind, '0')
        want = dict(unset)
        want['TACO_' + n] = expected(kind, default, v)
        assert want != unset
        assert dict(harness({'TACO_' + n: v})) == want, n


@pytest.mark.parametrize('call', ['sw_int<SW_QUIET>()', 'sw_on<SW_KSPLIT>()', 'sw_text<SW_TN2>()', 'sw_on<SW_GEMM2_VARIANT>()'])
def test_asking_for_the_wrong_type_does_not_compile(tmp_path, call):
    src = str(tmp_path / 'wrong.cpp')
    with open(src, 'w') as f:
        f.write('#include "switches.h"\nint main() { return (int)(long)%s; }\n' % call)
    done = host_compile(src, str(tmp_path / 'wrong'))
    assert done.returncode != 0 and 'the table' in done.stderr, done.stderr


def test_names_in_tests_tools_and_drivers_exist():
    files = (glob.glob(os.path.join(ROOT, 'tests', '*.py')) + glob.glob(os.path.join(ROOT, 'tools', '*.py')) +
             glob.glob(os.path.join(ROOT, 'tools', '*.sh')) + glob.glob(os.path.join(ROOT, 'tacotron_amd', '*.py')) +
             [os.path.join(ROOT, 'bench.py'), os.path.join(CSRC, 'build.sh')])
    known = ({'TACO_' + n for n, _, _, _ in TABLE} | compile_time_names() | PYTHON_SIDE |
             set(re.findall(r'^\s*#\s*define\s+(TACO_[A-Z0-9_]+)', read('include', 'taco_hip.h'), re.M)))
    unknown = {}
    for path in files:
        for name in set(NAME.findall(open(path).read())) - known:
            unknown.setdefault(name, []).append(os.path.relpath(path, ROOT))
    assert not unknown, 'names that nothing reads, tests or defines: %r' % unknown


def test_every_compile_time_name_is_selected_by_a_build_or_a_tool():
    """A fork that no build script, benchmark or tool compiles is code that nothing exercises: it goes, with its -D."""
    selectors = ''.join(open(path).read() for path in (
        [os.path.join(CSRC, 'build.sh'), os.path.join(ROOT, 'bench.py')] + glob.glob(os.path.join(ROOT, 'tools', '*.py')) +
        glob.glob(os.path.join(ROOT, 'tools', '*.sh')) + glob.glob(os.path.join(ROOT, 'tools', 'micro', '*.hip'))))
    names = compile_time_names()
    unselected = sorted(n for n in names if not re.search(r'(-D|#\s*define\s+)%s\b' % re.escape(n), selectors))
    assert not unselected, 'tested under csrc/, selected nowhere: %r' % unselected
    assert names == COMPILE_TIME


def test_units_is_the_one_list_of_translation_units():
    """csrc/UNITS names every .hip file but the decoder pair (which the build scripts take in several builds) exactly once, names
    nothing else, and neither build script keeps a list of its own beside it."""
    units = open(os.path.join(CSRC, 'UNITS')).read().split()
    on_disk = sorted(os.path.basename(p)[:-len('.hip')] for p in glob.glob(os.path.join(CSRC, '*.hip')))
    assert sorted(units) == [u for u in on_disk if u not in ('decoder', 'decoder3')]   # (sorted lists: a name twice would not match)
    for u in units:
        assert os.path.isfile(os.path.join(CSRC, u + '.hip')), u
    for script in (os.path.join(CSRC, 'build.sh'), os.path.join(ROOT, 'tools', 'ab_build.sh')):
        text = open(script).read()
        assert 'UNITS' in text, script
        for u in ('gemm2', 'vocoder', 'monitor'):
            assert not re.search(r'\b%s\b' % u, text), '%s names %s itself' % (os.path.relpath(script, ROOT), u)


def test_integration_md_documents_exactly_the_switches():
    section = read('INTEGRATION.md').split('\n## 4. ')[1].split('\n## ')[0]
    runtime, flags = set(), set()
    for line in section.splitlines():
        m = re.match(r'\| (.*?) \| ', line)
        if m:
            flags.update(re.findall(r'-D(TACO_[A-Z0-9_]+)', m.group(1)))
            runtime.update(NAME.findall(re.sub(r'-DTACO_[A-Z0-9_]+', '', m.group(1))))
    assert runtime - PYTHON_SIDE == {'TACO_' + n for n, _, _, _ in TABLE}
    assert PYTHON_SIDE <= runtime
    assert flags == compile_time_names()
