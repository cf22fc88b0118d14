"""taco_tensor_stats on the GPU (include/taco_hip.h) against the NumPy restatement (tests/monitor_ref.py).  Every call goes through
lib.tensor_stats with the buffer, the three outputs and the workspace carved from one guarded arena (tests/poison.py): outputs and
workspace start as poison, every output element must be written and the guard bands must come back as they were.

Shapes: with C = TACO_STATS_CHUNK (a wave's work item) the sizes 0, 1, 3, 4, 5, 63, 64, 65, C - 1, C, C + 1, 2 C + 7, each at float
offsets 0, 1, 2 and 3 mod 4 (an offset moves the chunk cut: positions count from the 16-byte boundary below the segment), two
overlapping segments, and a list of 300 that puts a size-1 segment between two of 3 C.  Values: normal draws scaled over 2^-30 ..
2^20, exact powers of two and their predecessors, +-0, subnormals, +-Inf and NaN of both signs, the specials also at a segment's
first and last element.

Bars: counts and hist exactly; min, max and absmax bit for bit; |sum - fsum| <= size 2^-53 sum|x| and the same for the squares -- the
bound of fp64 summation in any order (monitor_ref.sum_bounds), not a tuned figure."""
import numpy as np
import pytest
import torch

from tests import monitor_ref as mr
from tests.poison import Guarded

pytestmark = pytest.mark.gpu

SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 1e-45, -1e-45, 1.1754942e-38, 1.0, 0.99999994, -2.0, -1.9999999,
                     2.0 ** -24, 2.0 ** -24 * 0.99999994, 65536.0, 65535.996, 3.4028235e38], dtype=np.float32)
SPECIALS[5] = np.array([0xffc00000], dtype=np.uint32).view(np.float32)[0]     # a NaN with the sign bit set


def bits64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def values(n, seed):
    """n fp32 values: scaled normal draws with the specials sprinkled in, and one of them at each end"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * np.exp2(rng.uniform(-30, 20, n))).astype(np.float32)
    if n:
        k = max(1, n // 16)
        x[rng.integers(0, n, k)] = SPECIALS[rng.integers(0, len(SPECIALS), k)]
        e = np.exp2(rng.integers(-30, 21, k)).astype(np.float32)
        x[rng.integers(0, n, k)] = np.where(rng.integers(0, 2, k) > 0, e, mr.prev_toward_zero(e)) * rng.choice(np.float32([-1, 1]), k)
        x[0] = SPECIALS[seed % len(SPECIALS)]
        x[-1] = SPECIALS[(seed // 3 + 7) % len(SPECIALS)]
    return x


def layout(sizes_offsets, gap=9):
    """disjoint segments (size, offset mod 4) laid out in order with NaN gaps -> (base, [(offset, size)])"""
    segs, at = [], 4
    for i, (n, a) in enumerate(sizes_offsets):
        at += (a - at) % 4
        segs.append((at, n))
        at += n + gap
    base = np.full(at + 8, np.nan, dtype=np.float32)
    for i, (o, n) in enumerate(segs):
        base[o:o + n] = values(n, 100 + i)
    return base, segs


def run(lib, base, segs, e_lo=-24, e_hi=15, s=2, work_fill='qnan', plan=None):
    """one guarded call -> (counts, moments, hist) as host arrays"""
    nb = mr.n_bins(e_lo, e_hi, s)
    plan = plan or lib.tensor_stats_plan(segs, len(base))
    need = lib.tensor_stats_workspace_bytes(plan.n, plan.n_items, nb)
    G = Guarded({'base': ((len(base),), torch.float32, 'zeros'), 'counts': ((plan.n, 6), torch.int64, 'ones'),
                 'moments': ((plan.n, 5), torch.float64, 'ones'), 'hist': ((plan.n, nb), torch.int64, 'ones'),
                 'work': ((need,), torch.uint8, work_fill)})
    G['base'].copy_(torch.from_numpy(base))
    res = lib.tensor_stats(G['base'], plan, e_lo, e_hi, s, G['counts'], G['moments'], G['hist'], G['work'])
    torch.cuda.synchronize()
    assert res.counts is G['counts'] and res.moments is G['moments'] and res.hist is G['hist']
    G.check('counts', 'moments', 'hist')
    assert np.array_equal(G['base'].cpu().numpy().view(np.uint32), base.view(np.uint32)), 'base was written'
    return tuple(t.cpu().numpy() for t in res)


def compare(got, base, segs, e_lo=-24, e_hi=15, s=2, label=''):
    counts, moments, hist = got
    rc, rm, rh = mr.stats_many(base, segs, e_lo, e_hi, s)
    assert counts.dtype == np.int64 and moments.dtype == np.float64 and hist.dtype == np.int64
    assert np.array_equal(counts, rc), '%s counts differ at segments %s' % (label, np.flatnonzero((counts != rc).any(1))[:8])
    assert np.array_equal(hist, rh), '%s hist differs at segments %s' % (label, np.flatnonzero((hist != rh).any(1))[:8])
    assert (hist.sum(1) == counts[:, 1]).all()
    assert np.array_equal(bits64(moments[:, 2:]), bits64(rm[:, 2:])), '%s min / max / absmax differ at segments %s' % (
        label, np.flatnonzero((bits64(moments[:, 2:]) != bits64(rm[:, 2:])).any(1))[:8])
    worst = [0.0, 0.0]
    for i, (o, n) in enumerate(segs):
        b = mr.sum_bounds(base[o:o + n])
        for j in (0, 1):
            err = abs(moments[i, j] - rm[i, j])
            assert err <= b[j], '%s segment %d %s: |got - fsum| = %.3e, bound %.3e' % (label, i, mr.MOMENTS[j], err, b[j])
            if b[j] > 0:
                worst[j] = max(worst[j], err / b[j])
    print('  %-28s %4d segments: worst |sum - fsum| / bound %.2e, sumsq %.2e' % (label, len(segs), worst[0], worst[1]))
    return got


@pytest.fixture(scope='module')
def main_case(built_lib):
    Cc = built_lib.STATS_CHUNK
    sizes = [0, 1, 3, 4, 5, 63, 64, 65, Cc - 1, Cc, Cc + 1, 2 * Cc + 7]
    base, segs = layout([(n, a) for n in sizes for a in range(4)])
    # two overlapping segments inside the last (largest) one, at odd offsets
    o = segs[-1][0]
    segs = segs + [(o + 1, Cc + 100), (o + 51, Cc)]
    return base, segs


def test_sizes_and_offsets_against_the_restatement(built_lib, main_case):
    base, segs = main_case
    assert {o % 4 for o, _ in segs} == {0, 1, 2, 3}
    compare(run(built_lib, base, segs), base, segs, label='sizes x offsets')


def test_two_runs_give_the_same_bits_whatever_the_workspace_held(built_lib, main_case):
    base, segs = main_case
    a = run(built_lib, base, segs, work_fill='qnan')
    b = run(built_lib, base, segs, work_fill='noise')
    c = run(built_lib, base, segs, work_fill='ones')
    for x, y in ((a, b), (a, c)):
        assert np.array_equal(x[0], y[0]) and np.array_equal(bits64(x[1]), bits64(y[1])) and np.array_equal(x[2], y[2])


def test_each_row_equals_the_call_with_that_segment_alone(built_lib, main_case):
    base, segs = main_case
    counts, moments, hist = run(built_lib, base, segs)
    for i, seg in enumerate(segs):
        c1, m1, h1 = run(built_lib, base, [seg])
        assert np.array_equal(c1[0], counts[i]) and np.array_equal(h1[0], hist[i]), (i, seg)
        assert np.array_equal(bits64(m1[0]), bits64(moments[i])), (i, seg, m1[0], moments[i])


def test_floats_outside_the_segments_have_no_influence(built_lib, main_case):
    base, segs = main_case
    inside = np.zeros(len(base), bool)
    for o, n in segs:
        inside[o:o + n] = True
    assert np.isnan(base[~inside]).all() and (~inside).sum() > 100
    other = base.copy()
    other[~inside] = values(int((~inside).sum()), 9)
    a, b = run(built_lib, base, segs), run(built_lib, other, segs)
    assert np.array_equal(a[0], b[0]) and np.array_equal(bits64(a[1]), bits64(b[1])) and np.array_equal(a[2], b[2])


def test_three_hundred_segments_with_a_single_float_between_two_long_ones(built_lib):
    Cc = built_lib.STATS_CHUNK
    rng = np.random.default_rng(11)
    sizes = [int(n) for n in rng.integers(0, 200, 300)]
    sizes[148:151] = [3 * Cc, 1, 3 * Cc]
    base, segs = layout([(n, int(a)) for n, a in zip(sizes, rng.integers(0, 4, 300))], gap=1)
    assert len(segs) == 300 and [n for _, n in segs[148:151]] == [3 * Cc, 1, 3 * Cc]
    counts, moments, hist = compare(run(built_lib, base, segs), base, segs, label='300 segments')
    for i in [148, 149, 150] + list(range(0, 300, 25)):
        c1, m1, h1 = run(built_lib, base, [segs[i]])
        assert np.array_equal(c1[0], counts[i]) and np.array_equal(h1[0], hist[i]) and np.array_equal(bits64(m1[0]), bits64(moments[i])), i


@pytest.mark.parametrize('e_lo,e_hi,s', [(-24, 15, 0), (-24, 15, 3), (3, 3, 1), (0, 0, 0), (-126, 127, 3), (-126, 127, 0), (127, 127, 2)])
def test_other_buckets(built_lib, main_case, e_lo, e_hi, s):
    base, segs = main_case
    compare(run(built_lib, base, segs, e_lo, e_hi, s), base, segs, e_lo, e_hi, s, label='e_lo %d e_hi %d s %d' % (e_lo, e_hi, s))


def test_only_empty_segments_and_only_non_finite_values(built_lib):
    base = np.array([np.nan, np.inf, -np.inf, np.nan, 1.0, np.nan, np.nan, np.nan], dtype=np.float32)
    for segs in ([(0, 0), (3, 0), (8, 0)], [(0, 4), (5, 3), (1, 2)]):
        counts, moments, hist = compare(run(built_lib, base, segs), base, segs, label='nothing finite')
        assert not hist.any() and moments.tolist() == [[0.0, 0.0, np.inf, -np.inf, 0.0]] * 3


def test_a_plan_serves_many_calls_and_default_buffers(built_lib, main_case):
    base, segs = main_case
    plan = built_lib.tensor_stats_plan(segs, len(base))
    x = torch.from_numpy(base).cuda()
    a = built_lib.tensor_stats(x, plan)
    x2 = x.clone()
    x2[segs[20][0]:segs[20][0] + segs[20][1]] = 1.0
    b = built_lib.tensor_stats(x2, plan)
    torch.cuda.synchronize()
    assert a.hist.shape == (len(segs), 321) and a.counts.dtype == torch.int64 and a.moments.dtype == torch.float64
    compare(tuple(t.cpu().numpy() for t in a), base, segs, label='fresh buffers')
    compare(tuple(t.cpu().numpy() for t in b), x2.cpu().numpy(), segs, label='same plan, other values')


def test_graph_capture(built_lib, main_case):
    """one captured call replays to the eager results, bit for bit, and follows what the buffer holds at replay time"""
    base, segs = main_case
    lib = built_lib
    plan = lib.tensor_stats_plan(segs, len(base))
    x = torch.from_numpy(base).cuda()
    out = lib.tensor_stats(x, plan)
    work = torch.empty(lib.tensor_stats_workspace_bytes(plan.n, plan.n_items, 321), dtype=torch.uint8, device='cuda')
    torch.cuda.synchronize()
    ref = tuple(t.clone() for t in out)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        lib.tensor_stats(x, plan, counts=out.counts, moments=out.moments, hist=out.hist, work=work)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            lib.tensor_stats(x, plan, counts=out.counts, moments=out.moments, hist=out.hist, work=work)
    torch.cuda.synchronize()
    for t in out:
        t.view(torch.int64).fill_(-1)
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.int64), b.view(torch.int64)) for a, b in zip(out, ref))
    other = values(len(base), 77)
    x.copy_(torch.from_numpy(other))
    g.replay()
    torch.cuda.synchronize()
    compare(tuple(t.cpu().numpy() for t in out), other, segs, label='replay, other values')


def test_bad_arguments_enqueue_nothing(built_lib):
    lib = built_lib
    plan = lib.tensor_stats_plan([(0, 5), (8, 3)], 16)
    x = torch.zeros(20, device='cuda')
    counts = torch.full((2, 6), -1, dtype=torch.int64, device='cuda')
    moments = torch.full((2, 5), float('nan'), dtype=torch.float64, device='cuda')
    hist = torch.full((2, 321), -1, dtype=torch.int64, device='cuda')
    work = torch.zeros(lib.tensor_stats_workspace_bytes(2, plan.n_items, 321), dtype=torch.uint8, device='cuda')
    P = lib.ptr
    import ctypes as C
    hdr = C.c_void_p(plan.header.ctypes.data)
    other = plan.header.copy()
    other[1] = 3
    good = dict(base=P(x), plan=P(plan.dev), header=hdr, n=2, n_items=plan.n_items, e_lo=-24, e_hi=15, s=2, counts=P(counts), moments=P(moments),
                hist=P(hist), work=P(work))
    cases = [(dict(base=None), 'NULL'), (dict(plan=None), 'NULL'), (dict(header=None), 'NULL'), (dict(counts=None), 'NULL'),
             (dict(moments=None), 'NULL'), (dict(hist=None), 'NULL'), (dict(work=None), 'NULL'), (dict(n=0), 'n=0'),
             (dict(n=lib.STATS_MAX_SEGMENTS + 1), 'n=4097'), (dict(e_lo=-127), 'e_lo=-127'), (dict(e_hi=128), 'e_hi=128'),
             (dict(e_lo=16), 'e_lo=16'), (dict(s=4), 'sub_bits=4'), (dict(s=-1), 'sub_bits=-1'), (dict(n=1), 'header'),
             (dict(n_items=plan.n_items + 1), 'header'), (dict(header=C.c_void_p(other.ctypes.data)), 'header'),
             (dict(base=C.c_void_p(x.data_ptr() + 4)), '16-byte')]
    for kw, word in cases:
        a = dict(good, **kw)
        rc = lib._lib.taco_tensor_stats(a['base'], a['plan'], a['header'], a['n'], a['n_items'], a['e_lo'], a['e_hi'], a['s'], a['counts'],
                                        a['moments'], a['hist'], a['work'], lib.stream_ptr())
        assert rc == -1, kw
        assert lib.last_error().startswith('tensor_stats:') and word in lib.last_error(), (kw, lib.last_error())
    torch.cuda.synchronize()
    assert (counts == -1).all() and torch.isnan(moments).all() and (hist == -1).all() and not work.any()
    with pytest.raises(ValueError):
        lib.tensor_stats(x[1:], lib.tensor_stats_plan([(0, 5)], 16))          # a view that is not 16-byte aligned
    with pytest.raises(ValueError):
        lib.tensor_stats(x, plan, work=work[:-8])
