"""GPU: taco_f0_range_curve (include/taco_hip.h) against the float64 restatement of tests/f0_range_ref.py on the cases of
tests/f0_range_cases.py, within F0_RANGE_STEP_ATOL (sized on the CPU from the float32 restatement, never on the device's output),
and its exact guarantees: the statistics of taco_f0_stats bit for bit, neutral rows copied, TACO_PITCH_ONE behind a row, row
independence, the same bits on a second call and at another alignment, every refusal with its message, one captured graph of
frames_f0 -> f0_range_curve -> frames_pitch_curve, and poisoned inputs behind F_b with guard bands round the outputs.
The worst device error of every case is printed and, when F0_RANGE_ERRORS_OUT names a file, written there
(profiles/f0_range_errors.txt is such a file)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import f0_cases as fc
from tests import f0_ref as fr
from tests import f0_range_cases as rc
from tests import f0_range_ref as rr
from tests import poison
from tests.poison import Guarded

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in rc.all_cases()}
ERRORS = {}     # case -> (elements compared, worst |device - float64| in steps)


@pytest.fixture(scope='module', autouse=True)
def _error_table():
    yield
    out = os.environ.get('F0_RANGE_ERRORS_OUT')
    lines = ['%-28s %8d %10.3f\n' % (k, ERRORS[k][0], ERRORS[k][1]) for k in ERRORS]
    if out and ERRORS:
        with open(out, 'w') as f:
            f.write('# tests/test_gpu_f0_range.py: per case the live elements of step_q compared and the worst |device - float64 restatement|\n'
                    '# in step units; the bar is tests.f0_range_ref.F0_RANGE_STEP_ATOL = %.2f\n' % rr.F0_RANGE_STEP_ATOL)
            f.write('%-28s %8s %10s\n' % ('case', 'elements', 'worst'))
            f.writelines(lines)


def dev(x, dtype=torch.float32):
    return None if x is None else torch.as_tensor(np.asarray(x), dtype=dtype).cuda()


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def run(lib, c, shift=0, fill='qnan', want_stats=True, period=None, frames='case', scale_q='case', base_q='case'):
    """one call on case c -> (step_q, stats | None) as host arrays; the outputs between guard bands, preset to `fill`, every buffer
    `shift` words behind a 256-byte boundary; the bands and the words in front of a shifted output must be intact, every element of
    the outputs written and the inputs unwritten"""
    period = c.period if period is None else period
    frames = c.frames if isinstance(frames, str) else frames
    scale_q = c.scale_q if isinstance(scale_q, str) else scale_q
    base_q = c.base_q if isinstance(base_q, str) else base_q
    B, F = period.shape
    G = Guarded({'period': ((B * F + shift,), torch.float32, 'qnan'), 'base': ((B * F + shift,), torch.int32, 'ones'),
                 'step': ((B * F + shift,), torch.int32, fill), 'stats': ((B * 3 + shift,), torch.float32, fill)})
    p = G['period'][shift:].view(B, F)
    p.copy_(torch.from_numpy(period))
    base = None
    if base_q is not None:
        base = G['base'][shift:].view(B, F)
        base_q = np.array(base_q, dtype=np.int32)
        for b in range(B):   # behind a row's end base_q may hold anything
            base_q[b, rr.row_frames(None if frames is None else frames[b], c.per_unit, F):] = -1
        base.copy_(torch.from_numpy(base_q))
    step, stats = G['step'][shift:].view(B, F), G['stats'][shift:].view(B, 3)
    assert all(t.data_ptr() % 256 == 4 * shift for t in (p, step, stats))
    got = lib.f0_range_curve(p, dev(frames, torch.int32), c.per_unit, dev(scale_q, torch.int32), base, c.smooth, c.limit,
                             out=(step, stats) if want_stats else step, want_stats=want_stats)
    torch.cuda.synchronize()
    assert (got[0] if want_stats else got).data_ptr() == step.data_ptr()
    G.check()
    mark = {k: G.marks[k] for k in ('step', 'stats')}
    for k, t in (('step', step), ('stats', stats)):
        assert bool(poison.untouched(G[k][:shift], mark[k]).all()), 'the words in front of %s were written' % k
    tail = lambda k: poison.untouched(G[k], mark[k])[shift:]   # noqa: E731
    if fill != 'noise':   # (a noise word may equal a result by chance)
        assert not bool(tail('step').any()), 'an element of step_q still holds the fill'
        assert not want_stats or not bool(tail('stats').any()), 'an element of stats still holds the fill'
    assert want_stats or bool(tail('stats').all()), 'stats was written although it was not asked for'
    assert np.array_equal(bits(p.cpu().numpy()), bits(period)), 'period was written'
    if base is not None:
        assert np.array_equal(base.cpu().numpy(), np.asarray(base_q, dtype=np.int32)), 'base_q was written'
    return step.cpu().numpy(), stats.cpu().numpy() if want_stats else None


def check(lib, c):
    """the call against the float64 restatement; its stats against lib.f0_stats on the same input, bit for bit"""
    want, wstats, _ = rr.curve(c.period, c.frames, c.per_unit, c.scale_q, c.base_q, c.smooth, c.limit)
    step, stats = run(lib, c)
    B, F = c.period.shape
    live = np.zeros((B, F), dtype=bool)
    for b in range(B):
        Fb = rr.row_frames(None if c.frames is None else c.frames[b], c.per_unit, F)
        live[b, :Fb] = True
        assert (step[b, Fb:] == rr.ONE).all(), 'row %d: not TACO_PITCH_ONE behind frame %d' % (b, Fb)
        kq = rr.clamp_scale(None if c.scale_q is None else c.scale_q[b])
        if kq == rr.ONE or wstats[b, 0] == 0:     # neutral, or nothing voiced: copied, no rounding question
            assert np.array_equal(step[b], want[b]), 'row %d: a neutral row is not clamp(base) / TACO_PITCH_ONE bit for bit' % b
    assert step.min() >= rr.MIN_STEP and step.max() <= rr.MAX_STEP
    err = rc.step_err(step[live], want[live]) if live.any() else 0.0
    ERRORS[c.name] = (int(live.sum()), err)
    print('  %s: B %d F %d W %d: worst step error %.3f (bar %.2f)' % (c.name, B, F, c.smooth, err, rr.F0_RANGE_STEP_ATOL))
    assert err <= rr.F0_RANGE_STEP_ATOL
    ref = lib.f0_stats(dev(c.period), None, dev(c.frames, torch.int32), c.per_unit)
    torch.cuda.synchronize()
    assert np.array_equal(bits(stats), bits(ref.cpu().numpy())), 'stats differ from taco_f0_stats on the same input'
    assert fc.stats_err(stats, wstats) <= fr.F0_STATS_ATOL
    return step, stats


@pytest.mark.parametrize('name', list(CASES))
def test_against_float64(built_lib, name):
    check(built_lib, CASES[name])


@pytest.mark.parametrize('name', ['F257', 'cap_gaps', 'base_wild', 'gap_64_255_F700', 'smooth_8_short', 'empty_row'])
def test_same_bits_again_misaligned_poisoned_and_without_stats(built_lib, name):
    """a second call, buffers 1 and 3 words behind their boundary, outputs that arrive holding qnan / ones / noise (the inputs
    behind F_b hold NaN in these cases), and stats == NULL: the same bits every time"""
    c = CASES[name]
    step, stats = run(built_lib, c)
    again = run(built_lib, c)
    assert np.array_equal(step, again[0]) and np.array_equal(bits(stats), bits(again[1])), 'a second call gives other bits'
    for shift in (1, 3):
        for fill in poison.PATTERNS:
            s2, t2 = run(built_lib, c, shift=shift, fill=fill)
            assert np.array_equal(step, s2) and np.array_equal(bits(stats), bits(t2)), (shift, fill)
    s3, _ = run(built_lib, c, want_stats=False)
    assert np.array_equal(step, s3), 'stats == NULL changes step_q'


@pytest.mark.parametrize('name', ['F700', 'F65', 'per_unit_7', 'scales_b', 'base_wild', 'cap_gaps'])
def test_rows_are_independent(built_lib, name):
    """row b of the B-row call equals the call on that row alone, and does not change when every other row turns to NaN"""
    c = CASES[name]
    step, stats = run(built_lib, c)
    B = c.period.shape[0]
    for b in range(B):
        one = run(built_lib, c, period=c.period[b:b + 1], frames=None if c.frames is None else c.frames[b:b + 1],
                  scale_q=None if c.scale_q is None else c.scale_q[b:b + 1], base_q=None if c.base_q is None else c.base_q[b:b + 1])
        assert np.array_equal(step[b], one[0][0]) and np.array_equal(bits(stats[b]), bits(one[1][0])), 'row %d alone differs' % b
        spoiled = np.full_like(c.period, np.nan)
        spoiled[b] = c.period[b]
        got = run(built_lib, c, period=spoiled)
        assert np.array_equal(step[b], got[0][b]) and np.array_equal(bits(stats[b]), bits(got[1][b])), 'row %d reads another row' % b


def test_bad_arguments_enqueue_nothing(built_lib):
    """every TACO_EINVAL case returns before a launch: the outputs keep their fill, and the message names the argument"""
    lib = built_lib
    c = CASES['scales_b']
    B, F = c.period.shape
    period, frames, scale, base = dev(c.period), dev((F, F - 1, F), torch.int32), dev(c.scale_q, torch.int32), dev(c.base_q, torch.int32)
    G = Guarded({'step': ((B, F), torch.int32, 7.0), 'stats': ((B, 3), torch.float32, 7.0)})
    fn = C.CDLL(lib.LIB_PATH).taco_f0_range_curve
    fn.restype, fn.argtypes = lib.EXPORTS['taco_f0_range_curve']
    order = ('period', 'frames', 'per_unit', 'scale_q', 'base_q', 'smooth', 'limit', 'step_q', 'stats', 'B', 'F')
    good = dict(period=lib.ptr(period), frames=lib.ptr(frames), per_unit=1, scale_q=lib.ptr(scale), base_q=lib.ptr(base), smooth=2,
                limit=0.5, step_q=lib.ptr(G['step']), stats=lib.ptr(G['stats']), B=B, F=F)
    last = lambda t: C.c_void_p(t.data_ptr() + 4 * (t.numel() - 1))   # noqa: E731
    nan = float('nan')
    cases = [({'period': None}, 'period'), ({'step_q': None}, 'step_q'),
             ({'step_q': good['period']}, 'step_q overlaps period'), ({'step_q': last(period)}, 'step_q overlaps period'),
             ({'period': last(G['step'])}, 'step_q overlaps period'),
             ({'step_q': good['base_q']}, 'step_q overlaps base_q'), ({'step_q': last(base)}, 'step_q overlaps base_q'),
             ({'base_q': last(G['step'])}, 'step_q overlaps base_q'),
             ({'B': 0}, 'B='), ({'B': -1}, 'B='), ({'F': 0}, 'F='), ({'F': -1}, 'F='), ({'F': 8193}, 'F='),
             ({'per_unit': 0}, 'frames_per_unit'), ({'per_unit': -3}, 'frames_per_unit'),
             ({'smooth': -1}, 'smooth'), ({'smooth': 9}, 'smooth'),
             ({'limit': 0.0}, 'limit'), ({'limit': -0.5}, 'limit'), ({'limit': 1.0001}, 'limit'), ({'limit': nan}, 'limit')]
    everything = {k: torch.ones(G[k].shape, dtype=torch.bool, device='cuda') for k in ('step', 'stats')}
    for change, word in cases:
        for nulls in ((), ('frames', 'scale_q', 'stats')):
            if set(nulls) & set(change):
                continue
            a = dict(good)
            a.update({k: None for k in nulls})
            a.update(change)
            lib.griffinlim_workspace_floats(1, 8)   # (a successful call in between: the string below is this refusal's)
            rc_ = fn(*[a[k] for k in order], lib.stream_ptr())
            torch.cuda.synchronize()
            msg = lib.last_error()
            print('  %r%s: rc %d, %s' % (change, ' frames / scale_q / stats NULL' if nulls else '', rc_, msg))
            assert rc_ == -1, (change, rc_)
            assert 'f0_range_curve' in msg and word in msg, (change, msg)
            assert all(G.margin_intact(k, everything[k]) for k in everything), 'an output was written although %r is refused' % (change,)
    G.check()
    assert fn(*[good[k] for k in order], lib.stream_ptr()) == 0              # and the good arguments do run
    torch.cuda.synchronize()
    G.check('step', 'stats')
    want, _, _ = rr.curve(c.period, (F, F - 1, F), 1, c.scale_q, c.base_q, 2, 0.5)
    assert rc.step_err(G['step'].cpu().numpy(), want) <= rr.F0_RANGE_STEP_ATOL


def test_wrapper_arguments(built_lib):
    """the wrapper's own forms of scale_q: None, an int for the batch, a host sequence; a device tensor out of range is clamped there"""
    lib = built_lib
    c = CASES['scales_a']
    p = dev(c.period)
    host = lib.f0_range_curve(p, scale_q=[rc.q(0.0), rc.q(0.5), rc.q(1.0)], smooth=c.smooth, limit=c.limit)
    tens = lib.f0_range_curve(p, scale_q=dev(c.scale_q, torch.int32), smooth=c.smooth, limit=c.limit)
    assert torch.equal(host, tens)
    assert torch.equal(lib.f0_range_curve(p), torch.full_like(host, rr.ONE)), 'scale_q None is not neutral'
    one = lib.f0_range_curve(p, scale_q=lib.range_scale(0.5), smooth=c.smooth, limit=c.limit)
    assert torch.equal(one[1], host[1])
    with pytest.raises(ValueError, match='scale_q'):
        lib.f0_range_curve(p, scale_q=[0, 5 * 65536, 0])


def test_graph_replay_follows_the_device_arguments(built_lib):
    """one capture of frames_f0 -> f0_range_curve -> frames_pitch_curve (a linear graph): the replay equals the eager chain bit for
    bit and reads frames and scale_q at replay time"""
    lib = built_lib
    B, Cw, F, lag_min, lag_max, Q = 3, 33, 72, 3, 30, 8
    x = dev(fc.voices(B, Cw, F, lag_min, lag_max, seed=12))
    plans = (((72, 40, 65), (rc.q(1.5), rc.q(0.5), rc.q(1.0))), ((13, 72, 0), (rc.q(0.0), rc.q(4.0), rc.q(1.5))))
    frames, scale = dev(plans[0][0], torch.int32), dev(plans[0][1], torch.int32)
    names = ('period', 'strength', 'step', 'stats', 'out')
    G = Guarded({'period': ((B, F), torch.float32, 'qnan'), 'strength': ((B, F), torch.float32, 'qnan'), 'step': ((B, F), torch.int32, 'ones'),
                 'stats': ((B, 3), torch.float32, 'qnan'), 'out': ((B, Cw, F), torch.float32, 'qnan')})

    def call(period, strength, step, stats, out):
        lib.frames_f0(x, frames, 1, None, None, lag_min, lag_max, 0.9, 0.0, out=(period, strength))
        lib.f0_range_curve(period, frames, 1, scale, None, 1, 0.5, out=(step, stats), want_stats=True)
        lib.frames_pitch_curve(x, frames, step, 1, Q, out=out)

    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call(*[G[k] for k in names])
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            call(*[G[k] for k in names])
    torch.cuda.synchronize()
    seen = []
    for fr_b, sc_b in (plans[0], plans[1], plans[0]):
        frames.copy_(dev(fr_b, torch.int32))
        scale.copy_(dev(sc_b, torch.int32))
        G.refill(*names)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        G.check(*names)
        eager = [torch.empty_like(G[k]) for k in names]
        call(*eager)
        torch.cuda.synchronize()
        for k, e in zip(names, eager):
            assert torch.equal(G[k].view(torch.int32), e.view(torch.int32)), 'replay with frames %s: %s differs from the eager call' % (fr_b, k)
        period = G['period'].cpu().numpy()
        want, _, _ = rr.curve(period, fr_b, 1, sc_b, None, 1, 0.5)
        assert rc.step_err(G['step'].cpu().numpy(), want) <= rr.F0_RANGE_STEP_ATOL
        seen.append(G['step'].cpu().numpy())
    assert np.array_equal(seen[0], seen[2]) and not np.array_equal(seen[0], seen[1])
    assert (seen[0] != rr.ONE).any(), 'the tracker found no pitch: the graph moved nothing'
