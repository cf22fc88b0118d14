"""tacotron_amd/argcheck.py: the argument checks every entry-point wrapper of lib.py is written in.  Host only, no shared library:
for each checker a table of values the wrappers accept and of the bad ones they rely on it to refuse."""
import numpy as np
import pytest
import torch

from tacotron_amd import argcheck as ac

F32, I32 = torch.float32, torch.int32
CPU, META = torch.device('cpu'), torch.device('meta')   # ('meta': another device object that needs no GPU)


def _strided(*shape):
    """a float32 tensor of that shape whose last dimension has stride 2"""
    return torch.ones(*shape[:-1], shape[-1] * 2)[..., ::2]


TENSOR_GOOD = [   # (x, dtype, shape, device, optional) -> free dimensions
    ((torch.ones(2, 3, 8), F32, ('B', 'C', 'F'), None, False), (2, 3, 8)),
    ((torch.ones(2, 3, 8), F32, (2, 'Fb', 8), CPU, False), (3,)),
    ((torch.ones(4, dtype=I32), I32, (4,), CPU, True), ()),
    ((None, I32, (4,), CPU, True), None),
    ((torch.ones(5, 3, 14, dtype=torch.float16), (torch.float16, F32), ('N', 'Td', 'C'), None, False), (5, 3, 14)),
    ((torch.ones(1, 1), F32, ('B', 'F'), None, False), (1, 1)),
    ((torch.ones(6, 4)[:3].view(3, 1, 4), F32, ('B', 'F', 'C'), None, False), (3, 1, 4)),   # a view, still contiguous
]
TENSOR_BAD = [   # (x, dtype, shape, device, optional), what is wrong
    ((torch.ones(2, 3, 8).double(), F32, ('B', 'C', 'F'), None, False), 'dtype'),
    ((torch.ones(2, 3, 8, dtype=torch.bfloat16), (torch.float16, F32), ('N', 'Td', 'C'), None, False), 'dtype, two allowed'),
    ((torch.ones(3, 8), F32, ('B', 'C', 'F'), None, False), 'rank'),
    ((torch.ones(2, 3, 8, 1), F32, ('B', 'C', 'F'), None, False), 'rank'),
    ((torch.ones(2, 0, 8), F32, ('B', 'C', 'F'), None, False), 'zero-size free dimension'),
    ((torch.ones(0, dtype=torch.int64), torch.int64, ('B',), None, False), 'zero-size free dimension'),
    ((torch.ones(2, 3, 8), F32, (2, 4, 8), None, False), 'exact size'),
    ((torch.ones(5, dtype=I32), I32, (4,), CPU, True), 'exact size'),
    ((torch.ones(3, 2, 8).transpose(0, 1), F32, ('B', 'C', 'F'), None, False), 'transposed view'),
    ((_strided(2, 8), F32, (2, 8), None, False), 'strided view'),
    ((torch.ones(4, dtype=I32), I32, (4,), META, False), 'wrong device object'),
    ((torch.ones(4, dtype=I32, device='meta'), I32, (4,), CPU, False), 'wrong device object'),
    ((np.ones((2, 3, 8), np.float32), F32, ('B', 'C', 'F'), None, False), 'numpy array'),
    (([[1.0, 2.0]], F32, ('B', 'F'), None, False), 'list'),
    ((None, I32, (4,), CPU, False), 'None where it is not optional'),
    ((4, I32, (4,), CPU, True), 'an int'),
]


def test_tensor_arg():
    for (x, dtype, shape, dev, optional), want in TENSOR_GOOD:
        assert ac.tensor_arg('f', 'x', x, dtype, shape, dev, optional) == want
    for (x, dtype, shape, dev, optional), why in TENSOR_BAD:
        with pytest.raises(ValueError, match=r'^f: x must be a contiguous .* tensor of shape \(.*, got ') as e:
            ac.tensor_arg('f', 'x', x, dtype, shape, dev, optional)
        assert (' on %s, got' % dev in str(e.value)) == (dev is not None), why
    with pytest.raises(ValueError, match=r'float16 or float32 tensor of shape \(N, Td, C\), got bfloat16 \(2, 3, 8\)$'):
        ac.tensor_arg('f', 'src', torch.ones(2, 3, 8, dtype=torch.bfloat16), (torch.float16, F32), ('N', 'Td', 'C'))
    with pytest.raises(ValueError, match=r'mean must be .* shape \(14,\) on cpu, got float32 \(13,\) on cpu$'):
        ac.tensor_arg('f', 'mean', torch.zeros(13), F32, (14,), CPU)
    with pytest.raises(ValueError, match=r'got float32 \(2, 8\) with strides \(16, 2\)$'):
        ac.tensor_arg('f', 'x', _strided(2, 8), F32, ('B', 'F'))
    with pytest.raises(ValueError, match='got a ndarray$'):
        ac.tensor_arg('f', 'x', np.ones(3, np.float32), F32, (3,))
    # empty_ok: only the free dimensions may be empty, everything else is checked as before
    assert ac.tensor_arg('f', 'x', torch.ones(2, 1025, 0), F32, ('B', 1025, 'F'), empty_ok=True) == (2, 0)
    with pytest.raises(ValueError):
        ac.tensor_arg('f', 'x', torch.ones(2, 1024, 0), F32, ('B', 1025, 'F'), empty_ok=True)


INT_GOOD = [((1,), 1), ((0, 0), 0), ((7, 1, 7), 7), ((3.0, 1), 3), ((np.int64(5), 0, 8), 5), ((-2,), -2), ((torch.tensor(4), 1, 4), 4),
            (((1 << 31) - 1, 0, (1 << 31) - 1), (1 << 31) - 1)]
INT_BAD = [(True,), (False, 0), (1.5,), (float('nan'),), (float('inf'),), (None,), ('3',), ([3],), (0, 1), (9, 1, 8), (-1, 0, None),
           (1 << 31, 0, (1 << 31) - 1), (np.float32(2.5), 1), (torch.tensor(1.5), 1)]


def test_int_arg():
    for args, want in INT_GOOD:
        got = ac.int_arg('f', 'n', *args)
        assert type(got) is int and got == want, args
    for args in INT_BAD:
        with pytest.raises(ValueError, match='^f: n must be an integer'):
            ac.int_arg('f', 'n', *args)
    with pytest.raises(ValueError, match=r'an integer in \[1, 8\], got 9$'):
        ac.int_arg('f', 'n', 9, 1, 8)
    with pytest.raises(ValueError, match='an integer >= 1, got 0$'):
        ac.int_arg('f', 'n', 0, 1)
    with pytest.raises(ValueError, match='an integer, got True$'):
        ac.int_arg('f', 'n', True)


def test_unit_interval():
    for x, want in ((0, 0.0), (0.99, 0.99), (0.97, 0.97), (np.float32(0.5), 0.5)):
        assert ac.unit_interval(x, 'f: m') == want
    for bad in (1.0, 1.5, -0.01, float('nan'), float('inf'), 1.0 - 2.0 ** -30):   # (the last one is 1 as a float32)
        with pytest.raises(ValueError, match='^f: m '):
            ac.unit_interval(bad, 'f: m')


def test_host_int32():
    for x, n, want in (([0, 3], 2, [0, 3]), ((5,), 1, [5]), (torch.tensor([1, 2, 3]), 3, [1, 2, 3]), (np.array([4, 5]), 2, [4, 5]),
                       ([2.0, -(1 << 31)], 2, [2, -(1 << 31)]), (range(3), 3, [0, 1, 2])):
        got = ac.host_int32(x, n, 'f: v')
        assert got == want and all(type(v) is int for v in got)
    for x, n in (([0, 3], 3), ([0.5, 1], 2), ([True, 1], 2), ([1 << 31], 1), ([None], 1), (['a'], 1), (7, 1), (torch.tensor([1.0]), 1),
                 (torch.tensor([True]), 1), (torch.ones(2, dtype=I32, device='meta'), 2)):
        with pytest.raises(ValueError, match='^f: v must'):
            ac.host_int32(x, n, 'f: v')


def test_own_or_given():
    fresh = ac.own_or_given(None, (2, 3), torch.int16, CPU, 'f: x')
    assert fresh.shape == (2, 3) and fresh.dtype == torch.int16 and fresh.device == CPU
    assert ac.own_or_given(None, (0,), torch.uint8, CPU, 'f: x').numel() == 0        # (an empty workspace is a size like any other)
    mine = torch.empty(2, 3)
    assert ac.own_or_given(mine, (2, 3), F32, CPU, 'f: x') is mine
    for bad in (torch.empty(2, 4), torch.empty(3, 2), torch.empty(2, 3, dtype=torch.float64), torch.empty(3, 2).t(),
                torch.empty(2, 3, device='meta')):
        with pytest.raises(ValueError, match='f: x: expected'):
            ac.own_or_given(bad, (2, 3), F32, CPU, 'f: x')


def test_no_overlap():
    buf = torch.zeros(64)
    a = buf[:32].view(4, 8)
    for other in (buf[32:].view(4, 8), buf[32:40], torch.zeros(4, 8), None):         # touching but disjoint, elsewhere, absent
        ac.no_overlap('f', 'a', a, 'out', other)
        if other is not None:
            ac.no_overlap('f', 'out', other, 'a', a)
    for other in (a, buf[31:63], buf[:1], buf[16:24], buf.view(torch.int16)[62:66]):   # same, one element in at either end, inside
        with pytest.raises(ValueError, match='^f: out may not overlap a$'):
            ac.no_overlap('f', 'a', a, 'out', other)
    rows = buf.view(4, 16)[:, :8]                                # 4 rows of 8, 16 apart: they span (3 * 16 + 8) floats
    span = (3 * 16 + 8) * 4
    ac.no_overlap('f', 'pieces', rows, 'out', buf[56:], span_in=span)
    with pytest.raises(ValueError, match='^f: out may not overlap pieces$'):
        ac.no_overlap('f', 'pieces', rows, 'out', buf[55:], span_in=span)
    with pytest.raises(ValueError):                              # (between the rows: inside the span all the same)
        ac.no_overlap('f', 'pieces', rows, 'out', buf[8:16], span_in=span)


def test_on_gpu():
    ac.on_gpu('f', 'x', torch.device('cuda', 0))
    ac.on_gpu('f', 'x', torch.device('cuda'))
    for dev in (CPU, META):
        with pytest.raises(ValueError, match=r'^f: x must be on the GPU, got %s \(there is no CPU fallback\)$' % dev):
            ac.on_gpu('f', 'x', dev)


LO, HI = 16384, 262144


def test_step_q_arg():
    assert ac.step_q_arg('f', None, 3, CPU, LO, HI, 'rates') == (None, None)
    for step_q, want in ((65536, [65536] * 3), ([LO, 65536, HI], [LO, 65536, HI]), ((70000, 65536, 20000), [70000, 65536, 20000]),
                         (torch.tensor([65536, 65537, 65538]), [65536, 65537, 65538]), (np.array([HI, HI, HI]), [HI] * 3),
                         (65536.0, [65536] * 3)):
        t, slowest = ac.step_q_arg('f', step_q, 3, CPU, LO, HI, 'rates')
        assert t.dtype == I32 and t.device == CPU and t.tolist() == want and slowest == min(want)
    on_device = torch.ones(3, dtype=I32, device='meta')          # a device tensor is shape-checked, passed through and never read
    t, slowest = ac.step_q_arg('f', on_device, 3, META, LO, HI, 'rates')
    assert t is on_device and slowest == LO
    for bad in (100, HI + 1, [65536, 65536], [65536] * 4, [65536.5, 65536, 65536], [65536, 300000, 65536], [True, 65536, 65536], 'fast',
                torch.tensor([65536.0] * 3), 65536.5, True):
        with pytest.raises(ValueError, match='^f: step_q'):
            ac.step_q_arg('f', bad, 3, CPU, LO, HI, 'rates')
    with pytest.raises(ValueError, match=r'^f: step_q must be in \[16384, 262144\] \(rates\), got 100$'):
        ac.step_q_arg('f', 100, 3, CPU, LO, HI, 'rates')
    for bad in (torch.ones(4, dtype=I32, device='meta'), torch.ones(3, dtype=torch.int64, device='meta'),
                torch.ones(6, dtype=I32, device='meta')[::2]):
        with pytest.raises(ValueError, match='^f: step_q on a device must be a contiguous int32 tensor'):
            ac.step_q_arg('f', bad, 3, META, LO, HI, 'rates')
    with pytest.raises(ValueError, match='step_q on a device'):  # (a device tensor, but of another device than the frames)
        ac.step_q_arg('f', on_device, 3, CPU, LO, HI, 'rates')


def test_pow2_bins():
    for C in (9, 17, 33, 129, 513, 1025):
        ac.pow2_bins('f', C)
    for C in (1, 2, 5, 8, 10, 16, 1024, 1026, 2049):
        with pytest.raises(ValueError, match=r'^f: C - 1 must be a power of two in \[8, 1024\], got C = %d$' % C):
            ac.pow2_bins('f', C)


def test_steps_of(built_lib):
    lib = built_lib
    assert lib.steps_of(None, lib.stretch_step) is None and lib.steps_of(None, lib.pitch_step, 3) is None
    assert lib.steps_of(0.5, lib.stretch_step) == 32768 and lib.steps_of(12, lib.pitch_step, 3) == 32768
    assert lib.steps_of([1.0, 2.0], lib.stretch_step) == [65536, 131072] == lib.steps_of((1.0, 2.0), lib.stretch_step, 2)
    assert lib.steps_of(torch.tensor([0.0, -12.0]), lib.pitch_step) == [65536, 131072] and lib.steps_of([], lib.pitch_step) == []
    assert lib.steps_of(np.array([0.25, 4.0]), lib.stretch_step, 2) == [16384, 262144]
    on_device = torch.ones(2, dtype=I32, device='meta')
    assert lib.steps_of(on_device, lib.stretch_step, 5) is on_device
    for values, to_step, n in (([1.0, 2.0], lib.stretch_step, 3), (5.0, lib.stretch_step, None), ([1.0, 0.1], lib.stretch_step, 2),
                               (float('nan'), lib.pitch_step, None), ([0, 13], lib.pitch_step, None), ('fast', lib.stretch_step, None)):
        with pytest.raises(ValueError):
            lib.steps_of(values, to_step, n)


def test_the_wrappers_are_written_in_the_vocabulary(built_lib):
    """lib.py keeps resolving the names other modules and tests use, and spells none of the shared checks out by hand"""
    lib = built_lib
    assert lib._own_or_given is ac.own_or_given and lib._host_int32 is ac.host_int32 and lib._unit_interval is ac.unit_interval
    assert lib._frames_arg('f', 'x', torch.ones(2, 5, 4)) == (2, 5, 4)
    with pytest.raises(ValueError, match=r'^f: x must be a contiguous float32 tensor of shape \(B, F, C\), got '):
        lib._frames_arg('f', 'x', torch.ones(2, 5))
    src = open(lib.__file__).read()
    assert src.count('is_contiguous()') == 1                     # ptr()'s own assertion
    assert 'isinstance(v, bool)' not in src and 'there is no CPU fallback' not in src
