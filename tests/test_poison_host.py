"""CPU: the poison / guard-band helper (tests/poison.py) itself -- carving and alignment, each pattern's bit image, and that the
checks DO fire: three planted mistakes of a Python stand-in "kernel" on CPU tensors (a store one float past a buffer, an output
element left unwritten, an add into an accumulator nobody cleared) must each be reported, at the right place."""
import numpy as np
import pytest
import torch

from tests import poison


def _bits(t):
    return t.contiguous().view(-1).view(torch.int32).numpy().view(np.uint32)


def test_carve_alignment_order_and_bands():
    sizes = [('ws', 1000), ('out', 77), ('loss', 3), ('grads', 64)]
    a = poison.carve(sizes, guard_floats=100)
    assert a.names == ['ws', 'out', 'loss', 'grads']
    end = 0
    for name, n in sizes:
        o, s = a.spans[name]
        t = a.f32(name)
        assert s == n and t.numel() == n and t.dtype == torch.float32
        assert t.data_ptr() % 256 == 0, '%s does not start on a 256-byte boundary' % name
        assert o - end >= 100, 'fewer than guard_floats sentinel words in front of %s' % name
        end = o + n
    assert a.total - end >= 100
    # the bands tile everything that is not a buffer, and start at the very float behind each buffer
    bands = a.bands()
    assert sum(hi - lo for lo, hi, _, _ in bands) + sum(n for _, n in sizes) == a.total
    assert [lo for lo, _, _, _ in bands[1:]] == [a.spans[n][0] + a.spans[n][1] for n, _ in sizes]
    assert np.all(_bits(a.raw[bands[0][0]:bands[0][1]]) == poison.GUARD_WORD)
    assert poison.guards_intact(a)
    # a buffer is a view of the arena, not a copy
    a.f32('loss')[1] = 5.0
    assert a.raw[a.spans['loss'][0] + 1].item() == np.float32(5.0).view(np.int32)
    assert a.view('out', torch.uint8).numel() == 77 * 4 and a.view('out', torch.int32, 7, 11).shape == (7, 11)
    assert a.f32('grads', 8, 8).shape == (8, 8)
    with pytest.raises(AssertionError):
        poison.carve({'x': 0})


def test_pattern_bit_images():
    buf = torch.zeros(4099)
    assert poison.poison(buf, 'qnan') == 'qnan'
    assert np.all(_bits(buf) == 0x7fc00000) and bool(torch.isnan(buf).all())
    poison.poison(buf, 'ones')
    assert np.all(_bits(buf) == 0xffffffff) and bool(torch.isnan(buf).all())
    assert bool((buf.view(torch.int32) == -1).all()) and bool((buf.view(torch.uint8) == 255).all())
    saved = poison.poison(buf, 'noise', seed=7, scale=2.0)
    x = buf.numpy()
    assert np.isfinite(x).all() and not (x == 0).any()
    small, big = np.abs(x[0::2]), np.abs(x[1::2])
    assert 0.5 < np.sqrt((small ** 2).mean()) / 2.0 < 2.0 and 0.5 < np.sqrt((big ** 2).mean()) / 2e3 < 2.0
    again = torch.empty(4099)
    poison.poison(again, 'noise', seed=7, scale=2.0)
    other = torch.empty(4099)
    poison.poison(other, 'noise', seed=8, scale=2.0)
    assert torch.equal(buf, again) and not torch.equal(buf, other)
    assert np.array_equal(saved.numpy().view(np.uint32), _bits(buf))
    poison.poison(buf, 'zeros')
    assert not buf.any()
    # other element types are filled through their bytes
    b8 = torch.zeros(1024, dtype=torch.uint8)
    poison.poison(b8, 'ones')
    assert bool((b8 == 255).all())
    i32 = torch.zeros(6, dtype=torch.int32)
    poison.poison(i32, 'ones')
    assert i32.tolist() == [-1] * 6
    with pytest.raises(ValueError):
        poison.poison(buf, 'salt')
    # a buffer longer than one noise block repeats the block
    long = torch.empty(poison.NOISE_BLOCK + 5)
    poison.poison(long, 'noise', seed=1)
    assert torch.equal(long[:5], long[poison.NOISE_BLOCK:])


@pytest.mark.parametrize('pattern', ['qnan', 'ones', 'noise'])
def test_untouched_and_fully_written(pattern):
    buf = torch.empty(300)
    mark = poison.poison(buf, pattern, seed=3)
    assert bool(poison.untouched(buf, mark).all())
    assert poison.fully_written(buf, mark) == (False, 0, 300)
    buf[:] = torch.arange(300, dtype=torch.float32)        # (0.0 included: a written zero is written)
    assert poison.fully_written(buf, mark) == (True, None, 0)
    fresh = torch.empty(300)
    poison.poison(fresh, pattern, seed=3)
    buf[17], buf[255] = fresh[17], fresh[255]
    assert poison.fully_written(buf, mark) == (False, 17, 2)
    assert torch.nonzero(poison.untouched(buf, mark)).view(-1).tolist() == [17, 255]


def test_untouched_on_narrow_and_wide_elements():
    b8 = torch.empty(1001 + 3, dtype=torch.uint8)
    mark = poison.poison(b8, 'ones')
    b8[:1001] = 1
    assert torch.nonzero(poison.untouched(b8, mark)).view(-1).tolist() == [1001, 1002, 1003]
    h = torch.empty(10, dtype=torch.float16)
    mark = poison.poison(h, 'qnan')
    h[:9] = 1.5
    assert torch.nonzero(poison.untouched(h, mark)).view(-1).tolist() == [9]
    h[:9] = 0.0
    assert torch.nonzero(poison.untouched(h, mark)).view(-1).tolist() == [0, 2, 4, 6, 8, 9]
    # (the low half of the qnan word is 0x0000: a half-precision ZERO at an even index reads as untouched -- fp16 outputs are
    #  therefore poisoned with `ones`, whose every byte differs from a zero)
    h2 = torch.empty(10, dtype=torch.float16)
    mark = poison.poison(h2, 'ones')
    h2[:] = 0.0
    assert poison.fully_written(h2, mark)[0]
    q = torch.empty(4, dtype=torch.int64)
    mark = poison.poison(q, 'ones')
    q[1] = 12
    assert torch.nonzero(poison.untouched(q, mark)).view(-1).tolist() == [0, 2, 3]


def _standin_scale(src, dst, n, start=0):
    """the stand-in "kernel": dst[i] = 2 src[i] for i in [start, n) -- host code on CPU tensors"""
    for i in range(start, n):
        dst[i] = 2.0 * src[i]


def test_planted_store_one_float_past_a_buffer_is_reported():
    a = poison.carve([('x', 40), ('y', 40), ('z', 8)], guard_floats=64)
    for name in a.names:
        poison.poison(a.f32(name), 'qnan')
    x, y = a.f32('x'), a.f32('y')
    x[:] = torch.arange(40, dtype=torch.float32)
    _standin_scale(x, y, 40)
    assert poison.guards_intact(a) and poison.fully_written(y, 'qnan')[0]
    # the mistake: n + 1 elements -- the store lands on the first float behind y (written through the arena, as a device pointer would)
    o, n = a.spans['y']
    wide = a.raw[o:o + n + 1].view(torch.float32)
    _standin_scale(torch.cat([x, x[:1]]), wide, 41)
    rep = poison.guards_intact(a)
    assert not rep and rep.buffer == 'y' and rep.side == 'after' and rep.byte_offset == (o + n) * 4, rep
    assert 'y' in repr(rep) and str((o + n) * 4) in repr(rep)
    # ... and one float in front of z, one byte only
    a.raw[o + n] = poison._i32(poison.GUARD_WORD)
    assert poison.guards_intact(a)
    oz = a.spans['z'][0]
    a.raw[oz - 1:oz].view(torch.uint8)[2] = 0
    rep = poison.guards_intact(a)
    assert not rep and rep.buffer == 'z' and rep.side == 'before' and rep.byte_offset == (oz - 1) * 4 + 2, rep
    # a store in front of the first buffer
    a.raw[oz - 1] = poison._i32(poison.GUARD_WORD)
    a.raw[a.spans['x'][0] - 1] = 0
    rep = poison.guards_intact(a)
    assert not rep and rep.buffer == 'x' and rep.side == 'before', rep


@pytest.mark.parametrize('pattern', ['qnan', 'ones', 'noise'])
def test_planted_unwritten_output_element_is_reported(pattern):
    a = poison.carve([('x', 33), ('y', 33)])
    x, y = a.f32('x'), a.f32('y')
    x[:] = torch.linspace(-1, 1, 33)
    mark = poison.poison(y, pattern, seed=5)
    _standin_scale(x, y, 33, start=1)          # the mistake: the loop starts at 1, element 0 is never stored
    assert poison.fully_written(y, mark) == (False, 0, 1)
    assert poison.guards_intact(a)
    _standin_scale(x, y, 33)
    assert poison.fully_written(y, mark)[0]


@pytest.mark.parametrize('pattern', ['qnan', 'ones', 'noise'])
def test_planted_add_into_an_uncleared_accumulator_is_reported(pattern):
    """A column sum that ACCUMULATES into its output (as the atomics of the weight-gradient kernels do) and forgot the fill in
    front: on a zeroed buffer it is right, on every poison it differs from the clean run -- `noise` included, which is the
    pattern a NaN-blind reader (here: a ReLU on the sum) needs."""
    rows = torch.linspace(-2, 3, 24 * 16).view(24, 16)

    def colsum(acc, clear):
        if clear:
            acc.zero_()
        for r in rows:
            acc += r
        return torch.where(acc > 0, acc, torch.zeros_like(acc))     # x > 0 ? x : 0 maps NaN to 0

    clean = torch.zeros(16)
    want = colsum(clean, clear=False).clone()          # the state every other test starts from: the mistake is invisible
    a = poison.carve([('acc', 16)])
    acc = a.f32('acc')
    poison.poison(acc, pattern, seed=9, scale=1.0)
    got = colsum(acc, clear=False)
    same = np.array_equal(_bits(got), _bits(want))
    if pattern == 'noise':
        assert not same, 'noise must survive the NaN-blind select'
        assert int((got != want).sum()) >= 8
    else:
        assert not same                                   # NaN + x = NaN, selected to 0: differs wherever the clean sum is positive
    poison.poison(acc, pattern, seed=9, scale=1.0)
    assert np.array_equal(_bits(colsum(acc, clear=True)), _bits(want))
    assert poison.guards_intact(a)


def test_table_gaps_and_row_groups():
    table = [('a.x', 0, 100, (100,)), ('a.y', 128, 64, (64,)), ('b.z', 192, 10, (10,)), ('b.alias', 130, 20, (20,)),
             ('dec.err', 256, 512, (512,)), ('dec.xchg', 768, 32, (32,))]
    assert poison.table_gaps(table, 832) == [(100, 128), (202, 256), (800, 832)]
    assert poison.table_gaps(table, 800) == [(100, 128), (202, 256)]
    with pytest.raises(AssertionError):
        poison.table_gaps(table, 700)
    assert poison.rows_with_prefix(table, 'a.') == [(0, 100), (128, 64)]
    assert poison.rows_with_prefix(table, 'dec.') == [(768, 32)]
    assert poison.rows_with_prefix(table, 'dec.xchg') == [(768, 32)]


@pytest.mark.parametrize('train', [True, False])
def test_workspace_table_gaps_of_the_built_library(built_lib, train):
    """The library loads without a GPU: the gaps of the real layouts are alignment padding only (fewer than 64 floats each),
    every row starts on a 64-float boundary, and no row reaches past taco_workspace_bytes."""
    for B, Tt, Td, r, V, S in ((2, 9, 5, 2, 20, 1), (4, 37, 12, 2, 40, 1), (11, 41, 9, 5, 33, 1), (3, 13, 7, 3, 17, 1),
                               (32, 200, 180, 2, 60, 1), (2, 9, 5, 2, 20, 4)):
        sh = built_lib.make_shape(B, Tt, Td, r, V, S)
        table = built_lib.workspace_table(sh, train)
        total = built_lib.workspace_bytes(sh, train) // 4
        gaps = poison.table_gaps(table, total)
        assert all(0 < hi - lo < 64 for lo, hi in gaps), gaps
        assert all(o % 64 == 0 for _, o, _, _ in table)
        assert sum(hi - lo for lo, hi in gaps) < 64 * len(table)
        names = [n for n, _, _, _ in table]
        assert 'dec.err' in names and 'dec.xchg' in names
        assert not any(n == 'dec.xchg' or n.startswith('bwd.') for n in poison.EXEMPT)


def test_guarded_buffers_for_op_tests():
    G = poison.Guarded({'C': ((5, 7), torch.float32, 'qnan'), 'dW': ((3, 4), torch.float32, 7.0),
                        'bytes': ((1001,), torch.uint8, 'ones'), 'half': ((3, 5), torch.float16, 'ones'),
                        'slab': ((100,), torch.float32, 'noise'), 'n': ((4,), torch.int32, 'ones')}, device='cpu', guard_floats=64)
    assert G['C'].shape == (5, 7) and G['bytes'].dtype == torch.uint8 and G['half'].shape == (3, 5)
    assert bool((G['dW'] == 7.0).all()) and bool(torch.isnan(G['C']).all()) and G['n'].tolist() == [-1] * 4
    assert all(G[k].data_ptr() % 256 == 0 for k in G.t)
    G.check()
    with pytest.raises(AssertionError, match="'C' still hold"):
        G.check('C')
    G['C'][:] = 1.0
    G['bytes'][:] = 0
    G['half'][:] = 0.0
    G['n'][:] = 3
    G.check('C', 'bytes', 'half', 'n')
    # a strided consumer: columns [0, 5) of C written, the margin [5, 7) keeps its fill bytewise
    G.refill('C')
    G['C'][:, :5] = 2.0
    margin = torch.zeros(5, 7, dtype=torch.bool)
    margin[:, 5:] = True
    assert G.margin_intact('C', margin)
    G['C'][2, 6] = 0.0
    assert not G.margin_intact('C', margin)
    # the stand-in writes 1004 bytes into the 1001-byte buffer: the bytes behind the last element are watched too
    G.arena.view('bytes', torch.uint8)[1001] = 0
    with pytest.raises(AssertionError, match='behind the last element'):
        G.check()
    G.arena.view('bytes', torch.uint8)[1001] = 255
    G.check()
    # ... and dW's value fill is recognised as "not written" like a pattern
    with pytest.raises(AssertionError, match="'dW' still hold"):
        G.check('dW')
    o, n = G.arena.spans['slab']
    G.arena.raw[o + n] = 0
    with pytest.raises(AssertionError, match="after buffer 'slab'"):
        G.check()


def test_wrappers_check_the_buffers_a_caller_hands_in(built_lib):
    """lib.griffinlim / denorm_unframe / audio_features take the caller's own out / work buffers (so that a test can poison and
    guard them); a buffer of the wrong shape, type or layout is refused before anything is enqueued."""
    own = built_lib._own_or_given
    dev = torch.device('cpu')
    fresh = own(None, (2, 3), torch.float32, dev, 'x')
    assert fresh.shape == (2, 3) and fresh.dtype == torch.float32
    mine = torch.empty(2, 3)
    assert own(mine, (2, 3), torch.float32, dev, 'x') is mine
    for bad in (torch.empty(3, 2), torch.empty(2, 3, dtype=torch.float16), torch.empty(3, 2).t()):
        with pytest.raises(ValueError, match='x: expected'):
            own(bad, (2, 3), torch.float32, dev, 'x')
