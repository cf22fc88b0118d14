"""Poisoned buffers and guard bands: the tools the suite has for uninitialised reads and out-of-bounds writes.

The C ABI's contract is that workspace, outputs and scratch arrive with ARBITRARY contents (include/taco_hip.h; the host class
allocates them with torch.empty), apart from the `dec.err` block that taco_clear_error zeroes.  A test that wants to hold a
kernel to that contract
  - carves its buffers out of one allocation, each between guard bands of a sentinel bit pattern (`carve`), so that a store
    outside a buffer lands in a band and is found afterwards (`guards_intact`);
  - fills the buffers with a poison pattern in front of the call (`poison`), so that a read of something the call never wrote
    changes the result, and an output element the call never wrote still holds the pattern (`untouched` / `fully_written`).
Plain functions over torch tensors; they work on CPU tensors (tests/test_poison_host.py) and import without a GPU.

Patterns, applied by bit pattern to 4-byte words:
  qnan   0x7fc00000  a read that reaches an output makes it non-finite
  ones   0xffffffff  also a NaN; as int32 -1, as uint8 255 (counters, tickets, flags, byte masks)
  noise  seeded finite values, one half of the scale of the model's activations and one half 1e3 times that: survives
         NaN-blind readers (`x > 0 ? x : 0`, a max, fmaxf) and still changes an accumulated result
  zeros  the state every other test of the suite starts from (the clean comparison run)
`foreign` is not a fill but a history -- an earlier complete call on the same workspace with other parameters and inputs; the
tests build it themselves (tests/test_gpu_poison.py).
"""
import numpy as np
import torch

ALIGN_FLOATS = 64                 # 256 bytes: what torch's caching allocator gives every tensor of the other tests
GUARD_WORD = 0x7fa5c3d2           # sentinel of the guard bands (a signalling-NaN pattern no fill and no kernel produces)
QNAN_WORD = 0x7fc00000
ONES_WORD = 0xffffffff
PATTERNS = ('qnan', 'ones', 'noise')
NOISE_BLOCK = 1 << 20

# Workspace ranges that may keep prior contents although a kernel reads them, each by workspace-table name with the proof that
# the value read cannot reach a result next to it.  May never name dec.xchg, a bwd.* accumulator or a documented output.
EXEMPT = {}


def _i32(word):
    """the 32-bit pattern as the Python int torch wants for an int32 fill"""
    return word - (1 << 32) if word >= (1 << 31) else word


def _up(n, a=ALIGN_FLOATS):
    return (int(n) + a - 1) // a * a


class Arena:
    """One allocation: guard band, buffer, guard band, buffer, ..., guard band.  `raw` is the int32 view of the 256-byte aligned
    part; `spans[name] = (offset, size)` in floats; band i lies in front of buffer i, the last band behind the last buffer, and
    every band runs from the very end of one buffer to the start of the next."""

    def __init__(self, raw, names, spans, total):
        self.raw, self.names, self.spans, self.total = raw, names, spans, total

    def f32(self, name, *dims):
        o, n = self.spans[name]
        t = self.raw[o:o + n].view(torch.float32)
        return t.view(*dims) if dims else t

    def view(self, name, dtype, *dims):
        """the buffer's bytes as `dtype` (all of them, or the first prod(dims) elements shaped `dims`)"""
        o, n = self.spans[name]
        t = self.raw[o:o + n].view(dtype)
        if dims:
            t = t[:int(np.prod(dims))].view(*dims)
        return t

    def bands(self):
        """[(start, end, adjoining buffer, 'before' | 'after')] in floats"""
        out, pos = [], 0
        for name in self.names:
            o, n = self.spans[name]
            out.append((pos, o, name, 'before'))
            pos = o + n
        out.append((pos, self.total, self.names[-1], 'after'))
        return out


def carve(sizes, guard_floats=256, device='cpu'):
    """sizes: {name: floats} (or a list of pairs; order kept).  Every buffer starts on a 256-byte boundary and has at least
    `guard_floats` sentinel words in front of it and directly behind its last float."""
    items = list(sizes.items()) if isinstance(sizes, dict) else list(sizes)
    assert items and all(int(n) > 0 for _, n in items), 'carve: empty arena or empty buffer'
    guard = _up(max(int(guard_floats), 1))
    spans, pos = {}, guard
    for name, n in items:
        assert name not in spans, 'carve: duplicate buffer name %r' % name
        spans[name] = (pos, int(n))
        pos = _up(pos + int(n) + guard)
    total = pos
    store = torch.empty(total + ALIGN_FLOATS, dtype=torch.int32, device=device)
    skip = (-(store.data_ptr() // 4)) % ALIGN_FLOATS          # (a CPU allocation is 64-byte aligned only)
    raw = store[skip:skip + total]
    assert raw.data_ptr() % (4 * ALIGN_FLOATS) == 0
    raw.fill_(_i32(GUARD_WORD))
    return Arena(raw, [k for k, _ in items], spans, total)


class GuardReport:
    """Truthy when every band holds the sentinel; else `byte_offset` (from the arena's start) of the first damaged byte, the
    buffer it adjoins and on which side."""

    def __init__(self, ok, byte_offset=None, buffer=None, side=None):
        self.ok, self.byte_offset, self.buffer, self.side = ok, byte_offset, buffer, side

    def __bool__(self):
        return self.ok

    def __repr__(self):
        if self.ok:
            return 'guard bands intact'
        return 'guard band damaged at byte %d, %s buffer %r' % (self.byte_offset, self.side, self.buffer)


_GUARD_BYTES = np.frombuffer(np.array([GUARD_WORD], dtype='<u4').tobytes(), dtype=np.uint8)


def guards_intact(arena):
    for lo, hi, name, side in arena.bands():
        band = arena.raw[lo:hi]
        if bool((band == _i32(GUARD_WORD)).all()):
            continue
        got = band.view(torch.uint8).cpu().numpy()
        bad = np.flatnonzero(got != np.tile(_GUARD_BYTES, hi - lo))
        at = int(bad[0])
        if side == 'before' and lo > 0:
            # a band between two buffers: damage in its first half is an overrun of the buffer in front of it
            prev = arena.names[arena.names.index(name) - 1]
            if at < (hi - lo) * 2:
                name, side = prev, 'after'
        return GuardReport(False, lo * 4 + at, name, side)
    return GuardReport(True)


def _noise_block(seed, scale, n):
    g = torch.Generator(device='cpu').manual_seed(int(seed))
    x = torch.randn(n, generator=g, dtype=torch.float32)
    x = torch.where(x.abs() < 1e-3, torch.full_like(x, 0.37), x)      # (never 0: a written zero must differ from the poison)
    amp = torch.where(torch.arange(n) % 2 == 0, torch.tensor(float(scale)), torch.tensor(1e3 * float(scale)))
    return x * amp


def poison(buf, pattern, seed=0, scale=1.0):
    """Fills `buf` (any dtype whose byte count is a multiple of 4; contiguous) with the pattern.  Returns what `untouched` /
    `fully_written` need to recognise it afterwards: the pattern's name, or for `noise` a copy of the fill."""
    words = buf.view(-1).view(torch.int32)
    if pattern == 'qnan':
        words.fill_(_i32(QNAN_WORD))
    elif pattern == 'ones':
        words.fill_(_i32(ONES_WORD))
    elif pattern == 'zeros':
        words.zero_()
    elif pattern == 'noise':
        n = words.numel()
        block = _noise_block(seed, scale, min(n, NOISE_BLOCK)).to(buf.device)
        reps = -(-n // block.numel())
        fill = block if reps == 1 else block.repeat(reps)[:n]
        words.copy_(fill.view(torch.int32))
        return fill.view(torch.int32).clone()
    else:
        raise ValueError('poison: unknown pattern %r' % (pattern,))
    return pattern


def _int_view(buf):
    t = buf.contiguous().view(-1)
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def untouched(buf, mark):
    """Boolean tensor over the flattened elements of `buf`: True where the element still holds the poison bit pattern.
    `mark` is what `poison` returned.  Elements narrower than 4 bytes are compared with the matching part of the word (`ones`:
    255 / -1; `qnan` and `noise` by their position in the word), wider ones (int64) with both halves."""
    v = _int_view(buf)
    size = v.element_size()
    if isinstance(mark, str) and size == 4:
        return v == _i32({'qnan': QNAN_WORD, 'ones': ONES_WORD, 'zeros': 0}[mark])
    if isinstance(mark, str):
        word = {'qnan': QNAN_WORD, 'ones': ONES_WORD, 'zeros': 0}[mark]
        ref_bytes = np.frombuffer(np.array([word], dtype='<u4').tobytes(), dtype=np.uint8)
        nbytes = v.numel() * size
        ref = torch.from_numpy(np.tile(ref_bytes, -(-nbytes // 4))[:nbytes].copy())
    else:
        ref = mark.view(-1).view(torch.uint8).cpu()
        assert ref.numel() >= v.numel() * size, 'untouched: the saved noise is shorter than the buffer'
        ref = ref[:v.numel() * size]
    ref = ref.view(v.dtype).to(v.device)
    return v == ref


def fully_written(buf, mark):
    """(ok, first, count): ok when no element of `buf` holds the poison any more; else the flat index of the first one that does
    and how many do."""
    m = untouched(buf, mark)
    count = int(m.sum())
    if count == 0:
        return True, None, 0
    return False, int(torch.nonzero(m)[0]), count


def table_gaps(workspace_table, total_floats):
    """Float ranges [(start, end)] of a workspace of `total_floats` that no row of taco_workspace_table covers (the 64-float
    alignment padding between tensors).  Rows are (name, offset, size, dims); rows may overlap."""
    spans = sorted((int(o), int(o) + int(s)) for _, o, s, _ in workspace_table)
    gaps, pos = [], 0
    for lo, hi in spans:
        if lo > pos:
            gaps.append((pos, lo))
        pos = max(pos, hi)
    if pos < total_floats:
        gaps.append((pos, int(total_floats)))
    assert pos <= total_floats, 'table_gaps: a row ends at %d, behind the workspace (%d floats)' % (pos, total_floats)
    return gaps


def rows_with_prefix(workspace_table, prefix, exclude=('dec.err',)):
    """[(offset, size)] of the rows whose name is `prefix` or starts with it (localisation), without the names in `exclude`."""
    return [(int(o), int(s)) for n, o, s, _ in workspace_table
            if (n == prefix or n.startswith(prefix)) and n not in exclude]


class Guarded:
    """Op-level convenience: tensors of given shape / dtype / fill carved from one arena.
    specs: {name: (shape, dtype, fill)}, fill one of the pattern names, 'zeros', or a float (plain fill value, e.g. 7.0).
    G[name] is the tensor; G.check(*written) asserts that the guard bands are intact, that the bytes between a buffer's last
    element and its 4-byte boundary kept their fill, and that none of the `written` buffers still holds its poison."""

    def __init__(self, specs, device='cuda', guard_floats=1024, seed=0):
        self.specs, self.seed = dict(specs), seed
        sizes, self.marks, self.t = [], {}, {}
        for name, (shape, dtype, fill) in self.specs.items():
            nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
            sizes.append((name, max(1, -(-nbytes // 4))))
        self.arena = carve(sizes, guard_floats, device)
        for i, (name, (shape, dtype, fill)) in enumerate(self.specs.items()):
            whole = self.arena.f32(name)
            if isinstance(fill, str):
                self.marks[name] = poison(whole, fill, seed=seed + i)
            else:
                whole.fill_(float(fill))
                self.marks[name] = whole.view(torch.int32).clone()
            self.t[name] = self.arena.view(name, dtype, *shape)

    def __getitem__(self, name):
        return self.t[name]

    def refill(self, *names):
        for name in names:
            fill = self.specs[name][2]
            whole = self.arena.f32(name)
            if isinstance(fill, str):
                poison(whole, fill, seed=self.seed + list(self.specs).index(name))
            else:
                whole.fill_(float(fill))

    def check(self, *written):
        rep = guards_intact(self.arena)
        assert rep, repr(rep)
        for name, (shape, dtype, fill) in self.specs.items():
            raw = self.arena.view(name, torch.uint8)
            used = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
            if used < raw.numel():
                mark = self.marks[name]
                word = torch.empty(1, dtype=torch.int32)
                if isinstance(mark, str):
                    poison(word, mark)
                    ref = word.view(torch.uint8)[used % 4:].to(raw.device)
                else:
                    ref = mark.view(torch.uint8)[used:]
                assert torch.equal(raw[used:], ref), 'bytes behind the last element of %r were written' % name
        for name in written:
            ok, first, count = fully_written(self.t[name], self._mark_for(name))
            assert ok, '%d element(s) of %r still hold the fill, first at flat index %d' % (count, name, first)

    def _mark_for(self, name):
        return self.marks[name]

    def margin_intact(self, name, mask):
        """True when every element of G[name] selected by the boolean `mask` (same shape) still holds its fill, bytewise"""
        return bool(untouched(self.t[name], self._mark_for(name)).view(self.t[name].shape)[mask].all())
