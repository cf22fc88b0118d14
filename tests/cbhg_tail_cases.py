"""Case table, seeded operands and judges of the op-level tests of the CBHG tail: bigru_fwd_kernel / bigru_bwd_kernel
(csrc/bigru.hip), highway_stack_fwd_kernel / _bwd_kernel in both forms (csrc/highway.hip) and mlp2_kernel forward and backward
(csrc/prenet.hip).  Host only; tests/test_cbhg_tail_host.py drives it with the fp32 restatement (tests/cbhg_tail_ref.py F32),
tests/test_gpu_cbhg_tail.py with the taco_debug_* doors.

A runner (run_gru / run_highway / run_prenet) takes a case and a backend -- an object with the methods of cbhg_tail_ref.F32 --
and returns a Report: every output compared with the fp64 oracle through stage_bars.compare / failures as a whole tensor and row by
row (a row is one (b, t) or one m), the exact-zero checks, and the ReLU decisions that differ from the oracle's.
  forward    the backend's forward on the case's operands
  isolated   the backend's backward fed the ORACLE's forward stash rounded to fp32 (no flips by construction)
  chained    the backend's backward fed its own forward stash, as the model runs it; the ReLU decisions are read from that stash and
             forced on the oracle (tests/decisions.py), each flip must have an fp64 margin <= FLIP_MARGIN and a case may have at
             most MAX_FLIPS of them
"""
import collections
import functools
import zlib

import numpy as np

from tests import cbhg_tail_ref as ref
from tests import decisions as dn
from tests import stage_bars as sb

FLIP_MARGIN = 1e-5
MAX_FLIPS = 2
H = 128

GruCase = collections.namedtuple('GruCase', 'id B T h0 regime')          # regime: typical | saturated | impulse_fw | impulse_bw
HwCase = collections.namedtuple('HwCase', 'id M nl B T gates')           # B, T: the adapter form (M = B * T), else None; gates: typical | saturated
PnCase = collections.namedtuple('PnCase', 'id M masks')

GRU_SHAPES = ((1, 1), (2, 7), (2, 8), (3, 9), (2, 16), (3, 17), (5, 41), (64, 3), (65, 3))
GRU_CASES = [GruCase('%s-B%d-T%d-%s' % (rg[:3], B, T, 'h0' if h0 else 'zero'), B, T, h0, rg)
             for rg in ('typical', 'saturated') for (B, T) in GRU_SHAPES for h0 in (False, True)]
IMPULSE_AT = (1, 8)     # (b0, t0) of the impulse cases: the middle one of three rows; step 8 from either end, the first of the second chunk
GRU_CASES += [GruCase('impulse-fw', 3, 17, True, 'impulse_fw'), GruCase('impulse-bw', 3, 17, True, 'impulse_bw')]

HW_CASES = [HwCase('plain-M%d' % M, M, 4, None, None, 'typical') for M in (1, 31, 32, 33, 64, 95)]
HW_CASES += [HwCase('plain-M33-nl%d' % nl, 33, nl, None, None, 'typical') for nl in (1, 2, 3)]
HW_CASES += [HwCase('plain-M33-gates30', 33, 4, None, None, 'saturated')]
HW_CASES += [HwCase('adapter-B%d-T%d' % (B, T), B * T, 4, B, T, 'typical') for (B, T) in ((7, 5), (1, 33), (3, 32))]

# (M = 32 is not in the issue's list: it is here because the pre-net shares the 32-row tile and the list has no full last tile)
PN_CASES = [PnCase('M%d-%s' % (M, 'masks' if k else 'nomask'), M, k) for M in (1, 31, 32, 33, 65) for k in (False, True)]

# one chained case per backward kernel (bigru_bwd; highway_bwd plain and adapter; mlp2 backward), one streamed case per door
CHAINED = {'gru': ('typ-B3-T17-h0', 'sat-B3-T9-h0'), 'highway': ('plain-M95', 'adapter-B7-T5'), 'prenet': ('M65-masks',)}
STREAMED = {'gru': 'typ-B3-T9-h0', 'highway': 'adapter-B7-T5', 'prenet': 'M33-masks'}

# The edges named in the issue ("Why"), as predicates over the case lists: tests/test_cbhg_tail_host.py asserts each is reached.
EDGES = {
    'gru: a single step': lambda: any(c.T == 1 for c in GRU_CASES),
    'gru: one partial DMA chunk (T < 8)': lambda: any(1 < c.T < 8 for c in GRU_CASES),
    'gru: exactly one chunk (T == 8: (c + 1) * CH < T is false at the i == CH - 1 wait)': lambda: any(c.T == 8 for c in GRU_CASES),
    'gru: one step into the second chunk (T == 9)': lambda: any(c.T == 9 for c in GRU_CASES),
    'gru: exactly two chunks (T == 16)': lambda: any(c.T == 16 for c in GRU_CASES),
    'gru: third chunk reuses buffer 0, one step (T == 17)': lambda: any(c.T == 17 for c in GRU_CASES),
    'gru: many chunks and a partial last one': lambda: any(c.T > 32 and c.T % 8 for c in GRU_CASES),
    'gru: 2 B <= 128 (padded LDS request)': lambda: any(2 * c.B == 128 for c in GRU_CASES),
    'gru: 2 B > 128 (no padding)': lambda: any(2 * c.B == 130 for c in GRU_CASES),
    'gru: every shape with and without h0, in both regimes': lambda: all(
        any((c.B, c.T, c.h0, c.regime) == (B, T, h0, rg) for c in GRU_CASES)
        for (B, T) in GRU_SHAPES for h0 in (False, True) for rg in ('typical', 'saturated')),
    'gru: an impulse per direction across a chunk boundary, with h0': lambda: all(
        any(c.regime == rg and c.T > 16 and c.B > 2 and c.h0 for c in GRU_CASES) for rg in ('impulse_fw', 'impulse_bw')),
    'highway: M < 32': lambda: any(c.M < 32 and c.B is None for c in HW_CASES),
    'highway: M % 32 == 1, 31 and 0 over more than one block': lambda: all(
        any(c.M > 32 and c.M % 32 == k and c.B is None and c.nl == 4 for c in HW_CASES) for k in (1, 31, 0)),
    'highway: nl = 1, 2, 3, 4 on a partial tile': lambda: all(any(c.nl == nl and c.M % 32 for c in HW_CASES) for nl in (1, 2, 3, 4)),
    'highway: gate biases of +-30': lambda: any(c.gates == 'saturated' for c in HW_CASES),
    'highway adapter: a tile straddles two sequences': lambda: any(c.B and c.B > 1 and c.T % 32 and c.T < 32 for c in HW_CASES),
    'highway adapter: one sequence, partial last tile': lambda: any(c.B == 1 and c.T % 32 for c in HW_CASES),
    'highway adapter: sequences aligned with the tiles': lambda: any(c.B and c.B > 1 and c.T % 32 == 0 for c in HW_CASES),
    'prenet: M < 32, M % 32 == 1 / 31 / 0, three blocks': lambda: (
        {c.M for c in PN_CASES} >= {1, 31, 32, 33, 65}),
    'prenet: every shape with and without the keep masks': lambda: all(
        any(c.M == M and c.masks == k for c in PN_CASES) for M in (1, 31, 32, 33, 65) for k in (False, True)),
    'chained and streamed cases exist': lambda: all(
        n in {c.id for c in cs} for kind, cs in (('gru', GRU_CASES), ('highway', HW_CASES), ('prenet', PN_CASES))
        for n in CHAINED[kind] + (STREAMED[kind],)),
}


def case_by_id(cases, cid):
    return next(c for c in cases if c.id == cid)


def seed_of(kind, cid):
    return zlib.crc32(('%s/%s' % (kind, cid)).encode())


# ---------------------------------------------------------------------------------------------------------------- operands
@functools.lru_cache(maxsize=None)
def gru_operands(c):
    """fp32 operands of a bi-GRU case.  typical: xg ~ N(0, 1), weights U(+-0.15) as in test_bigru_fwd.  saturated: a third of
    the units (j % 3 == 0) get r, u and c pre-activations of magnitude U(40, 200) with random signs; the h side adds at most
    128 * 0.15 = 19.2, so the sign holds and |pre| >= 20.8: exp overflows for the larger ones, and every such gate rounds to
    exactly 0, 1 or -1 in fp32 except sigmoid of the negative ones (4e-18 .. 1e-9, representable)."""
    rng = np.random.default_rng(seed_of('gru', c.id))
    f = np.float32
    w = {}
    for d in ref.DIRS:
        wg, wc = rng.uniform(-0.15, 0.15, (256, 256)), rng.uniform(-0.15, 0.15, (256, 128))
        wg[:H], wc[:H] = 0.0, 0.0          # the x side: not an operand of the recurrence (the GPU test hands the kernel NaN there)
        w[d + '/gates/kernel'], w[d + '/candidate/kernel'] = wg.astype(f), wc.astype(f)
    xg = rng.standard_normal((c.B, c.T, 768))
    if c.regime == 'saturated':
        big = rng.uniform(40.0, 200.0, xg.shape) * rng.choice([-1.0, 1.0], xg.shape)
        unit = (np.arange(768) % H) % 3 == 0
        xg[:, :, unit] = big[:, :, unit]
    h0 = rng.uniform(-0.9, 0.9, (c.B, H)).astype(f) if c.h0 else None
    dout = rng.standard_normal((c.B, c.T, 256))
    if c.regime.startswith('impulse'):
        d = 0 if c.regime == 'impulse_fw' else 1
        keep = np.zeros_like(dout)
        b0, t0 = IMPULSE_AT
        keep[b0, t0, H * d:H * (d + 1)] = 1.0
        dout = dout * keep
    return {'xg': xg.astype(f), 'w': w, 'wT': ref.bigru_transposes(w), 'h0': h0, 'dout': dout.astype(f)}


@functools.lru_cache(maxsize=None)
def hw_operands(c):
    """fp32 operands of a highway case: x ~ N(0, 1), kernels N(0, 1 / 128), bt = -1 +- 0.3 (the reference's gate bias), bh +- 0.3;
    saturated: bt = +-30 by column.  Adapter form: wa N(0, 1 / 128), rowb ~ N(0, 0.25) per sequence."""
    rng = np.random.default_rng(seed_of('highway', c.id))
    f = np.float32
    p = {k: [] for k in ('wt', 'bt', 'wh', 'bh')}
    for l in range(c.nl):
        p['wt'].append((rng.standard_normal((H, H)) / np.sqrt(H)).astype(f))
        p['wh'].append((rng.standard_normal((H, H)) / np.sqrt(H)).astype(f))
        bt = -1.0 + rng.uniform(-0.3, 0.3, H)
        if c.gates == 'saturated':
            bt = 30.0 * rng.choice([-1.0, 1.0], H)
        p['bt'].append(bt.astype(f))
        p['bh'].append(rng.uniform(-0.3, 0.3, H).astype(f))
    if c.B is not None:
        p['wa'] = [(rng.standard_normal((H, H)) / np.sqrt(H)).astype(f) for _ in range(c.nl)]
        p['rowb'] = [(0.5 * rng.standard_normal((c.B, H))).astype(f) for _ in range(c.nl)]
    x = rng.standard_normal((c.M, H)).astype(f)
    g = rng.standard_normal((c.M, H)).astype(f)
    wT = [np.ascontiguousarray(np.concatenate([p['wt'][l].T, p['wh'][l].T], 0)) for l in range(c.nl)]
    waT = [np.ascontiguousarray(w.T) for w in p['wa']] if c.B is not None else None
    return {'x': x, 'p': p, 'g': g, 'wT': wT, 'waT': waT}


@functools.lru_cache(maxsize=None)
def pn_operands(c):
    rng = np.random.default_rng(seed_of('prenet', c.id))
    f = np.float32
    p = {'w1': (rng.standard_normal((256, 256)) / 16.0).astype(f), 'b1': rng.uniform(-0.3, 0.3, 256).astype(f),
         'w2': (rng.standard_normal((256, 128)) / 16.0).astype(f), 'b2': rng.uniform(-0.3, 0.3, 128).astype(f)}
    x = rng.standard_normal((c.M, 256)).astype(f)
    dy2 = rng.standard_normal((c.M, 128)).astype(f)
    k1 = rng.integers(0, 2, (c.M, 256)).astype(np.uint8) if c.masks else None
    k2 = rng.integers(0, 2, (c.M, 128)).astype(np.uint8) if c.masks else None
    return {'x': x, 'p': p, 'dy2': dy2, 'k1': k1, 'k2': k2, 'w2T': np.ascontiguousarray(p['w2'].T), 'w1T': np.ascontiguousarray(p['w1'].T)}


# ---------------------------------------------------------------------------------------------------------------- references
@functools.lru_cache(maxsize=None)
def gru_reference(c):
    o = gru_operands(c)
    return ref.bigru_oracle(o['xg'], o['w'], o['h0'], o['dout'])


@functools.lru_cache(maxsize=None)
def hw_reference(c):
    o = hw_operands(c)
    return ref.highway_oracle(o['x'], o['p'], c.nl, c.T, o['g'])


@functools.lru_cache(maxsize=None)
def pn_reference(c):
    o = pn_operands(c)
    return ref.prenet_oracle(o['x'], o['p'], o['k1'], o['k2'], o['dy2'])


# ---------------------------------------------------------------------------------------------------------------- judging
class Report:
    """stats: [(kernel, compare() dict)]; fails: the bars, exact-zero checks and flip conditions missed; flips: [(site, index, margin)]"""

    def __init__(self, cid):
        self.id, self.stats, self.fails, self.flips = cid, [], [], []

    def judge(self, kernel, name, got, want, lead):
        got = np.asarray(got)
        name = '%s %s' % (self.id, name)
        if got.shape != np.asarray(want).shape:
            self.fails.append('%s: shape %s, the reference has %s' % (name, got.shape, np.asarray(want).shape))
            return
        if not np.isfinite(got).all():
            self.fails.append('%s: %d non-finite elements, first at %s' % (name, int((~np.isfinite(got)).sum()),
                                                                          tuple(int(k) for k in np.argwhere(~np.isfinite(got))[0])))
            return
        if not np.any(want):    # (r * h_prev of a single step from a zero state, ..): no norm to compare with, and zero exactly
            self.zero(name + ' (the reference is all zeros)', got, True)
            return
        st = sb.compare(name, got, want, lead)
        self.stats.append((kernel, st))
        self.fails += sb.failures(st, *sb.CBHG_TAIL_BARS[kernel])

    def zero(self, name, got, mask):
        self.fails += sb.exact_zero_failures('%s %s' % (self.id, name), got, mask)

    def worst(self, kernel):
        """(worst tensor rel-L2, worst row) over this report's outputs of one kernel"""
        st = [s for k, s in self.stats if k == kernel]
        return (max(s['rel'] for s in st), max(s['row'] for s in st)) if st else (0.0, 0.0)

    def take_flips(self, hip, ok, dec):
        fl = dn.flips(hip, ok, dec)
        self.flips += fl
        for site, idx, margin in fl:
            if not margin <= FLIP_MARGIN:
                self.fails.append('%s: decision %s%s differs from fp64 with a margin of %.3e > %.0e' % (self.id, site, idx, margin, FLIP_MARGIN))
        if len(fl) > MAX_FLIPS:
            self.fails.append('%s: %d ReLU decisions differ from fp64, at most %d may' % (self.id, len(fl), MAX_FLIPS))
        return fl


def _f32(a):
    return None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def _gru_bwd_checks(rep, c, tag, got, want, stash_ruc, with_dh0):
    dxg, rh, dh0 = got
    B, T = c.B, c.T
    impulse = c.regime.startswith('impulse')
    rep.judge('bigru_bwd', tag + ' dxg', dxg, want['dxg'], (B, T))
    rep.judge('bigru_bwd', tag + ' rh', rh, want['rh'], (B, T))
    if with_dh0:
        if not impulse:
            rep.judge('bigru_bwd', tag + ' dh0', dh0, want['dh0'], (2, B))
        elif np.isfinite(np.asarray(dh0)).all():
            d = 0 if c.regime == 'impulse_fw' else 1
            rep.judge('bigru_bwd', tag + ' dh0[%d]' % d, dh0[d], want['dh0'][d], (B,))
        else:
            rep.fails.append('%s %s dh0: non-finite' % (c.id, tag))
    if not np.isfinite(np.asarray(dxg)).all():
        return
    # u (1 - u), r (1 - r) and 1 - c^2 are exactly zero where the fp32 gate the kernel was fed is exactly 0 or 1 (c: -1 or 1)
    s = np.asarray(stash_ruc, dtype=np.float32).reshape(B, T, 2, 3, H)
    x = np.asarray(dxg).reshape(B, T, 2, 3, H)
    rep.zero(tag + ' dxg[r] where r is 0 or 1', x[:, :, :, 0], (s[:, :, :, 0] == 0) | (s[:, :, :, 0] == 1))
    rep.zero(tag + ' dxg[u] where u is 0 or 1', x[:, :, :, 1], (s[:, :, :, 1] == 0) | (s[:, :, :, 1] == 1))
    rep.zero(tag + ' dxg[c] where c is -1 or 1', x[:, :, :, 2], np.abs(s[:, :, :, 2]) == 1)
    if impulse:
        d = 0 if c.regime == 'impulse_fw' else 1
        b0, t0 = IMPULSE_AT
        quiet = np.ones((B, T, 2), dtype=bool)             # True: no gradient can reach (b, t, direction)
        quiet[b0, :t0 + 1, 0] = d != 0
        quiet[b0, t0:, 1] = d != 1
        rep.zero(tag + ' dxg outside the impulse row and its past', x, quiet[:, :, :, None, None])
        if with_dh0:
            q0 = np.ones((2, B), dtype=bool)
            q0[d, b0] = False
            rep.zero(tag + ' dh0 of the other rows and the other direction', dh0, q0[:, :, None])


def run_gru(c, be, chained=False):
    o, want = gru_operands(c), gru_reference(c)
    rep = Report(c.id)
    out, ruc = be.bigru_fwd(o['xg'], o['w'], o['h0'])
    rep.judge('bigru_fwd', 'out', out, want['out'], (c.B, c.T))
    rep.judge('bigru_fwd', 'ruc', ruc, want['ruc'], (c.B, c.T))
    for with_dh0 in ((True, False) if c.id == STREAMED['gru'] else (True,)):       # dh0 == NULL once
        fed = (_f32(want['out']), _f32(want['ruc']))
        got = be.bigru_bwd(o['dout'], fed[0], fed[1], o['wT'], o['h0'], want_dh0=with_dh0)
        _gru_bwd_checks(rep, c, 'isolated' if with_dh0 else 'isolated, no dh0', got, want, fed[1], with_dh0)
    if chained and np.isfinite(out).all() and np.isfinite(ruc).all():
        got = be.bigru_bwd(o['dout'], out, ruc, o['wT'], o['h0'], want_dh0=True)
        _gru_bwd_checks(rep, c, 'chained', got, want, ruc, True)
    return rep


def _hw_fwd_checks(rep, c, got, want):
    for l in range(c.nl):
        rep.judge('highway_fwd', 'y[%d]' % l, got['y'][l], want['y'][l], (c.M,))
        rep.judge('highway_fwd', 'th[%d]' % l, got['th'][l], want['th'][l], (c.M,))
        if c.B is not None:
            rep.judge('highway_fwd', 'hx[%d]' % l, got['hx'][l], want['hx'][l], (c.M,))


def _hw_bwd_checks(rep, c, tag, got, want, stash_th):
    for l in range(c.nl):
        rep.judge('highway_bwd', '%s dth[%d]' % (tag, l), got['dth'][l], want['dth'][l], (c.M,))
        if c.B is not None:
            rep.judge('highway_bwd', '%s dhx[%d]' % (tag, l), got['dhx'][l], want['dhx'][l], (c.M,))
        if np.isfinite(np.asarray(got['dth'][l])).all():
            s = np.asarray(stash_th[l], dtype=np.float32)
            # dT = g (H - x) T (1 - T) is exactly zero where the fp32 gate is exactly 0 or 1; dH where the stashed H is not positive
            rep.zero('%s dT[%d] where T is 0 or 1' % (tag, l), np.asarray(got['dth'][l])[:, :H], (s[:, :H] == 0) | (s[:, :H] == 1))
            rep.zero('%s dH[%d] where H <= 0' % (tag, l), np.asarray(got['dth'][l])[:, H:], ~(s[:, H:] > 0))
    rep.judge('highway_bwd', '%s gout' % tag, got['gout'], want['gout'], (c.M,))


def run_highway(c, be, chained=False):
    o, want = hw_operands(c), hw_reference(c)
    rep = Report(c.id)
    got = be.highway_fwd(o['x'], o['p'], c.nl, c.T)
    finite = all(np.isfinite(np.asarray(a)).all() for a in got['th'] + got['y'] + (got['hx'] or []))
    fl = rep.take_flips(ref.highway_decisions(got['th']), {}, want['dec']) if finite else []
    forced = want
    if fl:      # the fp64 graph with the backend's decisions imposed
        forced = ref.highway_oracle(o['x'], o['p'], c.nl, c.T, o['g'], force=[s[:, H:] > 0 for s in got['th']])
    _hw_fwd_checks(rep, c, got, forced)
    if c.gates == 'saturated' and finite:
        for l in range(c.nl):
            up = o['p']['bt'][l] > 0
            t = np.asarray(got['th'][l])[:, :H]
            # |x Wt| stays below 30 - 17 (x Wt ~ N(0, 1) by construction), so 1 + exp(-(x Wt + 30)) rounds to 1 in fp32: T is exactly 1.
            # sigmoid(-30 + ..) ~ 9e-14 is an ordinary fp32 number, NOT zero: there the bars apply and T must stay below 2^-20
            if not (t[:, up] == 1).all():
                rep.fails.append('%s: T[%d] is not exactly 1 under a gate bias of +30' % (c.id, l))
            if not (t[:, ~up] < 2.0 ** -20).all():
                rep.fails.append('%s: T[%d] is not below 2^-20 under a gate bias of -30' % (c.id, l))
    x_of = lambda r: [_f32(a) for a in (r['hx'] if c.B is not None else [o['x']] + list(r['y'][:c.nl - 1]))]
    fed_th = [_f32(a) for a in want['th']]
    _hw_bwd_checks(rep, c, 'isolated', be.highway_bwd(o['g'], o['wT'], fed_th, x_of(want), o['waT']), want, fed_th)
    if chained and finite:
        _hw_bwd_checks(rep, c, 'chained', be.highway_bwd(o['g'], o['wT'], got['th'], x_of(got), o['waT']), forced, got['th'])
    return rep


def _pn_bwd_checks(rep, c, tag, got, want, y1, y2, k1, k2):
    dz2, dz1, dx = got
    rep.judge('prenet_bwd', tag + ' dz2', dz2, want['dz2'], (c.M,))
    rep.judge('prenet_bwd', tag + ' dz1', dz1, want['dz1'], (c.M,))
    rep.judge('prenet_bwd', tag + ' dx', dx, want['dx'], (c.M,))
    if np.isfinite(np.asarray(dz2)).all() and np.isfinite(np.asarray(dz1)).all():
        off2 = ~(np.asarray(y2) > 0) | (False if k2 is None else k2 == 0)
        off1 = ~(np.asarray(y1) > 0) | (False if k1 is None else k1 == 0)
        rep.zero(tag + ' dz2 where the unit was dropped or its ReLU is off', dz2, off2)
        rep.zero(tag + ' dz1 where the unit was dropped or its ReLU is off', dz1, off1)


def run_prenet(c, be, chained=False):
    o, want = pn_operands(c), pn_reference(c)
    rep = Report(c.id)
    y1, y2 = be.prenet_fwd(o['x'], o['p'], o['k1'], o['k2'])
    finite = np.isfinite(np.asarray(y1)).all() and np.isfinite(np.asarray(y2)).all()
    forced = want
    if finite:
        d, ok = ref.prenet_decisions(y1, y2, o['k1'], o['k2'])
        if rep.take_flips(d, ok, want['dec']):
            forced = ref.prenet_oracle(o['x'], o['p'], o['k1'], o['k2'], o['dy2'], force=d)
    rep.judge('prenet_fwd', 'y1', y1, forced['y1'], (c.M,))
    rep.judge('prenet_fwd', 'y2', y2, forced['y2'], (c.M,))
    f1, f2 = _f32(want['y1']), _f32(want['y2'])
    _pn_bwd_checks(rep, c, 'isolated', be.prenet_bwd(o['dy2'], o['w2T'], o['w1T'], f1, f2, o['k1'], o['k2']), want, f1, f2, o['k1'], o['k2'])
    if chained and finite:
        _pn_bwd_checks(rep, c, 'chained', be.prenet_bwd(o['dy2'], o['w2T'], o['w1T'], y1, y2, o['k1'], o['k2']), forced, y1, y2, o['k1'], o['k2'])
    return rep


KINDS = {'gru': (GRU_CASES, run_gru), 'highway': (HW_CASES, run_highway), 'prenet': (PN_CASES, run_prenet)}
KERNELS = ('bigru_fwd', 'bigru_bwd', 'highway_fwd', 'highway_bwd', 'prenet_fwd', 'prenet_bwd')
