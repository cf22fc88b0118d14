"""Host (no GPU): the references, the restated contracts and the case lists of tests/gemm_forms.py.  The case lists must reach
every new label of PATH_TABLE and put a sequence end or start on every seam of the pooled epilogues' overlapping tiles; the
references are held against independent restatements (autograd of max(z[m], z[m+1]), the transposed convolutions, torch's
conv1d gradient); deliberate defects put into the restatements must be caught by the cases; and the wrappers of the debug doors
refuse bad arguments by name before the library is called."""
import numpy as np
import pytest
import torch

from tests import gemm_forms as gf
from tests import gemm_paths as gp


def test_case_lists_reach_every_form_label():
    got = gf.form_labels()
    assert set(got) == set(gf.FORM_LABELS) and set(gf.FORM_LABELS) <= set(gp.PATH_TABLE)
    ids = [i for v in got.values() for i in v if not i.startswith('pf-') and not i.startswith('pb-')]
    ids += [c.id for c in gf.POOL_FWD_CASES + gf.POOL_BWD_CASES]
    assert len(ids) == len(set(ids)), 'duplicate case ids'


def test_restated_m_tiles_and_tile_rows():
    assert [gf.m_tiles(M, True) for M in (1, 2, 127, 128, 129, 254, 255, 256, 260)] == [1, 1, 1, 1, 2, 2, 2, 3, 3]
    assert [gf.m_tiles(M, False) for M in (1, 128, 129, 256, 257)] == [1, 1, 2, 2, 3]
    for M in (1, 127, 128, 129, 255, 256, 260):
        tiles = gf.tile_rows(M, True)
        owned = [m for tmm, m0, rows in tiles for m in rows if m - m0 >= 1 or tmm == 0]            # pool == 2: rows 1..127 (tile 0 also row 0)
        written = [m for tmm, m0, rows in tiles for m in rows if m - m0 < 127 or m == M - 1]        # pool == 1: the halo row is the next tile's
        assert owned == list(range(M)) and sorted(written) == list(range(M)), M


@pytest.mark.parametrize('cases', (gf.POOL_FWD_CASES, gf.POOL_BWD_CASES), ids=('fwd', 'bwd'))
def test_pool_cases_place_sequences_on_every_seam(cases):
    """from the restated tiling: a sequence ending on local row 0, 31, 32, 63, 126 and 127, one starting on local row 0 and on local
    row 1 of a tile with tmm > 0, M - 1 a multiple of 127 and not, T = 1; 1, 2 and 3 m-tiles; T from the issue's list"""
    p = gf.seam_placements(cases)
    assert p['ends'] >= {0, 31, 32, 63, 126, 127}, sorted(p['ends'])
    assert p['starts'] >= {0, 1}, sorted(p['starts'])
    assert p['mult'] and p['nomult'] and p['t1']
    assert {gf.m_tiles(c.M, True) for c in cases} == {1, 2, 3}
    assert {c.T for c in cases} >= {1, 2, 5, 126, 127, 128, 129}
    assert {c.M for c in cases} >= {127, 128, 129, 254, 255, 256, 260}
    # the same placements by rows with T > 2, where the pooled value really depends on its successor and a sequence is longer than a lane group
    long_ = gf.seam_placements([c for c in cases if c.T > 2])
    assert long_['ends'] >= {0, 126, 127} and long_['starts'] >= {0, 1}
    for c in cases:
        assert c.M % c.T == 0 and c.N % 4 == 0 and c.K % 32 == 0, c.id


def test_pool_cases_cover_columns_and_arguments():
    f, b = gf.POOL_FWD_CASES, gf.POOL_BWD_CASES
    for rows in (f, b):
        assert {c.N for c in rows} == {128, 132, 4} and {c.cpad for c in rows} == {0, 4} and {c.K for c in rows} == {32, 64}
        assert {c.smul for c in rows} == {'1', 'rs'} and {c.bx for c in rows} == {'0', '1'} and {c.apad for c in rows} == {0, 4}
    assert {c.F for c in f} == {1, 3} and {c.pre for c in f} == {True, False}
    # a partly filled second n-tile (132) and a tile whose lanes are mostly col_ok-false (4), each with and without pitch padding
    assert {(c.N, c.cpad) for c in f} >= {(132, 0), (132, 4), (4, 0), (4, 4), (128, 0), (128, 4)}
    assert {c.data for c in b} == {'margin', 'grid'} and all(c.smul == '1' for c in b if c.data == 'grid')
    assert gf.POOL_BWD_TAPS == 3 and gf.POOL_BWD_PAD == 1
    # the bitwise two-pass twin runs in every seam case, with a gamma whose product with the twin's own 1 / sqrt(1 + eps) is the fused
    # launch's factor to the bit
    assert gf.form_labels()['ew.bnpool.fwd'] == [c.id for c in f]
    for c in f:
        o, rs = gf.pool_fwd_operands(c), np.float32(gf.RS)
        fused = (o['scale'] * np.float32(gf.scale_mul_of(c))).astype(np.float32)
        assert fused.dtype == np.float32 and np.array_equal(fused, (o['gamma'] * rs).astype(np.float32)), c.id
    # the B-image form of the bf16x3 kernel (how the model runs these launches): some cases of each list
    for rows in (f, b, gf.GATHER_CASES):
        assert any(c.img for c in rows) and all(c.bx == '1' for c in rows if c.img) and any(not c.img and c.bx == '1' for c in rows)
    assert any(c.img and c.data == 'grid' for c in b) and {c.N for c in f if c.img} == {128, 132, 4}


def _autograd_pool(x, scale, shift, scale_mul, dy, T):
    """brute force: pooled = max(z[m], z[m+1]) inside a sequence through torch autograd, in fp64"""
    M, N = x.shape
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    g = torch.tensor(np.asarray(scale, np.float64), requires_grad=True)
    b = torch.tensor(np.asarray(shift, np.float64), requires_grad=True)
    z = (xt * (g * scale_mul) + b).view(M // T, T, N)
    pooled = torch.cat([torch.maximum(z[:, :-1], z[:, 1:]), z[:, -1:]], 1) if T > 1 else z
    (pooled.reshape(M, N) * torch.tensor(dy)).sum().backward()
    return xt.grad.numpy(), g.grad.numpy(), b.grad.numpy()


@pytest.mark.parametrize('c', [c for c in gf.POOL_BWD_CASES if c.data == 'margin'], ids=lambda c: c.id)
def test_pool_bwd_ref_is_the_gradient_of_the_pooled_affine(c):
    """margin cases only (ties are defined by the rule, not by a derivative).  dx of the reference goes through the ReLU that
    produced x: the autograd's d/dx is masked with x > 0 here."""
    o = gf.margin_pool_operands(c.id, c.M, c.T, c.N, c.K, gf.POOL_BWD_TAPS)
    sm = gf.scale_mul_of(c)
    assert gf.decision_margin(o['x'], o['scale'], o['shift'], sm, c.T) >= 1e-3
    r = gf.pool_bwd_ref(o['A'], o['W'], o['x'], o['scale'], o['shift'], sm, c.T, gf.POOL_BWD_PAD)
    dx, dg, db = _autograd_pool(o['x'].astype(np.float64), o['scale'], o['shift'], sm, r['dy'], c.T)
    assert np.allclose(r['dx'], dx * (o['x'] > 0), rtol=1e-12, atol=1e-12)
    assert np.allclose(r['dgamma'], dg, rtol=1e-11, atol=1e-11) and np.allclose(r['dbeta'], db, rtol=1e-11, atol=1e-11)
    assert ((o['x'] == 0).mean() > 0.2) and (r['dx'][o['x'] == 0] == 0).all() and (r['S_dx'][o['x'] == 0] == 0).all()


@pytest.mark.parametrize('c', [c for c in gf.POOL_BWD_CASES if c.data == 'grid'], ids=lambda c: c.id)
def test_grid_case_is_exact_in_fp32_and_holds_every_tie_situation(c):
    o = gf.grid_pool_operands(c.id, c.M, c.T, c.N, c.K, gf.POOL_BWD_TAPS)
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    for k in ('x', 'scale', 'shift', 'A', 'W'):
        assert np.array_equal(f32(o[k]), o[k]), k
    r = gf.pool_bwd_ref(o['A'], o['W'], o['x'], o['scale'], o['shift'], 1.0, c.T, gf.POOL_BWD_PAD)
    z = o['x'] * o['scale'] + o['shift']
    for k, v in (('z', z), ('dy', r['dy']), ('dz', r['dz']), ('dx', r['dx'])):
        assert np.array_equal(f32(v), v), k                        # what the kernel forms is exact: compare bitwise
    # every partial sum of dy is exact too, whatever the order: multiples of 2^-5 below 2^7
    assert np.abs(o['A']).max() <= 1 and np.abs(o['W']).max() <= 0.5 and gf.POOL_BWD_TAPS * c.K * 0.5 < 2 ** 7
    assert np.array_equal(np.round(r['dy'] * 32), r['dy'] * 32)
    nxt = gf._has_next(c.M, c.T)
    ties = (z[nxt] == z[1:][nxt[:-1]])
    assert 0.2 < ties.mean() < 0.9 and (o['x'] == 0).mean() > 0.4
    assert set(np.unique(o['scale'])) == {-1, -0.5, 0, 0.5, 1, 2}
    zero_scale, neg = o['scale'] == 0, o['scale'] < 0
    assert ties[:, zero_scale[:ties.shape[1]]].all() and neg.any()
    # columns whose x is all zero: dx exactly 0, dbeta still receives every dy
    assert (o['x'][:, 6:8] == 0).all() and (r['dx'][:, 6:8] == 0).all() and np.array_equal(r['dbeta'][6:8], r['dy'][:, 6:8].sum(0))
    assert np.abs(r['dbeta'][6:8]).min() > 0
    # the rule decides: with >= and > swapped the result differs (mutation 1), and owning local row 0 twice would double-count
    dz_swapped = _route_variant(z, r['dy'], c.T, swap=True)
    assert not np.array_equal(dz_swapped, r['dz'])
    g = gf.gamma_for_scale(o['scale'])
    assert np.array_equal((g * np.float32(gf.RS)).astype(np.float64), o['scale'])


def _route_variant(z, dy, T, swap=False):
    M = z.shape[0]
    t = np.arange(M) % T
    first, last = (t == 0)[:, None], (t == T - 1)[:, None]
    zn, zp, dyp = np.roll(z, -1, 0), np.roll(z, 1, 0), np.roll(dy, 1, 0)
    ge = last | ((z > zn) if swap else (z >= zn))
    gt = ~first & ((z >= zp) if swap else (z > zp))
    return ge * dy + gt * dyp


def test_mutations_of_the_pool_rules_are_caught_by_the_references():
    """mutations 1 (>= -> >) and 2 (`lr >= 1` -> `lr >= 0` in `own`) of the issue against the Python restatements: a kernel with
    either defect produces what is computed here, and the cases tell it from the reference by more than the bound"""
    c = next(c for c in gf.POOL_BWD_CASES if c.id == 'pb-tie-254x127')
    o = gf.grid_pool_operands(c.id, c.M, c.T, c.N, c.K, gf.POOL_BWD_TAPS)
    r = gf.pool_bwd_ref(o['A'], o['W'], o['x'], o['scale'], o['shift'], 1.0, c.T, gf.POOL_BWD_PAD)
    z = o['x'] * o['scale'] + o['shift']
    # 1: `z >= zn` -> `z > zn` alone: a tie routes dy[m] nowhere
    M = c.M
    t = np.arange(M) % c.T
    first, last = (t == 0)[:, None], (t == c.T - 1)[:, None]
    ge1 = last | (z > np.roll(z, -1, 0))
    gt = ~first & (z > np.roll(z, 1, 0))
    dz1 = ge1 * r['dy'] + gt * np.roll(r['dy'], 1, 0)
    dx1 = (o['x'] > 0) * dz1 * o['scale']
    bound = gp.element_bound(r['n_dx'], r['S_dx'], r['g_dx'], r['dx'])
    assert (np.abs(dx1 - r['dx']) > bound).any() and not np.allclose(dz1.sum(0), r['dy'].sum(0))
    # 2: every tile owns its local row 0 as well: the rows m0 = 127 tmm, tmm > 0, are written twice (same value) and SUMMED twice
    twice = [m0 for tmm, m0, rows in gf.tile_rows(M, True) if tmm > 0]
    assert twice == [127]
    db2 = r['dbeta'] + r['dz'][twice].sum(0)
    bb = gp.element_bound(r['n_col'], r['S_b'], 1.0, r['dbeta'])
    assert (np.abs(db2 - r['dbeta']) > bb).any()
    # ... and so in every case with more than one tile, on its own data and with its own bound (dbeta holds no prior content here)
    for cc in gf.POOL_BWD_CASES:
        twice = [m0 for tmm, m0, rows in gf.tile_rows(cc.M, True) if tmm > 0]
        assert len(twice) == gf.m_tiles(cc.M, True) - 1 and all(0 < m < cc.M for m in twice), cc.id
        if not twice:
            continue
        oc = (gf.grid_pool_operands if cc.data == 'grid' else gf.margin_pool_operands)(cc.id, cc.M, cc.T, cc.N, cc.K, gf.POOL_BWD_TAPS)
        rc = gf.pool_bwd_ref(oc['A'], oc['W'], oc['x'], oc['scale'], oc['shift'], gf.scale_mul_of(cc), cc.T, gf.POOL_BWD_PAD)
        assert (np.abs(rc['dz'][twice].sum(0)) > gp.element_bound(rc['n_col'], rc['S_b'], 1.0, rc['dbeta'])).any(), cc.id


def test_the_two_bank_gather_restatements_agree_and_are_the_conv_banks_gradient():
    for c in gf.GATHER_CASES:
        rng = np.random.default_rng(gp.seed_of(c.id))
        M = c.B * c.T
        dbank = rng.standard_normal((M, c.F * c.K))
        WTs = [rng.standard_normal((f, c.K, c.N)) for f in range(1, c.F + 1)]
        res, prior = rng.standard_normal((M, c.N)), rng.standard_normal((M, c.N))
        a, S, n = gf.gather_ref(dbank, WTs, c.T, res, prior)
        b = gf.gather_ref_convs(dbank, WTs, c.T, res, prior)
        assert np.allclose(a, b, rtol=1e-12, atol=1e-12) and n == c.F * (c.F + 1) // 2 * c.K and (S >= np.abs(a) - 1e-9).all(), c.id
    # ... and, for the transposed kernels WT_f[j] = W_f[f - 1 - j]^T, the gradient of the forward bank (pad_l = (f - 1) / 2) w.r.t. its input
    rng = np.random.default_rng(3)
    B, T, cin, cb, F = 3, 5, 6, 4, 4
    x = torch.tensor(rng.standard_normal((B, cin, T)), requires_grad=True)
    Ws = [rng.standard_normal((f, cin, cb)) for f in range(1, F + 1)]                       # forward kernels (taps, K = cin, N = cb)
    dbank = rng.standard_normal((B * T, F * cb))
    loss = 0
    for f in range(1, F + 1):
        pad_l = (f - 1) // 2
        y = torch.nn.functional.conv1d(torch.nn.functional.pad(x, (pad_l, f - 1 - pad_l)), torch.tensor(Ws[f - 1]).permute(2, 1, 0).contiguous())
        loss = loss + (y.transpose(1, 2).reshape(B * T, cb) * torch.tensor(dbank[:, (f - 1) * cb:f * cb])).sum()
    loss.backward()
    want = x.grad.transpose(1, 2).reshape(B * T, cin).numpy()
    WTs = [np.stack([Ws[f - 1][f - 1 - j].T for j in range(f)]) for f in range(1, F + 1)]  # (f, K = cb, N = cin)
    assert np.allclose(gf.gather_ref(dbank, WTs, T)[0], want, rtol=1e-12, atol=1e-12)


def test_gather_cases_cut_and_shift_where_the_issue_asks():
    mid_filter = mid_tap = undivided = False
    for c in gf.GATHER_CASES:
        nit, per, chunks = gf.gather_chunks(c.F, c.K, c.S)
        kt = c.K // 32
        assert chunks[0][0] == 0 and chunks[-1][1] == nit and all(a[1] == b[0] for a, b in zip(chunks, chunks[1:])) and len(chunks) in (2, 3), c.id
        for lo, _ in chunks[1:]:
            f, j = gf.gather_tap(lo // kt)
            mid_filter |= j > 0 or lo % kt > 0
            mid_tap |= lo % kt > 0
        undivided |= nit % c.S != 0
    assert mid_filter and mid_tap and undivided
    assert {c.F for c in gf.GATHER_CASES} == {1, 2, 3, 4} and {c.K for c in gf.GATHER_CASES} == {32, 64}
    assert {c.N for c in gf.GATHER_CASES} == {128, 80, 132} and {c.apad for c in gf.GATHER_CASES} == {0, 4} and {c.S for c in gf.GATHER_CASES} == {2, 3}
    ts = {(c.T - c.F) for c in gf.GATHER_CASES if c.T <= c.F}
    assert ts == {-1, 0} and {c.T for c in gf.GATHER_CASES} >= {7, 130}
    assert any(gp.cdiv(c.B * c.T, 128) >= 2 for c in gf.GATHER_CASES)
    # mutation 5 (row shift off by one for even f) against the restatement: every case with an even filter width tells it apart
    for c in gf.GATHER_CASES:
        if c.F < 2 or c.T == 1:
            continue
        rng = np.random.default_rng(gp.seed_of(c.id))
        M = c.B * c.T
        dbank = rng.standard_normal((M, c.F * c.K))
        WTs = [rng.standard_normal((f, c.K, c.N)) for f in range(1, c.F + 1)]
        good, S, n = gf.gather_ref(dbank, WTs, c.T)
        bad = np.zeros_like(good)
        for g in range(c.F * (c.F + 1) // 2):
            f, j = gf.gather_tap(g)
            sh = j - ((f - 1) - (f - 1) // 2) + (1 if f % 2 == 0 else 0)
            bad += gp._shifted(dbank[:, (f - 1) * c.K:f * c.K], c.T, sh) @ WTs[f - 1][j]
        assert (np.abs(bad - good) > gp.element_bound(n, S, 1.0, good)).any(), c.id
    assert not gf.gather_contract(3, 64, 6, 0, 192) and not gf.gather_contract(3, 48, 6, 1, 192) and gf.gather_contract(3, 64, 6, 1, 196)


def test_tn_group_and_strided_cases():
    for name, probs in gf.TN_GROUPS.items():
        assert 3 <= len(probs) <= 5, name
        for p in probs:
            assert p.M % p.T == 0 and p.M in (63, 260) and p.K in (80, 128, 132) and p.N in (128, 4) and p.taps in (1, 3, 8)
            plan = gp.tn_plan(gp.host_ptr(0), p.K, gp.host_ptr(0), p.N, p.M, p.N, p.K, p.taps, p.pad_l)
            assert plan['bm'] == 64 and plan['flags'] == 3               # what launch_gemm_tn_batch puts into its ONE grid
    allp = [p for probs in gf.TN_GROUPS.values() for p in probs]
    assert {p.taps for p in allp} == {1, 3, 8} and {p.K for p in allp} == {80, 128, 132} and {p.N for p in allp} == {128, 4} and {p.M for p in allp} == {63, 260}
    assert any(gp.tn_plan(gp.host_ptr(0), p.K, gp.host_ptr(0), p.N, p.M, p.N, p.K, p.taps, p.pad_l)['merged'] for p in allp)
    assert {(d, m, t) for _, d, m, t in gf.TN_GROUP_RUNS} == {(d, m, t) for d in (False, True) for m in '01' for t in '01'}
    cs = gf.TN_STRIDED_CASES
    assert {c.batch for c in cs} == {1, 3} and {c.M for c in cs} == {1, 7, 65} and {c.K for c in cs} == {5, 37, 130}
    # the reference keeps the batch members apart: read as ONE sequence of batch * M rows, the pad_l = 1 shift pulls the last row of
    # member z - 1 into row 0 of member z, and the result differs
    c = next(c for c in cs if c.id == 'ts-b3-Td7')
    rng = np.random.default_rng(gp.seed_of(c.id))
    A, Y = rng.standard_normal((c.batch, c.M, c.K)), rng.standard_normal((c.batch, c.M, gf.TN_STRIDED_N))
    W0 = np.zeros((c.batch, c.K, gf.TN_STRIDED_N))
    ref, S = gf.tn_strided_ref(A, Y, W0, 1)
    for z in range(c.batch):
        assert np.allclose(ref[z], A[z][:-1].T @ Y[z][1:], rtol=1e-12, atol=1e-12)      # row 0 of every member meets a zero row
    leak = np.stack([(gp._shifted(A.reshape(-1, c.K), c.batch * c.M, -1)[z * c.M:(z + 1) * c.M]).T @ Y[z] for z in range(c.batch)])
    assert np.allclose(leak[0], ref[0]) and (np.abs(leak[1:] - ref[1:]) > gp.element_bound(c.M, S[1:], 1.0, ref[1:])).any()
    # mutation 6 (strideY read as M ldy) against the restatement: member z > 0 would read dY rows from the wrong place
    N = gf.TN_STRIDED_N
    ldy, strideY = N + 4, c.M * (N + 4) + 12
    flat = np.full(c.batch * strideY, np.nan)
    for z in range(c.batch):
        flat[z * strideY:z * strideY + c.M * ldy].reshape(c.M, ldy)[:, :N] = Y[z]
    wrong = np.stack([flat[z * c.M * ldy:z * c.M * ldy + c.M * ldy].reshape(c.M, ldy)[:, :N] for z in range(c.batch)])
    mut, _ = gf.tn_strided_ref(A, wrong, W0, 1)
    assert np.array_equal(mut[0], ref[0]) and not (np.abs(mut[1:] - ref[1:]) <= gp.element_bound(c.M, S[1:], 1.0, ref[1:])).all()
    assert strideY != c.M * ldy and strideY % 4 == 0


def test_the_c_doors_refuse_bad_arguments_before_anything_is_enqueued(built_lib):
    """the C ABI's own checks (no GPU is touched: every call here is refused): TACO_EINVAL with a message that names the argument for a
    null operand, a size out of range, a pitch below the row, an output that meets another operand"""
    import ctypes as C
    L, P = built_lib._lib, C.c_void_p
    a = [P(0x10000 * (i + 1)) for i in range(12)]           # never dereferenced
    two = lambda p, q: (C.c_void_p * 2)(p.value, q.value)
    ints = lambda *v: (C.c_int * len(v))(*v)
    M, T, N, K = 8, 4, 4, 32
    calls = (
        (lambda: L.taco_debug_conv_bank_pool_fwd(a[0], K, two(a[1], a[2]), two(a[3], a[4]), None, a[6], 1.0, a[7], None, 8, M, T, 2, N, K, None), 'scale is null'),
        (lambda: L.taco_debug_conv_bank_pool_fwd(a[0], K, two(a[1], P(0)), two(a[3], P(0)), a[5], a[6], 1.0, a[7], None, 8, M, T, 2, N, K, None), r'W\[1\] is null'),
        (lambda: L.taco_debug_conv_bank_pool_fwd(a[0], K, two(a[1], a[2]), two(a[3], a[4]), a[5], a[6], 1.0, a[7], a[7], 8, M, T, 2, N, K, None), 'pool may not overlap bank'),
        (lambda: L.taco_debug_conv_bank_pool_fwd(a[0], K, two(a[1], a[2]), two(a[3], a[4]), a[5], a[6], 1.0, a[7], None, 7, M, T, 2, N, K, None), 'ldc must be >= F N = 8'),
        (lambda: L.taco_debug_conv_bank_pool_fwd(a[0], K, two(a[1], a[2]), two(a[3], a[4]), a[5], a[6], 1.0, a[7], None, 8, M, 3, 2, N, K, None), 'T must be positive and divide M'),
        (lambda: L.taco_debug_conv_bank_pool_fwd(a[0], K, two(a[1], a[2]), two(a[3], a[4]), a[5], a[6], 1.0, a[7], None, 8, M, T, 17, N, K, None), r'F must be in \[1, 16\]'),
        (lambda: L.taco_debug_conv_gemm_pool_bwd(a[0], K, a[1], N, a[2], a[3], a[4], 1.0, a[2], N, a[6], a[7], M, N, K, 3, T, 1, None), 'C may not overlap pool_x'),
        (lambda: L.taco_debug_conv_gemm_pool_bwd(a[0], K, a[1], N, a[2], a[3], a[4], 1.0, a[5], N, None, a[7], M, N, K, 3, T, 1, None), 'dgamma is null'),
        (lambda: L.taco_debug_conv_gemm_pool_bwd(a[0], K, a[1], N, a[2], a[3], a[4], 1.0, a[5], N, a[6], a[7], 0, N, K, 3, T, 1, None), r'M must be in \[1, 2\^22\]'),
        (lambda: L.taco_debug_conv_gemm_pool_bwd(a[0], K - 1, a[1], N, a[2], a[3], a[4], 1.0, a[5], N, a[6], a[7], M, N, K, 3, T, 1, None), 'lda must be >= K = 32'),
        (lambda: L.taco_debug_bn_maxpool_fwd(a[0], a[1], a[2], a[0], 2, T, N, None), 'y may not overlap x'),
        (lambda: L.taco_debug_bn_maxpool_fwd(a[0], a[1], a[2], a[3], 2, T, 6, None), 'C must be a multiple of 4'),
        (lambda: L.taco_debug_bn_maxpool_bwd(a[0], a[1], None, a[3], a[4], a[5], a[6], 2, T, N, None), 'beta is null'),
        (lambda: L.taco_debug_bn_maxpool_bwd(a[0], a[1], a[2], a[3], a[4], a[5], a[5], 2, T, N, None), 'dgamma may not overlap dbeta'),
        (lambda: L.taco_debug_bank_gather(a[0], 2 * K, two(a[1], a[2]), a[3], N, a[4], N, a[5], 1000, M, T, 2, K, N, 1, 0, None), r'S must be in \[1, 16\]'),
        (lambda: L.taco_debug_bank_gather(a[0], 2 * K, two(a[1], a[2]), a[3], N, a[3], N, a[5], 1000, M, T, 2, K, N, 1, 2, None), 'dx_out may not overlap residual'),
        (lambda: L.taco_debug_bank_gather(a[0], 2 * K - 4, two(a[1], a[2]), a[3], N, a[4], N, a[5], 1000, M, T, 2, K, N, 1, 2, None), 'lda must be >= F K = 64'),
        (lambda: L.taco_debug_conv_gemm_batch_atomic(a[0], 2 * K, two(a[1], a[2]), a[3], N, None, N, M, T, 2, K, N, None), 'dx_out is null'),
        (lambda: L.taco_debug_conv_gemm_rowbias(a[0], K, a[1], N, a[2], N - 1, a[3], N, M, T, N, K, None), 'bias_stride must be >= N = 4'),
        (lambda: L.taco_debug_conv_gemm_rowbias(a[0], K, a[1], N, None, N, a[3], N, M, T, N, K, None), 'rowb is null'),
        (lambda: L.taco_debug_gemm_tn_group(27, None, None, None, None, None, None, None, None, None, None, None, None, None, None), r'n must be in \[1, 26\]'),
        (lambda: L.taco_debug_gemm_tn_group(1, two(a[0], a[0]), ints(K), two(a[1], a[1]), ints(N), two(a[0], a[0]), ints(N), None, ints(M), ints(N), ints(K), ints(3),
                                    ints(T), ints(1), None), r'W\[0\] may not overlap A\[0\]'),
        (lambda: L.taco_debug_gemm_tn_group(1, two(a[0], a[0]), ints(K), two(a[1], a[1]), ints(N), two(a[2], a[2]), ints(N), None, ints(M), ints(N), ints(K), ints(0),
                                    ints(T), ints(1), None), r'taps\[0\] must be in \[1, 64\]'),
        (lambda: L.taco_debug_gemm_tn_strided(a[0], K, M * K, a[1], N, M * N - 1, a[2], N, K * N, M, N, K, M, 1, 2, None), r'strideY must be >= \(M - 1\) ldy \+ N = 32'),
        (lambda: L.taco_debug_gemm_tn_strided(a[0], K, M * K, a[1], N, M * N, a[0], N, K * N, M, N, K, M, 1, 2, None), 'W may not overlap A'),
        (lambda: L.taco_debug_gemm_tn_strided(a[0], K, M * K, a[1], N, M * N, a[2], N, K * N, M, N, K, M, 1, 0, None), r'batch must be in \[1, 4096\]'),
    )
    assert len(calls) == 26
    import re
    for call, msg in calls:
        assert call() == -1                                  # TACO_EINVAL
        got = built_lib.last_error()
        assert re.search(msg, got) and got.startswith('taco_debug_'), (msg, got)


def test_rowbias_reference_and_cases():
    rng = np.random.default_rng(1)
    A, W, rb = rng.standard_normal((6, 5)), rng.standard_normal((5, 4)), rng.standard_normal((2, 4))
    C, S = gf.rowbias_ref(A, W, rb, 3)
    for m in range(6):
        assert np.allclose(C[m], A[m] @ W + rb[m // 3])
    for c in gf.ROWBIAS_CASES:
        assert c.M // c.T == 3 and c.T == 50 and any(m // c.T != (m + 63) // c.T for m in range(0, c.M, 64))     # a 64-row tile spans two sequences
    assert {c.stride_pad for c in gf.ROWBIAS_CASES} == {0, 4} and {c.g2 for c in gf.ROWBIAS_CASES} == {'0', '1'}


def test_the_wrappers_refuse_bad_arguments_by_name(built_lib):
    """every check runs on tensors of any device and the device check comes last: CPU tensors reach it only when all else is right"""
    lib, z = built_lib, torch.zeros
    M, T, N, K, F = 8, 4, 4, 32, 2
    pf = dict(x=z(M * K), W=[z(f * K * N) for f in (1, 2)], bias=[z(N), None], scale=z(F * N), shift=z(F * N), pool=z(M * F * N), M=M, T=T, N=N, K=K,
              bank=z(M * F * N))
    pb = dict(A=z(M * K), W=z(3 * K * N), pool_x=z(M * N), scale=z(N), shift=z(N), C_out=z(M * N), dgamma=z(N), dbeta=z(N), M=M, T=T, N=N, K=K)
    bg = dict(dbank=z(M * F * K), WT=[z(f * K * N) for f in (1, 2)], dx_out=z(M * N), slabs=z(4 * M * N), M=M, T=T, K=K, N=N, S=2, residual=z(M * N))
    rb = dict(A=z(M * K), W=z(K * N), rowb=z(2 * N), C_out=z(M * N), M=M, T=T, N=N, K=K)
    bw = dict(x=z(M * N), gamma=z(N), beta=z(N), dy=z(M * N), dx=z(M * N), dgamma=z(N), dbeta=z(N), B=2, T=T, C_cols=N)
    tg = dict(problems=[dict(A=z(M * K), Y=z(M * N), W=z(3 * K * N), dbias=z(N), M=M, T=T, N=N, K=K, taps=3, pad_l=1)])
    ts = dict(A=z(2 * M * K), Y=z(2 * M * N + 12), W=z(2 * K * N), M=M, N=N, K=K, batch=2, strideA=M * K, strideY=M * N + 12, strideW=K * N)
    at = {k: v for k, v in bg.items() if k not in ('slabs', 'S')}
    fw = dict(x=z(M * N), gamma=z(N), beta=z(N), y=z(M * N), B=2, T=T, C_cols=N)
    for fn, args, first in ((lib.debug_conv_bank_pool_fwd, pf, 'x'), (lib.debug_conv_gemm_pool_bwd, pb, 'A'), (lib.debug_bank_gather, bg, 'dbank'),
                            (lib.debug_conv_gemm_batch_atomic, at, 'dbank'), (lib.debug_conv_gemm_rowbias, rb, 'A'), (lib.debug_bn_maxpool_fwd, fw, 'x'),
                            (lib.debug_bn_maxpool_bwd, bw, 'x'), (lib.debug_gemm_tn_group, tg, 'A\\[0\\]'), (lib.debug_gemm_tn_strided, ts, 'A')):
        with pytest.raises(ValueError, match=r'^%s: %s must be on the GPU' % (fn.__name__, first)):
            fn(**args)
    for fn, args, change, msg in (
            (lib.debug_conv_bank_pool_fwd, pf, dict(T=3), r'T must divide M'),
            (lib.debug_conv_bank_pool_fwd, pf, dict(W=[]), r'W must be a list of 1 to 16 tensors'),
            (lib.debug_conv_bank_pool_fwd, pf, dict(bias=[z(N)]), r'bias must be a list of 2 tensors or Nones'),
            (lib.debug_conv_bank_pool_fwd, pf, dict(W=[z(K * N), z(2 * K * N - 1)]), r'W\[1\] must hold at least 256 floats, got 255'),
            (lib.debug_conv_bank_pool_fwd, pf, dict(ldc=F * N - 1), r'ldc must be >= 8, got 7'),
            (lib.debug_conv_bank_pool_fwd, pf, dict(pool=z(M * F * N).view(M, F * N)), r'pool must be a contiguous float32 tensor of shape \(n,\)'),
            (lib.debug_conv_bank_pool_fwd, pf, dict(bank=pf['pool']), r'pool may not overlap bank'),
            (lib.debug_conv_bank_pool_fwd, pf, dict(scale=None), r'scale must be'),
            (lib.debug_conv_gemm_pool_bwd, pb, dict(C_out=pb['pool_x']), r'C_out may not overlap pool_x'),
            (lib.debug_conv_gemm_pool_bwd, pb, dict(dbeta=pb['dgamma']), r'dgamma may not overlap dbeta'),
            (lib.debug_conv_gemm_pool_bwd, pb, dict(N=0), r'N must be an integer in \[1, 16384\]'),
            (lib.debug_conv_gemm_pool_bwd, pb, dict(pool_x=z(M * N).double()), r'pool_x must be'),
            (lib.debug_conv_gemm_pool_bwd, pb, dict(ldc=N + 4), r'pool_x must hold at least 60 floats, got 32'),
            (lib.debug_bank_gather, bg, dict(S=0), r'S must be an integer in \[1, 16\]'),
            (lib.debug_bank_gather, bg, dict(dx_out=bg['residual']), r'dx_out may not overlap residual'),
            (lib.debug_bank_gather, bg, dict(slabs=None), r'slabs must be'),
            (lib.debug_bank_gather, bg, dict(lda=F * K - 4), r'lda must be >= 64, got 60'),
            (lib.debug_conv_gemm_batch_atomic, at, dict(WT=[z(K * N), None]), r'WT\[1\] must be'),
            (lib.debug_conv_gemm_rowbias, rb, dict(bias_stride=N - 1), r'bias_stride must be >= 4, got 3'),
            (lib.debug_conv_gemm_rowbias, rb, dict(rowb=z(N)), r'rowb must hold at least 8 floats, got 4'),
            (lib.debug_bn_maxpool_fwd, fw, dict(C_cols=6), r'C must be a multiple of 4'),
            (lib.debug_bn_maxpool_fwd, fw, dict(y=fw['x']), r'y may not overlap x'),
            (lib.debug_bn_maxpool_bwd, bw, dict(dx=bw['dy']), r'dx may not overlap dy'),
            (lib.debug_bn_maxpool_bwd, bw, dict(B=0), r'B must be an integer in \[1, 4194304\]'),
            (lib.debug_gemm_tn_group, tg, dict(problems=[]), r'problems must be a list of 1 to 26 dicts'),
            (lib.debug_gemm_tn_group, tg, dict(problems=[dict(tg['problems'][0], taps=0)]), r'problems\[0\]: taps must be an integer in \[1, 64\]'),
            (lib.debug_gemm_tn_group, tg, dict(problems=[dict(tg['problems'][0], A=tg['problems'][0]['W'])]), r'W\[0\] may not overlap A\[0\]'),
            (lib.debug_gemm_tn_strided, ts, dict(strideY=M * N - 1), r'strideY must be >= 32, got 31'),
            (lib.debug_gemm_tn_strided, ts, dict(batch=3), r'A must hold at least 768 floats, got 512')):
        with pytest.raises(ValueError, match='^%s: %s' % (fn.__name__, msg)):
            fn(**dict(args, **change))
