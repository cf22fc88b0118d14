"""CPU checks of the training monitor (taco_tensor_stats): the NumPy restatement against a second formulation of the bucket rule,
lib.tensor_stats_edges against the rule, the host-built plan and its refusals, the wrappers' refusals before any device call,
Tacotron.monitor_sites against the parameter and workspace tables, train.monitor_line on hand-made rows, the --monitor flag and the
header's documentation.  No compute call: there is no GPU here."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import monitor_ref as mr

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'taco_hip.h')
BUCKETS = [(-24, 15, 2), (-24, 15, 0), (-24, 15, 3), (3, 3, 1), (0, 0, 0), (-126, 127, 3), (-126, 127, 0), (-126, -126, 2), (127, 127, 3)]


def _probe_values(e_lo, e_hi, s):
    """every bucket edge, its predecessor and its successor in both signs, zeros, subnormals, the largest finite values, random bits"""
    edges = mr.edge_values(e_lo, e_hi, s)
    top = np.array([math.ldexp(1.0, e_hi + 1)], dtype=np.float32) if e_hi < 127 else np.array([], dtype=np.float32)
    edges = np.concatenate([edges, top])
    near = np.concatenate([edges, mr.prev_toward_zero(edges), (edges.view(np.uint32) + np.uint32(1)).view(np.float32)])
    special = np.array([0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38, 1.17549435e-38, 3.4028235e38, -3.4028235e38, 1.0, -1.0, 0.75, 1.5],
                       dtype=np.float32)
    rnd = np.random.default_rng(5).integers(0, 1 << 32, size=20000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    v = np.concatenate([near, -near, special, rnd])
    return v[np.isfinite(v)]


@pytest.mark.parametrize('e_lo,e_hi,s', BUCKETS)
def test_the_two_bucket_formulations_agree(e_lo, e_hi, s):
    v = _probe_values(e_lo, e_hi, s)
    a, b = mr.bucket_bits(v, e_lo, e_hi, s), mr.bucket_frexp(v, e_lo, e_hi, s)
    bad = np.flatnonzero(a != b)
    assert not len(bad), (v[bad[:5]], a[bad[:5]], b[bad[:5]])
    nb = mr.n_bins(e_lo, e_hi, s)
    assert a.min() >= 0 and a.max() < nb
    nm = (nb - 1) // 2
    assert (a[v == 0] == nm).all() and (a[v > 0] >= nm).all() and (a[v < 0] <= nm).all()
    # symmetric: -x lands in the mirrored bin
    assert (mr.bucket_bits(-v, e_lo, e_hi, s) == 2 * nm - a).all()


def test_restatement_on_hand_numbers():
    x = np.array([1.0, -2.0, 0.0, -0.0, np.nan, np.inf, -np.inf, 0.5, 3.0, 1e-30], dtype=np.float32)
    counts, moments, hist = mr.stats(x, e_lo=-1, e_hi=1, s=1)
    assert counts.tolist() == [10, 7, 1, 1, 1, 2]
    assert moments[0] == math.fsum([1.0, -2.0, 0.5, 3.0, float(np.float32(1e-30))]) and moments[2] == -2.0 and moments[3] == 3.0
    assert moments[4] == 3.0 and moments[1] == math.fsum([1.0, 4.0, 0.25, 9.0, float(np.float32(1e-30)) ** 2])
    # buckets [0.5, 0.75) [0.75, 1) [1, 1.5) [1.5, 2) [2, 3) [3, inf): Nm = 6, NB = 13
    want = np.zeros(13, dtype=np.int64)
    want[6] = 3            # +0, -0, 1e-30
    want[6 + 1] = 1        # 0.5
    want[6 + 3] = 1        # 1.0
    want[6 + 6] = 1        # 3.0
    want[6 - 5] = 1        # -2.0
    assert hist.tolist() == want.tolist() and hist.sum() == counts[1]
    empty = mr.stats(np.array([np.nan, np.inf], dtype=np.float32))
    assert empty[1].tolist() == [0.0, 0.0, np.inf, -np.inf, 0.0] and empty[2].sum() == 0
    assert mr.stats(np.array([0.0, -0.0], dtype=np.float32))[1][2:4].tolist() == [-0.0, 0.0]
    assert np.signbit(mr.stats(np.array([0.0, -0.0], dtype=np.float32))[1][2])


@pytest.mark.parametrize('e_lo,e_hi,s', BUCKETS)
def test_edges_open_their_buckets(built_lib, e_lo, e_hi, s):
    edges = built_lib.tensor_stats_edges(e_lo, e_hi, s)
    nb = mr.n_bins(e_lo, e_hi, s)
    nm = (nb - 1) // 2
    assert edges.dtype == np.float64 and edges.shape == (nb + 1,) and (np.diff(edges) > 0).all()
    assert edges[0] == -np.inf and edges[-1] == np.inf
    pos = edges[nm + 1:-1].astype(np.float32)
    assert (pos.astype(np.float64) == edges[nm + 1:-1]).all()                  # every edge is an fp32 value
    assert (pos == mr.edge_values(e_lo, e_hi, s)).all()
    at = np.arange(nm + 1, 2 * nm + 1)                                         # edges[i] opens bin i ...
    assert (mr.bucket_bits(pos, e_lo, e_hi, s) == at).all()
    assert (mr.bucket_bits(mr.prev_toward_zero(pos), e_lo, e_hi, s) == at - 1).all()   # ... and its predecessor is in the one before
    neg = edges[1:nm + 1].astype(np.float32)                                   # mirrored: edges[i] closes bin i - 1 from above
    assert (neg.astype(np.float64) == edges[1:nm + 1]).all()
    assert (mr.bucket_bits(neg, e_lo, e_hi, s) == np.arange(0, nm)).all()
    assert (mr.bucket_bits(mr.prev_toward_zero(neg), e_lo, e_hi, s) == np.arange(1, nm + 1)).all()
    sig = inspect.signature(built_lib.tensor_stats_edges).parameters
    assert [sig[k].default for k in sig] == [-24, 15, 2] and len(built_lib.tensor_stats_edges()) == 322
    for bad in (dict(e_lo=-127), dict(e_hi=128), dict(e_lo=3, e_hi=2), dict(sub_bits=4), dict(sub_bits=-1), dict(sub_bits=1.5)):
        with pytest.raises(ValueError):
            built_lib.tensor_stats_edges(**bad)


# ---- the plan ------------------------------------------------------------------------------------------------------------------------
def _plan_raw(lib, segs, base_floats):
    n = len(segs)
    flat = (C.c_int64 * (2 * n))(*[v for s in segs for v in s])
    nbytes = lib._lib.taco_tensor_stats_plan_bytes(flat, n)
    blob = np.full(max(nbytes, 8) // 8 + 4, -7, dtype=np.int64)
    items = C.c_int32(-1)
    rc = lib._lib.taco_tensor_stats_plan(flat, n, base_floats, C.c_void_p(blob.ctypes.data), nbytes, C.byref(items))
    return rc, nbytes, blob, items.value


def test_plan_lists_every_chunk_once(built_lib):
    lib = built_lib
    Cc = lib.STATS_CHUNK
    assert Cc == int(re.search(r'#define\s+TACO_STATS_CHUNK\s+(\d+)', open(HDR).read()).group(1)) and Cc % 256 == 0
    segs = [(0, 0), (5, 1), (3, Cc - 3), (3, Cc - 2), (4, Cc), (7, 3 * Cc), (1, 2 * Cc + 7), (100, 0), (0, 128)]
    rc, nbytes, blob, n_items = _plan_raw(lib, segs, 7 + 3 * Cc)
    assert rc == 0
    chunks = [0 if s == 0 else -(-((o & 3) + s) // Cc) for o, s in segs]
    assert chunks == [0, 1, 1, 2, 1, 4, 3, 0, 1] and n_items == sum(chunks)
    assert nbytes == 32 + 32 * len(segs) + 8 * n_items
    assert blob[1:4].tolist() == [len(segs), n_items, 7 + 3 * Cc]
    table = blob[4:4 + 4 * len(segs)].reshape(-1, 4)
    assert table[:, :2].tolist() == [list(s) for s in segs] and table[:, 3].tolist() == chunks
    assert table[:, 2].tolist() == np.concatenate([[0], np.cumsum(chunks)[:-1]]).tolist()
    items = blob[4 + 4 * len(segs):nbytes // 8].view(np.int32).reshape(-1, 2)
    assert items.tolist() == [[i, c] for i, k in enumerate(chunks) for c in range(k)]
    assert (blob[nbytes // 8:] == -7).all()                                    # nothing behind the blob
    p = lib.tensor_stats_plan(segs, 7 + 3 * Cc, device='cpu')
    assert (p.n, p.n_items, p.base_floats) == (len(segs), n_items, 7 + 3 * Cc) and p.header.tolist() == blob[:4].tolist()
    assert p.dev.numpy().tolist() == blob[:nbytes // 8].tolist()
    NB = 321
    assert lib.tensor_stats_workspace_bytes(p.n, p.n_items, NB) >= p.n_items * (48 + 4 * NB)
    with pytest.raises(lib.TacoError):
        lib.tensor_stats_workspace_bytes(p.n, p.n_items, 320)                   # NB is odd


def test_plan_refusals(built_lib):
    lib = built_lib
    for segs, base in (([(0, 11)], 10), ([(10, 1)], 10), ([(-1, 2)], 10), ([(0, -1)], 10), ([(0, 1), (4, 7)], 10)):
        rc, _, blob, _ = _plan_raw(lib, segs, base)
        assert rc == -1 and lib.last_error().startswith('tensor_stats:') and 'segment %d' % (len(segs) - 1) in lib.last_error()
        assert (blob == -7).all()
        with pytest.raises(ValueError):
            lib.tensor_stats_plan(segs, base, device='cpu')
    assert _plan_raw(lib, [(0, 10)], 10)[0] == 0 and _plan_raw(lib, [(10, 0)], 10)[0] == 0
    one = (C.c_int64 * 2)(0, 1)
    many = (C.c_int64 * (2 * (lib.STATS_MAX_SEGMENTS + 1)))()
    assert lib._lib.taco_tensor_stats_plan_bytes(one, 0) == -1 and lib._lib.taco_tensor_stats_plan_bytes(None, 1) == -1
    assert lib._lib.taco_tensor_stats_plan_bytes(many, lib.STATS_MAX_SEGMENTS + 1) == -1
    assert lib._lib.taco_tensor_stats_plan_bytes(many, lib.STATS_MAX_SEGMENTS) == 32 + 32 * lib.STATS_MAX_SEGMENTS
    blob, items = np.zeros(64, dtype=np.int64), C.c_int32(0)
    for n in (0, -1, lib.STATS_MAX_SEGMENTS + 1):
        assert lib._lib.taco_tensor_stats_plan(many, n, 10, C.c_void_p(blob.ctypes.data), 512, C.byref(items)) == -1
        assert 'n=%d' % n in lib.last_error()
    assert lib._lib.taco_tensor_stats_plan(one, 1, 10, C.c_void_p(blob.ctypes.data), 8, C.byref(items)) == -1   # blob too small
    assert 'plan_bytes' in lib.last_error() and not blob.any()
    for bad in ([], [(0, 1)] * (lib.STATS_MAX_SEGMENTS + 1), [(0.5, 1)], [(0, True)], [3], None):
        with pytest.raises(ValueError):
            lib.tensor_stats_plan(bad, 10, device='cpu')
    with pytest.raises(ValueError):
        lib.tensor_stats_plan([(0, 1)], -1, device='cpu')


def test_library_refuses_bad_arguments(built_lib):
    """every TACO_EINVAL case of the call itself, with its message.  The refusals come before the launch, so host memory stands in
    for the device buffers and nothing of it changes."""
    lib = built_lib
    rc, nbytes, blob, n_items = _plan_raw(lib, [(0, 5), (8, 3)], 16)
    assert rc == 0 and n_items == 2
    store = np.zeros(64, dtype=np.float32)
    base = store[(-(store.ctypes.data // 4)) % 4:][:16]
    out = {k: np.full(n, -7, dtype=np.int64) for k, n in (('counts', 12), ('moments', 10), ('hist', 2 * 321), ('work', 4096))}
    p = lambda x: C.c_void_p(x.ctypes.data)   # noqa: E731
    good = dict(base=p(base), plan=p(blob), header=p(blob), n=2, n_items=2, e_lo=-24, e_hi=15, s=2, counts=p(out['counts']),
                moments=p(out['moments']), hist=p(out['hist']), work=p(out['work']))
    other = blob.copy()
    other[2] = 3
    untagged = blob.copy()
    untagged[0] = 0
    cases = [(dict(base=None), 'NULL'), (dict(plan=None), 'NULL'), (dict(header=None), 'NULL'), (dict(counts=None), 'NULL'),
             (dict(moments=None), 'NULL'), (dict(hist=None), 'NULL'), (dict(work=None), 'NULL'),
             (dict(n=0), 'n=0'), (dict(n=-1), 'n=-1'), (dict(n=lib.STATS_MAX_SEGMENTS + 1), 'n=%d' % (lib.STATS_MAX_SEGMENTS + 1)),
             (dict(n_items=-1), 'n_items'), (dict(e_lo=-127), 'e_lo=-127'), (dict(e_hi=128), 'e_hi=128'), (dict(e_lo=3, e_hi=2), 'e_lo=3'),
             (dict(s=-1), 'sub_bits=-1'), (dict(s=4), 'sub_bits=4'),
             (dict(n=1), 'header'), (dict(n_items=1), 'header'), (dict(header=p(other)), 'header'), (dict(header=p(untagged)), 'header'),
             (dict(base=C.c_void_p(base.ctypes.data + 4)), '16-byte'), (dict(work=C.c_void_p(out['work'].ctypes.data + 4)), '8-byte')]
    for kw, word in cases:
        a = dict(good, **kw)
        rc = lib._lib.taco_tensor_stats(a['base'], a['plan'], a['header'], a['n'], a['n_items'], a['e_lo'], a['e_hi'], a['s'], a['counts'],
                                        a['moments'], a['hist'], a['work'], None)
        assert rc == -1, kw
        assert lib.last_error().startswith('tensor_stats:') and word in lib.last_error(), (kw, lib.last_error())
    assert all((v == -7).all() for v in out.values()) and not store.any()


def test_wrapper_refuses_bad_arguments_before_any_device_call(built_lib):
    lib = built_lib
    plan = lib.tensor_stats_plan([(0, 5), (8, 3)], 16, device='cpu')
    base = torch.zeros(16)
    called = []
    real = lib._lib.taco_tensor_stats
    bad = [dict(base=base.double()), dict(base=torch.zeros(15)), dict(base=torch.zeros(4, 8).t()), dict(base=np.zeros(16, dtype=np.float32)),
           dict(plan=None), dict(plan=(0, 5)), dict(e_lo=-127), dict(e_hi=128), dict(e_lo=3, e_hi=2), dict(sub_bits=4), dict(sub_bits=True),
           dict(counts=torch.zeros(2, 6)), dict(counts=torch.zeros(3, 6, dtype=torch.int64)), dict(moments=torch.zeros(2, 5)),
           dict(moments=torch.zeros(2, 4, dtype=torch.float64)), dict(hist=torch.zeros(2, 320, dtype=torch.int64)),
           dict(hist=torch.zeros(2, 321, dtype=torch.int32)), dict(work=torch.zeros(1 << 16)), dict(work=torch.zeros(0, dtype=torch.uint8)),
           dict()]                                                              # everything right, but on the CPU
    try:
        lib._lib.taco_tensor_stats = lambda *a: called.append(a) or 0
        for kw in bad:
            with pytest.raises(ValueError):
                lib.tensor_stats(**dict(dict(base=base, plan=plan), **kw))
    finally:
        lib._lib.taco_tensor_stats = real
    assert not called
    sig = inspect.signature(lib.tensor_stats).parameters
    assert [(k, sig[k].default) for k in list(sig)[2:]] == [('e_lo', -24), ('e_hi', 15), ('sub_bits', 2), ('counts', None), ('moments', None),
                                                            ('hist', None), ('work', None)]
    assert lib.TensorStats._fields == ('counts', 'moments', 'hist')
    assert lib.STATS_COUNTS == mr.COUNTS and lib.STATS_MOMENTS == mr.MOMENTS


# ---- the model's sites ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('r,S', [(2, 1), (5, 1), (2, 7)])
def test_monitor_sites_against_the_tables(built_lib, r, S):
    from tacotron_amd import model
    lib = built_lib
    shape = lib.make_shape(3, 10, 6, r, 20, S)
    sites = model.monitor_sites(shape)
    assert tuple(sites) and set(sites) == set(model.MONITOR_FORWARD + model.MONITOR_UPDATE)
    table = lib.param_table(shape)
    for buf, group in (('params', 'param'), ('grads', 'grad'), ('adam_m', 'adam_m'), ('adam_v', 'adam_v')):
        assert [(n, o, s) for n, o, s in sites[buf]] == [('%s/%s' % (group, n), o, s) for n, o, s, _ in table]   # once each, in order
    spans = sorted((o, o + s) for _, o, s in sites['params'])
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] == lib.param_count(shape)
    rows = {n: (o, s, d) for n, o, s, d in lib.workspace_table(shape, True)}
    B, Tt, Td = 3, 10, 6
    want = {'pre_net_out': ('enc.p2', (B * Tt, 128)),
            'encoder/conv_bank': ('enc.pool', (B * Tt, 16 * 128)), 'encoder/conv_proj_pre_bn': ('enc.pj2pre', (B * Tt, 128)),
            'encoder/conv_res': ('enc.res', (B * Tt, 128)), 'encoder/highway_out': ('enc.h4', (B * Tt, 128)),
            'encoder/encoded': ('enc.out', (B * Tt, 256)),
            'post/conv_bank': ('post.pool', (B * Td * r, 8 * 128)), 'post/conv_proj_pre_bn': ('post.pj2pre', (B * Td * r, 80)),
            'post/conv_res': ('post.res', (B * Td * r, 80)), 'post/highway_out': ('post.h4', (B * Td * r, 128)),
            'post/encoded': ('post.out', (B * Td * r, 256))}
    got = {n: (o, s) for n, o, s in sites['workspace']}
    assert list(got) == list(want)
    for name, (row, dims) in want.items():
        assert row in rows, row
        assert got[name] == rows[row][:2] and got[name][1] == int(np.prod(dims)), (name, rows[row])
    assert sites['seq2seq_output'] == [('seq2seq_output', 0, B * Td * 80 * r)] and sites['output'] == [('output', 0, B * Td * 1025 * r)]
    names = [n for buf in model.MONITOR_FORWARD + model.MONITOR_UPDATE for n, _, _ in sites[buf]]
    assert len(set(names)) == len(names) == 13 + 4 * len(table)
    assert 'conv_proj' not in ' '.join(n.replace('conv_proj_pre_bn', '') for n in names)   # no buffer is invented for it
    # every buffer's segments make a plan
    for buf, n_floats in (('params', lib.param_count(shape)), ('workspace', lib.workspace_bytes(shape, True) // 4)):
        p = lib.tensor_stats_plan([(o, s) for _, o, s in sites[buf]], n_floats, device='cpu')
        assert p.n == len(sites[buf]) and p.n_items >= p.n
    sig = inspect.signature(model.Tacotron.step).parameters
    assert sig['monitor'].default is False and 'after the update' in ' '.join(model.Tacotron.step.__doc__.lower().split())


# ---- the driver ----------------------------------------------------------------------------------------------------------------------
def test_monitor_line_on_hand_made_rows():
    from tacotron_amd import train
    names = ['pre_net_out', 'output', 'param/a', 'param/b', 'grad/a', 'grad/b', 'adam_m/a']
    #          size finite nan +inf -inf zeros
    counts = [[100, 100, 0, 0, 0, 25], [10, 10, 0, 0, 0, 0], [4, 4, 0, 0, 0, 0], [16, 16, 0, 0, 0, 0], [4, 4, 0, 0, 0, 0], [16, 16, 0, 0, 0, 0],
              [4, 4, 0, 0, 0, 0]]
    #           sum sumsq min max absmax
    moments = [[0, 1, 0, 1, 1], [0, 1, 0, 1, 1], [0, 4.0, -1, 1, 1], [0, 64.0, -2, 2, 2], [0, 1.0, -1, 1, 1], [0, 1.0, -1, 1, 1], [0, 0, 0, 0, 0]]
    line = train.monitor_line(names, counts, moments, 0.1)
    assert line == 'monitor grad-rms max 5.000e-01 (a) lr|g|/|w| max 5.000e-02 (a) pre_net_out zeros 25.0% non-finite 0'
    counts[5][1:5] = [13, 1, 2, 0]          # grad/b: one NaN, two +Inf; 13 finite elements with sumsq 52 -> RMS 2
    moments[5][1] = 52.0
    counts[1][1:5] = [9, 0, 0, 1]           # output: one -Inf
    line = train.monitor_line(np.array(names), np.array(counts), np.array(moments), 0.1)
    assert line == ('monitor grad-rms max 2.000e+00 (b) lr|g|/|w| max 9.014e-02 (b) pre_net_out zeros 25.0% non-finite 2: output, grad/b')
    assert train.monitor_nonfinite(names, counts) == ['output', 'grad/b']
    for i in (2, 3, 6):
        counts[i][2] = 1
    assert train.monitor_line(names, counts, moments, 0.1).endswith('non-finite 5: output, param/a, param/b, ...')
    assert 'proxy' in ' '.join(train.monitor_line.__doc__.lower().split()) and 'not computed' in train.monitor_line.__doc__
    empty = train.monitor_line(['grad/a'], [[0, 0, 0, 0, 0, 0]], [[0, 0, np.inf, -np.inf, 0]], 1.0)
    assert empty == 'monitor grad-rms max 0.000e+00 (-) lr|g|/|w| max 0.000e+00 (-) pre_net_out zeros - non-finite 0'


def test_the_flag_and_the_default():
    from tacotron_amd import train
    assert train.parse_args(['--monitor']).monitor is True and train.parse_args([]).monitor is False
    sig = inspect.signature(train.train).parameters
    assert sig['monitor'].default is False
    assert list(sig)[:7] == ['config', 'num_steps', 'log_every', 'save_every', 'corpus_fp32', 'align_log', 'holdout']   # nothing moved


# ---- the header ----------------------------------------------------------------------------------------------------------------------
def _args(decl):
    return [' '.join(a.split()) for a in decl.replace('\n', ' ').split(',')]


def test_header_documents_the_entry_points(built_lib):
    hdr = open(HDR).read()
    fn = re.search(r'\bint taco_tensor_stats\(([^)]*)\);', hdr)
    assert fn
    assert _args(fn.group(1)) == ['const float* base', 'const void* plan_dev', 'const void* plan_header', 'int n', 'int n_items', 'int e_lo',
                                  'int e_hi', 'int sub_bits', 'int64_t* counts', 'double* moments', 'int64_t* hist', 'void* workspace',
                                  'void* stream']
    assert re.search(r'\bint64_t taco_tensor_stats_plan_bytes\(const int64_t\* segments, int n\);', hdr)
    assert re.search(r'\bint taco_tensor_stats_plan\(const int64_t\* segments, int n, int64_t base_floats, void\* plan, int64_t plan_bytes, '
                     r'int32_t\* n_items\);', hdr)
    assert re.search(r'\bint64_t taco_tensor_stats_workspace_bytes\(int n, int n_items, int NB\);', hdr)
    assert int(re.search(r'#define\s+TACO_VERSION\s+(\d+)', hdr).group(1)) == 120 == built_lib.version()
    assert int(re.search(r'#define\s+TACO_STATS_MAX_SEGMENTS\s+(\d+)', hdr).group(1)) == built_lib.STATS_MAX_SEGMENTS == 4096
    assert int(re.search(r'#define\s+TACO_STATS_MAX_BINS\s+(\d+)', hdr).group(1)) == mr.n_bins(-126, 127, 3)
    comment = ' '.join(hdr[hdr.index('/* ---- training monitor'):fn.start()].split())
    for word in ('size, finite, NaN, +Inf, -Inf, exact zeros', 'sum, sumsq, min, max, absmax', '0, 0, +inf, -inf, 0', 'u >> (23 - s)',
                 'min(k, hi) - lo + 1', 'NB = 2 Nm + 1', '-126 <= e_lo <= e_hi <= 127', 'ORDER OF THE SUMS', 'partial-and-fold',
                 'No float atomics', 'may overlap', 'bit-identical to a call with that segment alone', 'graph-capturable',
                 'detect them by the symbol', 'arbitrary bytes', 'TACO_STATS_CHUNK', 'never read and may hold NaN'):
        assert word in comment, word
    P, I, L = C.c_void_p, C.c_int, C.c_int64
    assert built_lib.EXPORTS['taco_tensor_stats'] == (I, [P, P, P, I, I, I, I, I, P, P, P, P, P])
    assert built_lib.EXPORTS['taco_tensor_stats_workspace_bytes'] == (L, [I, I, I])
    for name in ('taco_tensor_stats', 'taco_tensor_stats_plan', 'taco_tensor_stats_plan_bytes', 'taco_tensor_stats_workspace_bytes'):
        assert hasattr(C.CDLL(built_lib.LIB_PATH), name)
