"""Comparison bars of the stage-by-stage backward tests (tests/test_gpu_backward_stages.py): one HIP buffer against the fp64
oracle's gradient of the matching intermediate, as a whole tensor AND row by row.  A weight gradient sums over every
(batch row, step), so a mistake confined to one row is diluted by the row count; the row bar sees it undiluted.  The forward
stage tests (tests/test_gpu_forward_stages.py) compare forward values the same way against bars of their own."""
import numpy as np

# Measured on MI355X at every shape of tests/test_gpu_backward_stages.py: worst tensor rel-L2 9.3e-6 (21x inside the suite's
# gradient bar of 2e-4, so this bar is tightened to 5e-5), worst row 5.6e-4 (S2, d keys; 3.6x inside 2e-3, which stays).
TENSOR_BAR = 5e-5   # rel-L2 of the whole tensor
ROW_BAR = 2e-3      # worst row: |hip_row - ref_row| / max(|ref_row|, 1e-2 RMS row norm)

# The forward stage tests (tests/test_gpu_forward_stages.py, map in tests/forward_map.py): forward VALUES against the fp64
# oracle's, same statistics.  Measured on MI355X at every shape of that module: worst tensor rel-L2 8.574e-7 (dec.vwxc, B=40 r=5),
# worst row 2.210e-6 (dec.vwxc, B=70 r=5, b 45, s 10).  Each bar is 4x its measurement rounded up to one significant digit (the
# backward bars above sit at 3.6x by the same reasoning: the slack covers shapes and seeds not in the table), and may never exceed
# 3e-5 (the loosest forward stage bar of test_encoder_stages_vs_oracle) resp. ROW_BAR: a measurement that needs more is a finding
# about a kernel.
FWD_TENSOR_BAR = 4e-6   # 4 x 8.574e-7 = 3.43e-6
FWD_ROW_BAR = 9e-6      # 4 x 2.210e-6 = 8.84e-6

# The op-level tests of the CBHG tail (tests/test_gpu_cbhg_tail.py, cases in tests/cbhg_tail_cases.py): kernel -> (tensor bar, row bar).
# Measured on MI355X over the whole case table (worst tensor rel-L2 / worst row against fp64; beside it the plain fp32 torch
# restatement of the same op on the same cases, tests/cbhg_tail_ref.py F32):
#     kernel             tensor          row    fp32 tensor     fp32 row
#     bigru_fwd       1.131e-07    1.336e-07      1.012e-07    1.244e-07
#     bigru_bwd       1.909e-07    2.033e-07      2.755e-07    2.755e-07
#     highway_fwd     2.478e-07    3.163e-07      3.365e-07    5.004e-07
#     highway_bwd     3.733e-07    5.882e-07      4.805e-07    6.423e-07
#     prenet_fwd      2.666e-07    3.748e-07      4.290e-07    4.290e-07
#     prenet_bwd      1.861e-07    2.245e-07      2.992e-07    2.992e-07
# Each bar is 4 x its measurement rounded up to one significant digit (the slack is for seeds that are not in the table).  Forward
# values may never exceed FWD_TENSOR_BAR / FWD_ROW_BAR, gradients never TENSOR_BAR / ROW_BAR: a measurement that needs more is a
# finding about a kernel.
CBHG_TAIL_BARS = {
    'bigru_fwd': (5e-7, 6e-7),     # 4 x 1.131e-7 = 4.52e-7, 4 x 1.336e-7 = 5.34e-7
    'bigru_bwd': (8e-7, 9e-7),     # 4 x 1.909e-7 = 7.64e-7, 4 x 2.033e-7 = 8.13e-7
    'highway_fwd': (1e-6, 2e-6),   # 4 x 2.478e-7 = 9.91e-7, 4 x 3.163e-7 = 1.27e-6
    'highway_bwd': (2e-6, 3e-6),   # 4 x 3.733e-7 = 1.49e-6, 4 x 5.882e-7 = 2.35e-6
    'prenet_fwd': (2e-6, 2e-6),    # 4 x 2.666e-7 = 1.07e-6, 4 x 3.748e-7 = 1.50e-6
    'prenet_bwd': (8e-7, 9e-7),    # 4 x 1.861e-7 = 7.44e-7, 4 x 2.245e-7 = 8.98e-7
}


def row_errors(hip, ref):
    """hip, ref: (N, ...) with one row per leading index.  Returns (N,) errors relative to max(|ref_row|, 1e-2 RMS row norm)."""
    h = np.asarray(hip, dtype=np.float64).reshape(len(ref), -1)
    f = np.asarray(ref, dtype=np.float64).reshape(len(ref), -1)
    nr = np.linalg.norm(f, axis=1)
    rms = float(np.sqrt(np.mean(nr ** 2)))
    return np.linalg.norm(h - f, axis=1) / np.maximum(nr, max(1e-2 * rms, 1e-300))


def compare(name, hip, ref, lead):
    """hip, ref: arrays of one shape whose leading dims `lead` (e.g. (B, T)) index the rows.  Returns a dict of the stats."""
    h = np.asarray(hip, dtype=np.float64)
    f = np.asarray(ref, dtype=np.float64)
    assert h.shape == f.shape, (name, h.shape, f.shape)
    n = int(np.prod(lead))
    nref, nhip = float(np.linalg.norm(f)), float(np.linalg.norm(h))
    rel = float(np.linalg.norm(h - f) / max(nref, 1e-300))
    rows = row_errors(h.reshape(n, -1), f.reshape(n, -1))
    i = int(np.argmax(rows))
    return {'name': name, 'rel': rel, 'row': float(rows[i]), 'at': tuple(int(k) for k in np.unravel_index(i, lead)),
            'norm_ref': nref, 'norm_hip': nhip, 'rows': rows.reshape(lead)}


def failures(st, tensor_bar=TENSOR_BAR, row_bar=ROW_BAR):
    """The bars one compare() result misses (empty list: it meets them).  A norm well above zero is part of the bar: a buffer
    the pass never wrote reads as zeros, and a reference that is zero would make any buffer pass."""
    bad = []
    if not st['norm_ref'] > 0 or not st['norm_hip'] >= 0.5 * st['norm_ref']:
        bad.append('%s: norm %.3e against a reference norm of %.3e' % (st['name'], st['norm_hip'], st['norm_ref']))
    if not st['rel'] <= tensor_bar:
        bad.append('%s: tensor rel-L2 %.3e > %.1e' % (st['name'], st['rel'], tensor_bar))
    if not st['row'] <= row_bar:
        bad.append('%s: worst row %.3e > %.1e at %s' % (st['name'], st['row'], row_bar, st['at']))
    return bad


def exact_zero_failures(name, hip, mask):
    """Every element of hip where `mask` (broadcastable) is set must be exactly zero."""
    h = np.asarray(hip)
    m = np.broadcast_to(np.asarray(mask, dtype=bool), h.shape)
    if not m.any():
        return []
    nz = (h != 0) & m
    if nz.any():
        return ['%s: %d of %d exact-zero sites are not zero (max |value| %.3e, first at %s)' %
                (name, int(nz.sum()), int(m.sum()), float(np.abs(h[nz]).max()), tuple(int(k) for k in np.argwhere(nz)[0]))]
    return []
