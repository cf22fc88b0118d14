"""References for the op-level tests of the CBHG tail (tests/cbhg_tail_cases.py): the bi-GRU recurrences, the highway stacks and
the encoder pre-net, each twice.  Host only.

  *_oracle   the fp64 torch oracle's own _gru / _highway / _prenet (oracle/taco_torch.py), driven with leaf tensors and autograd.
             The GRU's x-side projection is folded away: the step is fed x = 0 and the rows of xg as its (per-row) biases, and a
             Recorder keeps the gradients of the gate and candidate pre-activations, which are the rows of dxg.  The highway layers
             get per-row copies of their biases as leaves in the same way (their gradients are the rows of dth), and the adapter
             form is restated as x_l = h_l Wa[:128] + rowb[m // T].
  F32        a plain fp32 torch restatement of each op with the kernels' operand layouts and formulas: the CPU stand-in for the
             kernels (tests/test_cbhg_tail_host.py), optionally with one seeded defect, and the yardstick for what fp32 costs against
             fp64 (tests/test_gpu_cbhg_tail.py prints its error beside the kernels').

Layouts (include/taco_hip.h, the taco_debug_* doors): xg / dxg (B, T, 768) = per direction d at columns [384 d, 384 d + 384) the
pre-activations [r | u | c]; ruc likewise the activations; out / dout / rh (B, T, 256) = [fw | bw]; dh0 (2, B, 128)."""
import numpy as np
import torch

from oracle import taco_torch as ot

H = 128
F64, F32T = torch.float64, torch.float32
DIRS = ('fw', 'bw')

DEFECTS = ('chunk_hprev', 'bw_row_reversed', 'h0_ignored', 'tile_last_row', 'rowb_tile_first', 'relu_factor', 'keep_ignored')


def _t(a, dtype=F64, grad=False):
    return torch.tensor(np.asarray(a), dtype=dtype, requires_grad=grad)


def _g(t):
    """a leaf's (or retained tensor's) gradient as numpy; zeros where nothing flowed"""
    return (torch.zeros_like(t) if t.grad is None else t.grad).detach().numpy().copy()


# ---------------------------------------------------------------------------------------------------------------- bi-GRU
def bigru_oracle(xg, w, h0=None, dout=None):
    """xg (B, T, 768); w: '<fw|bw>/<gates|candidate>/kernel' in TF layout (rows [0, 128), the x side, meet x = 0); h0 (B, 128) or
    None (zeros); dout (B, T, 256) or None -> fp64 dict: out, ruc, rh, and with dout: dxg, dh0 (2, B, 128): the gradient of each
    direction's initial state, which exists whether or not that state is zero."""
    B, T, _ = xg.shape
    xl = _t(xg, grad=True)
    zero_x = torch.zeros(B, H, dtype=F64)
    rec = ot.Recorder(values=True)
    h0s = [_t(np.zeros((B, H)) if h0 is None else h0, grad=True) for _ in DIRS]
    outs = []
    for d, (name, order) in enumerate(zip(DIRS, (range(T), range(T - 1, -1, -1)))):
        wg, wc = _t(w[name + '/gates/kernel']), _t(w[name + '/candidate/kernel'])
        h = h0s[d]
        seq = [None] * T
        for t in order:
            h = ot._gru(zero_x, h, wg, xl[:, t, 384 * d:384 * d + 256], wc, xl[:, t, 384 * d + 256:384 * d + 384], rec,
                        name + '/{}@%d' % t)
            seq[t] = h
        outs.append(torch.stack(seq, 1))
    out = torch.cat(outs, 2)
    r = {'out': out.detach().numpy().copy(), 'ruc': np.zeros((B, T, 768)), 'rh': np.zeros((B, T, 256))}
    for d, name in enumerate(DIRS):
        for t in range(T):
            for i, k in enumerate('ruc'):
                r['ruc'][:, t, 384 * d + H * i:384 * d + H * (i + 1)] = rec.val['%s/%s@%d' % (name, k, t)]
            r['rh'][:, t, H * d:H * (d + 1)] = rec.val['%s/rh@%d' % (name, t)]
    if dout is not None:
        (out * _t(dout)).sum().backward()
        grads = rec.collect()
        r['dxg'] = np.zeros((B, T, 768))
        for d, name in enumerate(DIRS):
            for t in range(T):
                r['dxg'][:, t, 384 * d:384 * d + 256] = grads['%s/gates@%d' % (name, t)]
                r['dxg'][:, t, 384 * d + 256:384 * d + 384] = grads['%s/candidate@%d' % (name, t)]
        assert np.array_equal(r['dxg'], _g(xl)), 'the recorded pre-activation gradients are not the gradient of the xg leaf'
        r['dh0'] = np.stack([_g(h) for h in h0s])
    return r


def bigru_transposes(w):
    """the h-side kernels transposed, in the layout of BiGruBwdWeights: wghT (256, 128) = Wg[128:, :]^T, wchT (128, 128) = Wc[128:, :]^T"""
    wT = {}
    for name in DIRS:
        wT[name + '/wghT'] = np.ascontiguousarray(np.asarray(w[name + '/gates/kernel'])[H:, :].T)
        wT[name + '/wchT'] = np.ascontiguousarray(np.asarray(w[name + '/candidate/kernel'])[H:, :].T)
    return wT


def _visit_times(B, T, d, defect):
    """(T, B) int64: the time index row b visits at step s of direction d's FORWARD recurrence"""
    s = np.arange(T)
    times = np.repeat((s if d == 0 else T - 1 - s)[:, None], B, 1)
    if defect == 'bw_row_reversed' and d == 1:
        times[:, B - 1] = s
    return torch.tensor(times)


# ---------------------------------------------------------------------------------------------------------------- fp32
class F32:
    """The fp32 restatement behind the interface the case runners drive (tests/cbhg_tail_cases.py): numpy fp32 in, numpy fp32 out.
    defect: None, or one of DEFECTS --
      chunk_hprev      h_prev of recurrence step 8 (the first of the second DMA chunk) is the state of two steps back
      bw_row_reversed  the last batch row of the backward direction runs in forward time order
      h0_ignored       the initial state reads as zeros
      tile_last_row    the last row of a partial 32-row tile is not written (highway and pre-net outputs)
      rowb_tile_first  every row of a tile takes the per-sequence bias of the tile's first row
      relu_factor      dH = g T without the [H > 0] factor
      keep_ignored     the pre-net backward ignores keep1"""

    def __init__(self, defect=None):
        assert defect is None or defect in DEFECTS, defect
        self.defect = defect

    # -- bi-GRU
    def bigru_fwd(self, xg, w, h0=None):
        B, T, _ = xg.shape
        x = _t(xg, F32T)
        out, ruc = torch.zeros(B, T, 256), torch.zeros(B, T, 768)
        ar = torch.arange(B)
        for d, name in enumerate(DIRS):
            wgh, wch = _t(w[name + '/gates/kernel'], F32T)[H:], _t(w[name + '/candidate/kernel'], F32T)[H:]
            times = _visit_times(B, T, d, self.defect)
            h = torch.zeros(B, H) if (h0 is None or self.defect == 'h0_ignored') else _t(h0, F32T)
            before = h
            for s in range(T):
                t = times[s]
                hp = before if (self.defect == 'chunk_hprev' and s == 8) else h
                xs = x[ar, t, 384 * d:384 * d + 384]
                g = torch.sigmoid(xs[:, :256] + hp @ wgh)
                r, u = g[:, :H], g[:, H:]
                c = torch.tanh(xs[:, 256:] + (r * hp) @ wch)
                before = h
                h = u * hp + (1 - u) * c
                out[ar, t, H * d:H * (d + 1)] = h
                ruc[ar, t, 384 * d:384 * d + 384] = torch.cat([r, u, c], 1)
        return out.numpy(), ruc.numpy()

    def bigru_bwd(self, dout, out, ruc, wT, h0=None, want_dh0=False):
        """the formulas of bigru_bwd_kernel (csrc/bigru.hip), a batch at a time"""
        B, T, _ = dout.shape
        dout, out, ruc = _t(dout, F32T), _t(out, F32T), _t(ruc, F32T)
        dxg, rh, dh0 = torch.zeros(B, T, 768), torch.zeros(B, T, 256), torch.zeros(2, B, H)
        ar = torch.arange(B)
        for d, name in enumerate(DIRS):
            wghT, wchT = _t(wT[name + '/wghT'], F32T), _t(wT[name + '/wchT'], F32T)
            times = _visit_times(B, T, d, self.defect)
            first = torch.zeros(B, H) if (h0 is None or self.defect == 'h0_ignored') else _t(h0, F32T)
            dh = torch.zeros(B, H)
            for s in range(T - 1, -1, -1):
                t = times[s]
                back = 2 if (self.defect == 'chunk_hprev' and T - 1 - s == 8 and s >= 2) else 1
                hp = out[ar, times[s - back], H * d:H * (d + 1)] if s >= back else first
                v = ruc[ar, t, 384 * d:384 * d + 384]
                r, u, c = v[:, :H], v[:, H:2 * H], v[:, 2 * H:]
                dht = dh + dout[ar, t, H * d:H * (d + 1)]
                du = dht * (hp - c)
                dcp = dht * (1 - u) * (1 - c * c)
                dup = du * u * (1 - u)
                drh = dcp @ wchT
                drp = drh * hp * r * (1 - r)
                dh = dht * u + drh * r + torch.cat([drp, dup], 1) @ wghT
                dxg[ar, t, 384 * d:384 * d + 384] = torch.cat([drp, dup, dcp], 1)
                rh[ar, t, H * d:H * (d + 1)] = r * hp
            dh0[d] = dh
        return dxg.numpy(), rh.numpy(), (dh0.numpy() if want_dh0 else None)

    # -- highway stack
    def _drop(self, M, *arrays):
        if self.defect == 'tile_last_row' and M % 32:
            for a in arrays:
                a[M - 1] = np.nan
        return arrays

    def highway_fwd(self, x, p, nl, T=None):
        """p: lists wt, bt, wh, bh (and wa, rowb with T: the adapter form) -> dict y, th, hx (lists; hx None in the plain form)"""
        M = x.shape[0]
        h = _t(x, F32T)
        ad = 'wa' in p
        m = torch.arange(M)
        seq = ((m // 32 * 32) if self.defect == 'rowb_tile_first' else m) // T if ad else None
        y, th, hx = [], [], []
        for l in range(nl):
            if ad:
                h = h @ _t(p['wa'][l], F32T) + _t(p['rowb'][l], F32T)[seq]
                hx.append(h.numpy().copy())
            Tg = torch.sigmoid(h @ _t(p['wt'][l], F32T) + _t(p['bt'][l], F32T))
            Hh = torch.relu(h @ _t(p['wh'][l], F32T) + _t(p['bh'][l], F32T))
            h = Hh * Tg + h * (1 - Tg)
            th.append(torch.cat([Tg, Hh], 1).numpy().copy())
            y.append(h.numpy().copy())
        self._drop(M, *(y + th + hx))
        return {'y': y, 'th': th, 'hx': hx if ad else None}

    def highway_bwd(self, g, wT, th, x, waT=None):
        """wT[l] (256, 128) = [Wt^T ; Wh^T], th / x the forward stash (x[l]: the input of layer l's gates) -> dict dth, gout, dhx"""
        nl, M = len(th), g.shape[0]
        g = _t(g, F32T)
        dth, dhx = [None] * nl, [None] * nl
        for l in range(nl - 1, -1, -1):
            s, xl = _t(th[l], F32T), _t(x[l], F32T)
            Tg, Hh = s[:, :H], s[:, H:]
            dt = g * (Hh - xl) * Tg * (1 - Tg)
            dh = g * Tg if self.defect == 'relu_factor' else torch.where(Hh > 0, g * Tg, torch.zeros_like(g))
            dth[l] = torch.cat([dt, dh], 1).numpy().copy()
            g = torch.cat([dt, dh], 1) @ _t(wT[l], F32T) + g * (1 - Tg)
            if waT is not None:
                dhx[l] = g.numpy().copy()
                g = g @ _t(waT[l], F32T)
        gout = g.numpy().copy()
        self._drop(M, gout, *(dth + (dhx if waT is not None else [])))
        return {'dth': dth, 'gout': gout, 'dhx': dhx if waT is not None else None}

    # -- pre-net
    def prenet_fwd(self, x, p, k1=None, k2=None):
        M = x.shape[0]
        y1 = torch.relu(_t(x, F32T) @ _t(p['w1'], F32T) + _t(p['b1'], F32T))
        if k1 is not None:
            y1 = y1 * (2.0 * _t(k1, F32T))
        y2 = torch.relu(y1 @ _t(p['w2'], F32T) + _t(p['b2'], F32T))
        if k2 is not None:
            y2 = y2 * (2.0 * _t(k2, F32T))
        return self._drop(M, y1.numpy().copy(), y2.numpy().copy())

    def prenet_bwd(self, dy2, w2T, w1T, y1, y2, k1=None, k2=None):
        M = dy2.shape[0]
        y1, y2 = _t(y1, F32T), _t(y2, F32T)
        if self.defect == 'keep_ignored':
            k1 = None
        on2 = (y2 > 0) if k2 is None else (y2 > 0) & (_t(k2, F32T) > 0)
        dz2 = torch.where(on2, _t(dy2, F32T) * (1.0 if k2 is None else 2.0), torch.zeros_like(y2))
        on1 = (y1 > 0) if k1 is None else (y1 > 0) & (_t(k1, F32T) > 0)
        dz1 = torch.where(on1, (dz2 @ _t(w2T, F32T)) * (1.0 if k1 is None else 2.0), torch.zeros_like(y1))
        dx = dz1 @ _t(w1T, F32T)
        return self._drop(M, dz2.numpy().copy(), dz1.numpy().copy(), dx.numpy().copy())


# ---------------------------------------------------------------------------------------------------------------- highway
def highway_oracle(x, p, nl, T=None, g=None, force=None):
    """The fp64 oracle's _highway, nl layers.  p: lists wt, bt, wh, bh (and wa, rowb with T: x_l = h_l wa[l] + rowb[l][m // T]).
    force: None (the oracle's own ReLU decisions, recorded) or a list of (M, 128) 0 / 1 arrays imposed on the H sites.
    -> dict: y, th, hx (lists), dec (the Decisions), and with g (M, 128): dth, dhx (lists), gout."""
    M = x.shape[0]
    ad = 'wa' in p
    dec = ot.Decisions(None if force is None else {'hw%d/H' % l: _t(np.asarray(force[l], dtype=np.float64)) for l in range(nl)})
    x0 = _t(x, grad=True)
    h = x0
    seq = torch.arange(M) // T if ad else None
    r = {'y': [], 'th': [], 'hx': [], 'dec': dec}
    leaves = []
    for l in range(nl):
        if ad:
            h = h @ _t(p['wa'][l]) + _t(p['rowb'][l])[seq]
            h.retain_grad()
            r['hx'].append(h.detach().numpy().copy())
        bt = _t(np.broadcast_to(np.asarray(p['bt'][l], dtype=np.float64), (M, H)).copy(), grad=True)
        bh = _t(np.broadcast_to(np.asarray(p['bh'][l], dtype=np.float64), (M, H)).copy(), grad=True)
        pre = 'hw%d/' % l
        rec = ot.Recorder(values=True)
        leaves.append((bt, bh, h))
        h = ot._highway(h, {pre + 'T/kernel': _t(p['wt'][l]), pre + 'T/bias': bt, pre + 'H/kernel': _t(p['wh'][l]), pre + 'H/bias': bh},
                        pre, dec, rec)
        r['th'].append(np.concatenate([rec.val[pre + 'T'], rec.val[pre + 'H']], 1))
        r['y'].append(rec.val[pre + 'out'])
    if not ad:
        r['hx'] = None
    if g is not None:
        (h * _t(g)).sum().backward()
        r['dth'] = [np.concatenate([_g(bt), _g(bh)], 1) for bt, bh, _ in leaves]
        r['dhx'] = [_g(xl) for _, _, xl in leaves] if ad else None
        r['gout'] = _g(x0)
    return r


def highway_decisions(th):
    """the H sites' ReLU decisions as a stash th (list of (M, 256) [T | H]) shows them, in the oracle's site names"""
    return {'hw%d/H' % l: np.asarray(s)[:, H:] > 0 for l, s in enumerate(th)}


# ---------------------------------------------------------------------------------------------------------------- pre-net
def prenet_oracle(x, p, k1=None, k2=None, dy2=None, force=None):
    """The fp64 oracle's _prenet.  p: w1 (256, 256), b1, w2 (256, 128), b2; k1 / k2 0 / 1 keep masks or None; force: None or
    {'pn/l1': (M, 256), 'pn/l2': (M, 128)} 0 / 1.  -> dict y1, y2, dec, and with dy2: dz2, dz1 (pre-activation gradients), dx."""
    dec = ot.Decisions(None if force is None else {k: _t(np.asarray(v, dtype=np.float64)) for k, v in force.items()})
    rec = ot.Recorder(values=True)
    xl = _t(x, grad=True)
    P = {'pn/dense/kernel': _t(p['w1']), 'pn/dense/bias': _t(p['b1']), 'pn/dense_1/kernel': _t(p['w2']), 'pn/dense_1/bias': _t(p['b2'])}
    y2 = ot._prenet(xl, P, 'pn/', None if k1 is None else _t(k1), None if k2 is None else _t(k2), dec, rec=rec)
    r = {'y1': rec.val['pn/l1'], 'y2': rec.val['pn/l2'], 'dec': dec}
    if dy2 is not None:
        (y2 * _t(dy2)).sum().backward()
        grads = rec.collect()
        r['dz1'], r['dz2'], r['dx'] = grads['pn/l1pre'], grads['pn/l2pre'], _g(xl)
    return r


def prenet_decisions(y1, y2, k1=None, k2=None):
    """-> (decisions, observable): a unit dropped by dropout reads 0 whatever its ReLU decided"""
    d = {'pn/l1': np.asarray(y1) > 0, 'pn/l2': np.asarray(y2) > 0}
    ok = {}
    if k1 is not None:
        ok['pn/l1'] = np.asarray(k1) > 0
    if k2 is not None:
        ok['pn/l2'] = np.asarray(k2) > 0
    return d, ok
