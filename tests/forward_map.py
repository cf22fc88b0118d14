"""The forward pass's buffer map: which value of the fp64 oracle (oracle.taco_torch.Recorder(values=True)) every workspace
buffer of taco_forward / taco_infer holds, and the checks on it.  Shared by tests/test_gpu_forward_stages.py (the HIP path's
buffers) and tests/test_forward_stages_host.py (the oracle's own values rounded to fp32, then corrupted on purpose); the map
itself is described in the former's docstring."""
import numpy as np
import torch

from oracle import taco_torch as ot
from tests.decisions import (K_ST_ATT, K_ST_C, K_ST_CTX, K_ST_H, K_ST_P1, K_ST_P2, K_ST_Q, K_ST_R, K_ST_REC, K_ST_RH, K_ST_U,
                             K_ST_X, K_ST_Y)
from tests.stage_bars import FWD_ROW_BAR, FWD_TENSOR_BAR, compare, exact_zero_failures, failures

# dec.stash, one (b, t) record: (field, offset, width); the per-layer fields are compared layer by layer
STASH_FIELDS = ([('P1', K_ST_P1, 256), ('P2', K_ST_P2, 128), ('X', K_ST_X, 256)] +
                [('%s%d' % (n, l), o + 256 * l, 256) for n, o in (('H', K_ST_H), ('R', K_ST_R), ('U', K_ST_U), ('C', K_ST_C),
                                                                 ('RH', K_ST_RH)) for l in range(3)] +
                [('Q', K_ST_Q, 256), ('Y', K_ST_Y, 256)])
STASH_UNWRITTEN = [('Ctx', K_ST_CTX, 256), ('Att', K_ST_ATT, 256)]   # neither decoder kernel writes these slots
# oracle site of each stash field ('decoder/' + site + '@t')
_STASH_SITE = {'P1': 'pre_net/l1', 'P2': 'pre_net/l2', 'X': 'x', 'Q': 'q', 'Y': 'y'}
_STASH_SITE.update({'%s%d' % (n, l): 'gru_%d/%s' % (l, s) for n, s in (('H', 'h'), ('R', 'r'), ('U', 'u'), ('C', 'c'), ('RH', 'rh'))
                    for l in range(3)})
# forward-pass workspace tensors the map leaves out, and why (anything else under enc. / dec. / post. must be compared)
NOT_COMPARED = {'xg': 'scratch of the bi-GRU (x-side projections)', 'rowb': 'per-sequence adapter bias, enters hx',
                'dec.xchg': 'exchange area', 'dec.err': 'error words', 'post.wd_pad': 're-pitched parameter copy',
                'enc.dspk_e': 'backward', 'dh0': 'backward', 'dsmall': 'backward', 'dsmall2': 'backward', 'dsm': 'backward',
                'dsm2': 'backward', 'dspk_part': 'backward'}
# written only when a backward pass will read them (model.hip cbhg_fwd keep_ruc): not part of the inference map
TRAIN_ONLY = ('bank', 'th0', 'th1', 'th2', 'th3', 'ruc')


def stash_tiling_failures(record_width):
    """The compared fields and the unwritten slots tile [0, kStRec) exactly, and kStRec is the workspace table's record width."""
    bad, at = [], 0
    for name, off, w in sorted(STASH_FIELDS + STASH_UNWRITTEN, key=lambda f: f[1]):
        if off != at:
            bad.append('dec.stash map: [%d, %d) in front of %s is %s' % (min(at, off), max(at, off), name,
                                                                       'not covered' if off > at else 'covered twice'))
        at = off + w
    if at != K_ST_REC or record_width != K_ST_REC:
        bad.append('dec.stash map ends at %d, K_ST_REC = %d, the workspace table has %d floats per record' % (at, K_ST_REC, record_width))
    return bad


def oracle_forward(p, inp, masks, r, Td, train=True):
    """One fp64 forward under no_grad with the value recorder and the decisions recorded.  Returns (values, Decisions)."""
    rec, dec = ot.Recorder(values=True), ot.Decisions()
    with torch.no_grad():
        pt = ot.to_torch(p, torch.float64)
        ti = {'text': torch.tensor(np.asarray(inp['text']), dtype=torch.int64),
              'text_length': torch.tensor(np.asarray(inp['text_length']), dtype=torch.int64)}
        if train:
            ti['mel'] = torch.tensor(np.asarray(inp['mel']), dtype=torch.float64)
        if 'speaker' in inp:
            ti['speaker'] = torch.tensor(np.asarray(inp['speaker']), dtype=torch.int64)
        tm = {k: torch.tensor(np.asarray(v), dtype=torch.float64) for k, v in (masks or {}).items()}
        ot.forward(pt, ti, r, Td, train, tm, dec, rec)
    return rec.val, dec


def _steps(V, site, Td):
    return np.stack([V['decoder/%s@%d' % (site, t)] for t in range(Td)], 1)


def wx_c(p, r):
    """Wx_c = Wa[80r:] Wi[128:] (layout.hip: the context's path into the input projection), fp64."""
    return p['decoder/attention_layer/kernel'][80 * r:].astype(np.float64) @ p['decoder/in_proj/kernel'][128:].astype(np.float64)


def build_reference(V, p, inp, B, Tt, Td, r, S=1, train=True):
    """name -> (fp64 reference with its row-indexing dims in front, those dims).  Names are the workspace table's, plus
    'seq2seq_output', 'output' and 'alignments'; 'dec.stash' is one (B, Td, kStRec) array with NaN in the unwritten slots."""
    ref = {}
    L = np.asarray(inp['text_length'])
    ref['enc.emb'] = (V['encoder/emb'], (B, Tt))
    ref['enc.p1'] = (V['encoder/pre_net/l1'], (B, Tt))
    ref['enc.p2'] = (V['encoder/pre_net/l2'], (B, Tt))
    for pre, prefix, T in (('enc.', 'encoder/cbhg/', Tt), ('post.', 'post/cbhg/', Td * r)):
        spk = pre == 'enc.' and S > 1
        for buf, site in (('bank', 'bank'), ('pool', 'pool'), ('pj1pre', 'proj1act'), ('pj1', 'proj1'), ('pj2pre', 'proj2pre'),
                          ('res', 'res'), ('out', 'out')):
            ref[pre + buf] = (V[prefix + site], (B, T))
        for l in range(4):
            hp = prefix + 'highway_%d/' % l
            ref['%sh%d' % (pre, l + 1)] = (V[hp + 'out'], (B, T))
            ref['%sth%d' % (pre, l)] = (np.concatenate([V[hp + 'T'], V[hp + 'H']], 2), (B, T))
            if spk or (pre == 'post.' and l == 0):   # layers with an input adapter (layout.hip ws_cbhg: hx = h elsewhere)
                ref['%shx%d' % (pre, l)] = (V[hp + 'in'], (B, T))
        ref[pre + 'ruc'] = (np.concatenate([V[prefix + 'bigru/%s/%s' % (d, k)] for d in ('fw', 'bw') for k in 'ruc'], 2), (B, T))
        if spk:
            ref['enc.spk_e'] = (V['speaker_embed'], (B,))
            ref['enc.sv_h0'] = (np.stack([V[prefix + 'highway_%d/spk' % l] for l in range(4)] + [V[prefix + 'gru_init']]), (5, B))
        if not train:
            for buf in TRAIN_ONLY:
                del ref[pre + buf]
    values = V['decoder/values']
    ref['dec.values'] = (values, (B, Tt))
    ref['dec.keys'] = (V['decoder/keys'], (B, Tt))
    wxc = wx_c(p, r)
    ref['dec.vwx'] = (values @ wxc, (B, Tt))
    ref['dec.vwg'] = (values @ (wxc @ p['decoder/gru_0/gates/kernel'][:256].astype(np.float64)), (B, Tt))
    if train:
        valid = (np.arange(Tt)[None, :] < L[:, None])[:, :, None]
        vcen = (values - values.sum(1, keepdims=True) / np.maximum(L, 1)[:, None, None]) * valid   # (values past L are 0)
        ref['dec.vcen'] = (vcen, (B, Tt))
        ref['dec.vwxc'] = (vcen @ wxc, (B, Tt))
        st = np.full((B, Td, K_ST_REC), np.nan)
        for name, off, w in STASH_FIELDS:
            st[:, :, off:off + w] = _steps(V, _STASH_SITE[name], Td)
        ref['dec.stash'] = (st, (B, Td))
    ref['seq2seq_output'] = (_steps(V, 'o', Td), (B, Td))
    ref['output'] = (V['output'], (B, Td))
    ref['alignments'] = (_steps(V, 'alignments', Td), (B, Td))
    return ref


def fed_steps(masks, B, Td):
    """(B, Td) bool: step t of row b was fed the previous step's output (sample[t - 1, b]); step 0 never is."""
    fed = np.zeros((B, Td), bool)
    fed[:, 1:] = (np.asarray(masks['sample']) > 0)[:Td - 1].T
    return fed


def mask_coverage_failures(masks, B, Td):
    """Every training case holds a fed step, a teacher-forced step (past step 0) and a row whose step t is fed and t + 1 is not."""
    fed = fed_steps(masks, B, Td)
    bad = []
    if not fed[:, 1:].any():
        bad.append('no fed step')
    if fed[:, 1:].all():
        bad.append('no teacher-forced step past step 0')
    if not (fed[:, 1:-1] & ~fed[:, 2:]).any():
        bad.append('no row whose step t is fed and whose step t + 1 is teacher-forced')
    return bad


def assemble(ref):
    """What a faultless fp32 implementation would leave in its buffers: the reference rounded to fp32, one array per name."""
    return {k: v.astype(np.float32) for k, (v, _) in ref.items()}


def _bit_rows(name, got, want, lead):
    """got must equal want bit for bit; reports the first differing row."""
    g = np.ascontiguousarray(got, np.float32).reshape(int(np.prod(lead)), -1).view(np.uint32)
    w = np.ascontiguousarray(want, np.float32).reshape(int(np.prod(lead)), -1).view(np.uint32)
    rows = np.nonzero((g != w).any(1))[0]
    if len(rows):
        return ['%s: %d of %d rows are not bit-identical, first at %s' % (name, len(rows), len(g),
                                                                         tuple(int(k) for k in np.unravel_index(rows[0], lead)))]
    return []


def check_forward(bufs, ref, inp, masks, B, Tt, Td, r, train=True):
    """bufs: name -> array (any shape of the right size) for every name of `ref`, plus 'dec.prein' when training.  Returns
    (compare() results, failures): every mapped buffer as a whole tensor and per row against the forward bars, dec.stash field
    by field, and the exact checks (zeros, poison left in the unwritten slots, bit-identical rows), which carry no tolerance."""
    res, bad = [], []
    L = np.asarray(inp['text_length'])
    past = (np.arange(Tt)[None, :] >= L[:, None])[:, :, None]

    def cmp(name, got, want, lead):
        st = compare(name, got, want, lead)
        res.append(st)
        bad.extend(failures(st, FWD_TENSOR_BAR, FWD_ROW_BAR))
        return st

    got = {}
    for name, (want, lead) in ref.items():
        if name not in bufs:
            bad.append('%s: not among the buffers' % name)
            continue
        got[name] = np.asarray(bufs[name]).reshape(want.shape)
        if name == 'dec.stash':
            continue
        if name == 'enc.emb':
            bad += _bit_rows(name, got[name], want.astype(np.float32), lead)
        cmp(name, got[name], want, lead)
    if 'dec.stash' in got:
        st_hip, st_ref = got['dec.stash'], ref['dec.stash'][0]
        for name, off, w in STASH_FIELDS:
            st = cmp('stash.' + name, st_hip[:, :, off:off + w], st_ref[:, :, off:off + w], (B, Td))
            wt, wb = st['rows'].max(0), st['rows'].max(1)
            st['note'] = 'worst step %d (%.2e), worst batch row %d (%.2e)' % (int(np.argmax(wt)), np.max(wt), int(np.argmax(wb)),
                                                                             np.max(wb))
        for name, off, w in STASH_UNWRITTEN:
            if not np.isnan(st_hip[:, :, off:off + w]).all():
                bad.append('stash.%s: the slot no kernel writes no longer holds the poison' % name)
        k1, k2 = np.asarray(masks['dec_keep1']) > 0, np.asarray(masks['dec_keep2']) > 0
        bad += exact_zero_failures('stash.P1 (unit dropped)', st_hip[:, :, K_ST_P1:K_ST_P1 + 256], ~k1)
        bad += exact_zero_failures('stash.P2 (unit dropped)', st_hip[:, :, K_ST_P2:K_ST_P2 + 128], ~k2)
    if train:
        # dec.prein: the pre-net input frame each step actually used, bit for bit
        if 'dec.prein' not in bufs or 'seq2seq_output' not in got:
            bad.append('dec.prein: not among the buffers')
        else:
            fed = fed_steps(masks, B, Td)
            want = np.ascontiguousarray(np.asarray(inp['mel'], np.float32)[:, :, 80 * (r - 1):])
            prev = got['seq2seq_output'].astype(np.float32)[:, :-1, 80 * (r - 1):]
            want[:, 1:][fed[:, 1:]] = prev[fed[:, 1:]]
            bad += _bit_rows('dec.prein', np.asarray(bufs['dec.prein']).reshape(B, Td, 80), want, (B, Td))
        for name, keep in (('enc.p1', 'enc_keep1'), ('enc.p2', 'enc_keep2')):
            if name in got:
                bad += exact_zero_failures('%s (unit dropped)' % name, got[name], np.asarray(masks[keep]) == 0)
    for name in ('dec.values', 'dec.keys', 'dec.vcen', 'dec.vwxc'):
        if name in got:
            bad += exact_zero_failures('%s (past text_length)' % name, got[name], past)
    if 'alignments' in got:
        bad += exact_zero_failures('alignments (past text_length)', got['alignments'], past[:, None, :, 0])
    return res, bad


def print_table(tag, res, extra=''):
    print('  %-24s %10s %10s  %-12s %s' % (tag, 'rel-L2', 'worst row', 'at', ''))
    for st in res:
        print('  %-24s %10.3e %10.3e  %-12s %s' % (st['name'], st['rel'], st['row'], st['at'], st.get('note', '')))
    w = max(res, key=lambda s: s['rel'] if s['rel'] == s['rel'] else np.inf)
    wr = max(res, key=lambda s: s['row'] if s['row'] == s['row'] else np.inf)
    print('  FWD-STAGES %s: worst tensor %.3e (%s), worst row %.3e (%s at %s)%s' %
          (tag, w['rel'], w['name'], wr['row'], wr['name'], wr['at'], extra))
    return w, wr
