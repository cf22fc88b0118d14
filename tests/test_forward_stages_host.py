"""CPU: the forward stage comparison (tests/forward_map.py, bars in tests/stage_bars.py) must be able to fail.  The fp64
oracle's own recorded values, rounded to fp32 and assembled into stash / CBHG / attention-memory arrays with the map the GPU test
uses, pass every check: the reference alone stays inside the bars.  Then single-site corruptions of the kinds a decoder or
post-net kernel gets wrong -- one (b, t) record, one fed row, one 32-row tile edge -- are each reported at the buffer and the row
where they were planted, and nowhere else."""
import numpy as np
import pytest

from oracle import taco_numpy as on
from tests import forward_map as fm
from tests.decisions import K_ST_H, K_ST_P1, K_ST_P2, K_ST_R, K_ST_REC, K_ST_RH
from tests.stage_bars import FWD_ROW_BAR, FWD_TENSOR_BAR, ROW_BAR, compare
from tests.util import small_case

R_, V_, B_, TT_, TD_ = 5, 24, 3, 13, 8   # the post-net runs over Td r = 40 frames per row: one 32-row tile edge inside a row


@pytest.fixture(scope='module')
def case():
    p = on.init_params(V_, R_, seed=6, perturb=0.2)
    inp, masks = small_case(r=R_, V=V_, B=B_, Tt=TT_, Td=TD_, seed=21)
    assert not fm.mask_coverage_failures(masks, B_, TD_)
    V64, _ = fm.oracle_forward(p, inp, masks, R_, TD_, True)
    ref = fm.build_reference(V64, p, inp, B_, TT_, TD_, R_)
    bufs = fm.assemble(ref)
    fed = fm.fed_steps(masks, B_, TD_)
    prein = np.ascontiguousarray(inp['mel'][:, :, 80 * (R_ - 1):]).astype(np.float32)
    prein[:, 1:][fed[:, 1:]] = bufs['seq2seq_output'][:, :-1, 80 * (R_ - 1):][fed[:, 1:]]
    bufs['dec.prein'] = prein
    return p, inp, masks, ref, bufs, fed


def _check(case, bufs):
    p, inp, masks, ref, _, _ = case
    return fm.check_forward(bufs, ref, inp, masks, B_, TT_, TD_, R_)


def _corrupt(case, name):
    bufs = dict(case[4])
    bufs[name] = bufs[name].copy()
    return bufs, bufs[name]


def _expect(bad, names, at):
    """Every failure names one of `names`; one of them carries the planted row."""
    assert bad, 'the corruption was not reported'
    for msg in bad:
        assert msg.split(':')[0].split(' (')[0] in names, bad
    assert any(('at %s' % (at,)) in msg for msg in bad), (bad, at)


def _stat(res, name):
    return next(st for st in res if st['name'] == name)


def _show(what, st):
    print('  %-40s %-10s tensor rel-L2 %.2e (bar %.0e), worst row %.2e at %s (bar %.0e)' %
          (what, st['name'], st['rel'], FWD_TENSOR_BAR, st['row'], st['at'], FWD_ROW_BAR))


def test_the_bars_keep_their_caps():
    assert 0 < FWD_TENSOR_BAR <= 3e-5 and 0 < FWD_ROW_BAR <= ROW_BAR


def test_the_stash_map_tiles_the_record(monkeypatch):
    assert not fm.stash_tiling_failures(K_ST_REC)
    assert fm.stash_tiling_failures(K_ST_REC + 256)   # (a field added to the record behind the map's back)
    monkeypatch.setattr(fm, 'STASH_FIELDS', [f for f in fm.STASH_FIELDS if f[0] != 'U1'])
    assert any('not covered' in m for m in fm.stash_tiling_failures(K_ST_REC))


def test_the_reference_rounded_to_fp32_passes(case):
    res, bad = _check(case, case[4])
    w, wr = fm.print_table('oracle as fp32', res)
    assert not bad, bad
    assert len(res) > 60 and w['rel'] < 1e-7 and wr['row'] < 1e-6   # (fp32 rounding alone: 6e-8 per element)


def test_h_of_the_previous_step(case):
    b, t = 1, 4
    bufs, st = _corrupt(case, 'dec.stash')
    st[b, t, K_ST_H + 256:K_ST_H + 512] = st[b, t - 1, K_ST_H + 256:K_ST_H + 512]
    res, bad = _check(case, bufs)
    _show("H1 of (1, 4) holds step 3's state", _stat(res, 'stash.H1'))
    _expect(bad, {'stash.H1'}, (b, t))


def test_rh_formed_with_the_new_state(case):
    b, t, l = 2, 5, 0
    bufs, st = _corrupt(case, 'dec.stash')
    o = 256 * l
    st[b, t, K_ST_RH + o:K_ST_RH + o + 256] = st[b, t, K_ST_R + o:K_ST_R + o + 256] * st[b, t, K_ST_H + o:K_ST_H + o + 256]
    res, bad = _check(case, bufs)
    _show('RH0 of (2, 5) = r * h_new', _stat(res, 'stash.RH0'))
    _expect(bad, {'stash.RH0'}, (b, t))


def test_fed_row_holds_the_teacher_forced_pre_net(case):
    p, inp, masks, _, _, fed = case
    b, t = [int(i) for i in np.argwhere(fed)[len(np.argwhere(fed)) // 2]]
    x = inp['mel'][b, t, 80 * (R_ - 1):].astype(np.float64)
    pf = 'decoder/pre_net/'
    l1 = np.maximum(x @ p[pf + 'dense/kernel'] + p[pf + 'dense/bias'], 0) * 2 * masks['dec_keep1'][b, t]
    l2 = np.maximum(l1 @ p[pf + 'dense_1/kernel'] + p[pf + 'dense_1/bias'], 0) * 2 * masks['dec_keep2'][b, t]
    bufs, st = _corrupt(case, 'dec.stash')
    st[b, t, K_ST_P1:K_ST_P1 + 256] = l1
    st[b, t, K_ST_P2:K_ST_P2 + 128] = l2
    res, bad = _check(case, bufs)
    _show('P1 of a fed row from the mel frame', _stat(res, 'stash.P1'))
    _show('P2 of a fed row from the mel frame', _stat(res, 'stash.P2'))
    _expect([m for m in bad if m.startswith('stash.P1')], {'stash.P1'}, (b, t))
    _expect([m for m in bad if m.startswith('stash.P2')], {'stash.P2'}, (b, t))
    assert all(m.startswith(('stash.P1', 'stash.P2')) for m in bad), bad


def test_prein_of_a_fed_step_holds_the_mel_frame(case):
    p, inp, masks, _, _, fed = case
    b, t = [int(i) for i in np.argwhere(fed)[-1]]
    bufs, pr = _corrupt(case, 'dec.prein')
    pr[b, t] = inp['mel'][b, t, 80 * (R_ - 1):]
    _, bad = _check(case, bufs)
    assert len(bad) == 1
    _expect(bad, {'dec.prein'}, (b, t))


@pytest.mark.parametrize('name', ['post.h2', 'post.out', 'post.pool'])
def test_post_net_frames_swapped_at_a_tile_edge(case, name):
    b = 1
    bufs, x = _corrupt(case, name)
    x[b, [31, 32]] = x[b, [32, 31]]
    res, bad = _check(case, bufs)
    st = _stat(res, name)
    assert st['at'] in ((b, 31), (b, 32)) and sorted(np.argsort(st['rows'].ravel())[-2:]) == [b * TD_ * R_ + 31, b * TD_ * R_ + 32]
    _expect(bad, {name}, st['at'])


def test_ruc_row_with_u_and_c_exchanged(case):
    b, t = 0, 17
    bufs, x = _corrupt(case, 'post.ruc')
    x[b, t, 128:384] = np.concatenate([x[b, t, 256:384], x[b, t, 128:256]])
    _, bad = _check(case, bufs)
    _expect(bad, {'post.ruc'}, (b, t))


def test_values_row_past_text_length_is_not_zero(case):
    p, inp, masks, ref, _, _ = case
    b = int(np.argmin(inp['text_length']))
    s = int(inp['text_length'][b])
    assert s < TT_
    bufs, x = _corrupt(case, 'dec.values')
    x[b, s, 3] = 1e-30
    res, bad = _check(case, bufs)
    assert len(bad) == 1 and bad[0].startswith('dec.values (past text_length)') and 'at (%d, %d, 3)' % (b, s) in bad[0], bad
    st = compare('dec.values', x, ref['dec.values'][0], (B_, TT_))
    assert st['rel'] <= FWD_TENSOR_BAR and st['row'] <= FWD_ROW_BAR   # (which no tolerance would have seen)


def test_an_unwritten_row_fails(case):
    """A row the pass never wrote still holds the poison: reported at that buffer (NaN meets no bar)."""
    bufs, x = _corrupt(case, 'enc.th2')
    x[2, 7] = np.nan
    _, bad = _check(case, bufs)
    assert bad and all(m.startswith('enc.th2') for m in bad), bad
    bufs, st = _corrupt(case, 'dec.stash')
    st[0, 0, fm.STASH_UNWRITTEN[0][1]] = 0.0   # ... and a write into a slot the map calls unwritten is reported too
    _, bad = _check(case, bufs)
    assert len(bad) == 1 and bad[0].startswith('stash.Ctx'), bad
