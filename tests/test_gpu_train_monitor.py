"""The training monitor on the GPU: Tacotron.step(monitor=True) and train(..., monitor=True) (lib.tensor_stats underneath).

Part one, a small r = 2 model under TACO_DETERMINISTIC=1: the activation rows of monitor_result equal the NumPy restatement
(tests/monitor_ref.py) applied to the workspace rows and output tensors of a second, identical model copied out between its forward
and its backward pass; the parameter, gradient and Adam rows equal the restatement on copies of the flat buffers after the step;
monitor=False leaves bit-identical parameters after the same steps; a NaN planted in one parameter's gradient is reported under
exactly that name.  Part two: the driver for 4 steps with log_every = 2 writes two monitor_<step>.npz, prints the extra lines and
walks through the same losses and parameters as the run without the flag."""
import os
import re

import numpy as np
import pytest
import torch

from tests import monitor_ref as mr
from tests.util import small_case

pytestmark = pytest.mark.gpu

B, TT, TD, R, V = 3, 9, 8, 2, 20


def bits64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _model(seed=0):
    from tacotron_amd.config import Config
    from tacotron_amd.model import Tacotron
    c = Config()
    c.r, c.vocab_size, c.max_decode_iter = R, V, TD
    inp, masks = small_case(r=R, V=V, B=B, Tt=TT, Td=TD, seed=3)
    m = Tacotron(c, {k: torch.as_tensor(v) for k, v in inp.items()}, train=True, seed=seed)
    return m, {k: torch.as_tensor(v).cuda() for k, v in masks.items()}


def _rows_match(res, names, sites, bufs, label):
    """the rows of `sites` (buffer -> [(name, offset, size)]) in the host result against the restatement on the host copies `bufs`"""
    counts, moments, hist = res
    row = {n: i for i, n in enumerate(names)}
    for buf, segs in sites.items():
        rc, rm, rh = mr.stats_many(bufs[buf], [(o, s) for _, o, s in segs])
        idx = [row[n] for n, _, _ in segs]
        assert np.array_equal(counts[idx], rc), (label, buf)
        assert np.array_equal(hist[idx], rh), (label, buf)
        assert np.array_equal(bits64(moments[idx][:, 2:]), bits64(rm[:, 2:])), (label, buf)
        for k, (n, o, s) in enumerate(segs):
            bound = mr.sum_bounds(bufs[buf][o:o + s])
            for j in (0, 1):
                assert abs(moments[idx[k], j] - rm[k, j]) <= bound[j], (label, n, mr.MOMENTS[j], moments[idx[k], j], rm[k, j], bound[j])


def test_step_with_monitor_reads_the_sites_at_the_right_moments(built_lib, monkeypatch):
    from tacotron_amd import model as model_module
    monkeypatch.setenv('TACO_DETERMINISTIC', '1')
    a, masks = _model()
    assert a.monitor_result is None
    a.step(1e-3, masks=masks, monitor=True)
    torch.cuda.synchronize()
    a.check()
    res = tuple(t.cpu().numpy() for t in a.monitor_result)
    names, sites = a.monitor_names, a.monitor_sites()
    assert len(names) == res[0].shape[0] == res[1].shape[0] == res[2].shape[0] and res[2].shape[1] == 321
    assert names[:2] == ['pre_net_out', 'encoder/conv_bank'] and 'post/encoded' in names and 'output' in names
    # the second model, the two halves by hand: what the workspace holds between forward and backward
    b, _ = _model()
    b.forward(masks)
    torch.cuda.synchronize()
    fwd = {'workspace': b.workspace.cpu().numpy(), 'seq2seq_output': b.seq2seq_output.cpu().numpy().reshape(-1),
           'output': b.output.cpu().numpy().reshape(-1)}
    b.backward()
    b.apply_gradients(1e-3)
    torch.cuda.synchronize()
    assert torch.equal(a.seq2seq_output, b.seq2seq_output) and torch.equal(a.output, b.output)
    _rows_match(res, names, {k: sites[k] for k in model_module.MONITOR_FORWARD}, fwd, 'forward sites')
    # (the backward pass may reuse workspace rows: which sites read differently afterwards, for the record; none has to)
    after = b.workspace.cpu().numpy()
    print('  workspace sites changed by the backward pass: %s' %
          [n for n, o, s in sites['workspace'] if not np.array_equal(after[o:o + s].view(np.uint32), fwd['workspace'][o:o + s].view(np.uint32))])
    # the flat buffers after the update (the gradient buffer is not written by it)
    upd = {'params': a.params.flat.cpu().numpy(), 'grads': a.grads.cpu().numpy(), 'adam_m': a.adam_m.cpu().numpy(),
           'adam_v': a.adam_v.cpu().numpy()}
    assert torch.equal(a.grads, b.grads) and torch.equal(a.params.flat, b.params.flat)
    _rows_match(res, names, {k: sites[k] for k in model_module.MONITOR_UPDATE}, upd, 'flat buffers')
    # pre_net_out sits behind a dropout of 0.5 and a ReLU: the zeros are counted
    i = names.index('pre_net_out')
    assert res[0][i, 0] == B * TT * 128 and res[0][i, 5] >= res[0][i, 0] // 2 - 200 and res[0][i, 2:5].sum() == 0
    # the same tensors every time
    first = a.monitor_result
    a.step(1e-3, masks=masks, monitor=True)
    assert a.monitor_result is first and all(x is y for x, y in zip(a.monitor_result, first))


def test_monitor_false_changes_nothing(built_lib, monkeypatch):
    monkeypatch.setenv('TACO_DETERMINISTIC', '1')
    a, masks = _model()
    b, _ = _model()
    for k in range(3):
        a.step(1e-3, masks=masks, monitor=(k != 1))
        b.step(1e-3, masks=masks)
    torch.cuda.synchronize()
    assert b.monitor_result is None and b._monitor is None
    assert torch.equal(a.params.flat, b.params.flat) and torch.equal(a.adam_m, b.adam_m) and torch.equal(a.adam_v, b.adam_v)
    assert float(a.loss) == float(b.loss) and a.global_step == b.global_step == 3


def test_a_planted_nan_is_reported_under_its_name(built_lib, monkeypatch):
    from tacotron_amd import train
    monkeypatch.setenv('TACO_DETERMINISTIC', '1')
    m, masks = _model()
    m.step(1e-3, masks=masks, monitor=True)
    torch.cuda.synchronize()
    assert train.monitor_nonfinite(m.monitor_names, m.monitor_result.counts.cpu().numpy()) == []
    table = {n: (o, s) for n, o, s, _ in built_lib.param_table(m.shape)}
    for name in ('decoder/attention_v', 'embedding', 'post/cbhg/proj2/bias'):
        off, size = table[name]
        for at in (0, size // 2, size - 1):
            keep = m.grads[off + at].clone()
            m.grads[off + at] = float('nan')
            m.monitor_stats(('grads',))
            torch.cuda.synchronize()
            counts = m.monitor_result.counts.cpu().numpy()
            assert train.monitor_nonfinite(m.monitor_names, counts) == ['grad/' + name], (name, at)
            assert counts[m.monitor_names.index('grad/' + name)].tolist()[:5] == [size, size - 1, 1, 0, 0]
            line = train.monitor_line(m.monitor_names, counts, m.monitor_result.moments.cpu().numpy(), 1e-3)
            assert line.endswith('non-finite 1: grad/' + name), line
            m.grads[off + at] = keep
    m.monitor_stats(('grads',))
    assert train.monitor_nonfinite(m.monitor_names, m.monitor_result.counts.cpu().numpy()) == []


def test_driver_writes_the_files_and_the_lines(built_lib, tmp_path, monkeypatch, capsys):
    from tacotron_amd.config import Config
    from tacotron_amd.train import train as run_train
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('TACO_DETERMINISTIC', '1')

    def run(monitor, save_path):
        c = Config()
        c.batch_size, c.max_decode_iter, c.data_path, c.save_path = 2, 8, str(tmp_path / 'nodata'), save_path
        m = run_train(c, num_steps=4, log_every=2, save_every=1000, monitor=monitor)
        return m, capsys.readouterr().out

    m1, out1 = run(True, 'mon')
    m0, out0 = run(False, 'plain')
    assert m1.global_step == m0.global_step == 4
    loss = lambda out: re.findall(r'^step (\d+) loss (\S+) \(seq2seq (\S+) \+ output (\S+)\) gnorm (\S+)', out, re.M)   # noqa: E731
    assert len(loss(out1)) == 2 and loss(out1) == loss(out0), (out1, out0)
    assert torch.equal(m1.params.flat, m0.params.flat)
    lines = re.findall(r'^step (\d+) (monitor grad-rms max \S+ \(\S+\) lr\|g\|/\|w\| max \S+ \(\S+\) pre_net_out zeros \S+% non-finite 0)$', out1, re.M)
    assert [s for s, _ in lines] == ['2', '4'], out1
    assert 'monitor' not in out0 and not os.path.exists(os.path.join('log', 'plain', 'monitor'))
    edges = built_lib.tensor_stats_edges()
    files = sorted(os.listdir(os.path.join('log', 'mon', 'monitor')))
    assert files == ['monitor_2.npz', 'monitor_4.npz']
    z2, z4 = (np.load(os.path.join('log', 'mon', 'monitor', f)) for f in files)
    for z in (z2, z4):
        N = len(z['names'])
        assert sorted(z.files) == ['counts', 'e_hi', 'e_lo', 'edges', 'hist', 'moments', 'names', 'sub_bits']
        assert z['counts'].shape == (N, 6) and z['moments'].shape == (N, 5) and z['hist'].shape == (N, 321) and z['edges'].shape == (322,)
        assert (int(z['e_lo']), int(z['e_hi']), int(z['sub_bits'])) == (-24, 15, 2) and np.array_equal(z['edges'], edges)
        assert z['names'].tolist() == m1.monitor_names and (z['hist'].sum(1) == z['counts'][:, 1]).all()
        assert (z['counts'][:, 0] > 0).all() and (z['counts'][:, 2:5] == 0).all()
    assert z2['names'].tolist() == z4['names'].tolist() and not np.array_equal(z2['moments'], z4['moments'])
    # the last file is the device's result, and that is the restatement on the final buffers
    assert np.array_equal(z4['counts'], m1.monitor_result.counts.cpu().numpy())
    i = z4['names'].tolist().index('param/embedding')
    off, size = [(o, s) for n, o, s, _ in built_lib.param_table(m1.shape) if n == 'embedding'][0]
    want = mr.stats(m1.params.flat.cpu().numpy()[off:off + size])
    assert np.array_equal(z4['counts'][i], want[0]) and np.array_equal(z4['hist'][i], want[2])
