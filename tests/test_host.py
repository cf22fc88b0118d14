"""CPU: host-side mirror of the reference interface -- Config defaults, prompt front end, r-frame layout, synthetic
batches, parameter initialisation rules."""
import os

import numpy as np
import pytest
import torch

from tacotron_amd import config as cfg
from tacotron_amd.audio import reshape_frames
from tacotron_amd.data import Vocab, load_prompts, pad, pad_to_dense, synthetic_batch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def test_config_defaults_equal_reference():
    # models/tacotron.py:12-33, audio.py:10-17
    c = cfg.Config()
    assert c.max_decode_iter == 108000 // (2 * 300) == 180
    assert (c.attention_units, c.decoder_units, c.mel_features, c.embed_dim, c.fft_size) == (256, 256, 80, 256, 1025)
    assert (c.char_dropout_prob, c.audio_dropout_prob, c.scheduled_sample) == (0.5, 0.5, 0.5)
    assert (c.num_speakers, c.speaker_embed_dim, c.cap_grads, c.batch_size) == (1, 16, 5, 32)
    assert c.init_lr == 0.0005 and c.annealing_rate == 1
    assert (cfg.n_fft, cfg.win_length, cfg.hop_length, cfg.maximum_audio_length, cfg.r) == (2048, 1200, 300, 108000, 2)
    assert (cfg.SAVE_EVERY, cfg.MAX_TEXT_LEN, cfg.BATCH_SIZE) == (5000, 140, 32)
    c.validate()
    c.embed_dim = 128
    with pytest.raises(ValueError):
        c.validate()


@pytest.mark.parametrize('r,steps', [(1, 360), (2, 180), (3, 120), (4, 90), (5, 72)])
def test_max_decode_iter_follows_r(r, steps):
    """maximum_audio_length // (r hop_length) for the r in use: the drivers set config.r at run time (checkpoint, meta.pkl)."""
    c = cfg.Config()
    c.r = r
    assert c.max_decode_iter == steps == 108000 // (300 * r)
    c.max_decode_iter = 8                  # an explicit setting holds whatever r is
    c.r = 1 if r != 1 else 2
    assert c.max_decode_iter == 8
    assert cfg.Config().max_decode_iter == 180


def test_reshape_frames_matches_reference_vectors():
    g = np.load(os.path.join(GOLD, 'reshape_frames.npz'))
    n = 0
    for k in g.files:
        if not k.startswith('x_'):
            continue
        r = int(k[3])
        f = reshape_frames(g[k], r)
        assert np.array_equal(f, g['fwd' + k[1:]]), k
        assert np.array_equal(reshape_frames(f, r, forward=False), g['inv' + k[1:]]), k
        n += 1
    assert n == 10
    # audio.py:106-115 self-test: ramp round trip
    test = np.repeat(np.arange(40)[:, None] + 1, 7, axis=1)
    assert np.array_equal(reshape_frames(reshape_frames(test.T, 2), 2, forward=False), test)
    # forward layout at r=2 is row 4b+j = [frame 8b+j, frame 8b+j+4]
    x = np.arange(16)[None, :].astype(float)
    assert reshape_frames(x, 2).tolist() == [[0, 4], [1, 5], [2, 6], [3, 7], [8, 12], [9, 13], [10, 14], [11, 15]]


def test_load_prompts_semantics():
    ivocab = {0: '<pad>', 1: 'a', 2: 'b', 3: ' ', 4: 'c'}
    prompts = ['ab c\n', 'zzab\n', 'c']
    batches = list(load_prompts(prompts, ivocab, batch_size=2))
    assert [b['text'].shape for b in batches] == [torch.Size([2, 140]), torch.Size([1, 140])]   # smaller final batch
    assert batches[0]['text'][0, :5].tolist() == [1, 2, 3, 4, 0]
    assert batches[0]['text'][1, :3].tolist() == [1, 2, 0]           # unknown chars dropped (data_input.py:94)
    assert batches[0]['text_length'].tolist() == [5, 5]              # len(raw line) incl. newline / unknown (data_input.py:95)
    assert pad([[1, 2], [3]], 4, 0).tolist() == [[1, 2, 0, 0], [3, 0, 0, 0]]


def test_synthetic_batch_shape_and_determinism():
    a = synthetic_batch(4, 20, 6, 2, 60, seed=1)
    b = synthetic_batch(4, 20, 6, 2, 60, seed=1)
    c = synthetic_batch(4, 20, 6, 2, 60, seed=1, rank=1)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a['mel'], c['mel'])
    assert a['text_length'][0] == 20 and int(a['text'].max()) < 60
    for i, L in enumerate(a['text_length'].tolist()):
        assert torch.all(a['text'][i, L:] == 0) and torch.all(a['text'][i, :L] > 0)
    assert a['mel'].shape == (4, 6, 160) and a['stft'].shape == (4, 6, 2050)


def test_param_init_rules(built_lib):
    from tacotron_amd.params import ParamBuffer, glorot_limit
    pb = ParamBuffer(built_lib.make_shape(2, 8, 4, 2, 30)).init_(seed=0)
    assert torch.all(pb.view('decoder/gru_0/gates/bias') == 1)       # GRUCell gates bias init 1.0
    assert torch.all(pb.view('decoder/gru_0/candidate/bias') == 0)
    assert torch.all(pb.view('encoder/cbhg/bank_bn/gamma') == 1) and torch.all(pb.view('post/cbhg/proj2_bn/beta') == 0)
    k = pb.view('encoder/cbhg/bank_4/kernel')
    lim = glorot_limit((4, 128, 128))
    assert abs(lim - np.sqrt(6.0 / (4 * 128 + 4 * 128))) < 1e-12 and float(k.abs().max()) <= lim and float(k.std()) > 0.4 * lim
    d = pb.to_dict()
    pb2 = ParamBuffer(pb.shape).load_dict_(d)
    assert torch.equal(pb.flat, pb2.flat)


def test_text_frontend_matches_reference_vectors():
    """data_input.pad, preprocess.process_char and preprocess.pad_to_dense pinned by vectors generated from the
    REFERENCE's own functions (tests/golden/make_text_golden.py)."""
    g = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'text_frontend.npz'))
    lens = g['pad_lens'].tolist()
    flat = g['pad_flat'].tolist()
    rows, o = [], 0
    for n in lens:
        rows.append(flat[o:o + n])
        o += n
    a = pad(rows, 140, 0)
    assert a.dtype == g['pad_out_140_0'].dtype and np.array_equal(a, g['pad_out_140_0'])
    assert np.array_equal(pad(rows, 12, 9), g['pad_out_12_9'])
    v = Vocab()
    ids = [v.encode(str(p)) for p in g['prompts']]
    assert [i for r in ids for i in r] == g['char_ids_flat'].tolist()
    assert [len(r) for r in ids] == g['char_lens'].tolist()
    items = sorted(v.vocab.items(), key=lambda kv: kv[1])
    assert [k for k, _ in items] == [str(c) for c in g['vocab_chars']]
    assert [i for _, i in items] == g['vocab_ids'].tolist()
    d1 = pad_to_dense([np.array(r, dtype=np.int32) for r in ids])
    assert d1.dtype == g['dense_1d'].dtype and np.array_equal(d1, g['dense_1d'])
    d2 = pad_to_dense([g['mat_0'], g['mat_1'], g['mat_2']])
    assert d2.dtype == g['dense_2d'].dtype and np.array_equal(d2, g['dense_2d'])
    # the vocabulary feeds load_prompts exactly as the reference's pickled ivocab does
    b = next(load_prompts(['Hello'], v.ivocab, batch_size=4))
    assert b['text'][0, :5].tolist() == ids[0][:5]


def test_latest_checkpoint_is_numeric_and_prefix_aware(tmp_path):
    """'tacotron-5000' sorts after 'tacotron-10000' lexicographically; restore must pick the highest STEP and
    must find debug-mode checkpoints ('weights/debug-N') too (train.py:49-52 uses tf.train.latest_checkpoint)."""
    from tacotron_amd.train import latest_checkpoint
    d = tmp_path / 'weights' / 'nancy'
    d.mkdir(parents=True)
    for n in ('tacotron-5000', 'tacotron-10000', 'tacotron-95000', 'tacotron-100000', 'tacotron-old', 'other-999999'):
        (d / n).write_bytes(b'x')
    assert latest_checkpoint(str(d / 'tacotron')).endswith('tacotron-100000')
    (tmp_path / 'weights' / 'debug-15000').write_bytes(b'x')
    (tmp_path / 'weights' / 'debug-5000').write_bytes(b'x')
    assert latest_checkpoint(str(tmp_path / 'weights' / 'debug')).endswith('debug-15000')
    assert latest_checkpoint(str(tmp_path / 'nowhere' / 'tacotron')) is None


@pytest.mark.parametrize('S', [1, 7])
def test_tf_checkpoint_rename_table_round_trip(built_lib, S):
    """the TF-1.2 scope -> taco_param_table rename map is code (tacotron_amd/tf_import.py).  A synthetic
    "checkpoint" keyed by the TF names (plus Adam slots, BN moving statistics and bookkeeping variables, as a real one has)
    imports to exactly the parameter buffer it was made from; name mismatches are reported, not guessed."""
    from oracle import taco_numpy as on
    from tacotron_amd.params import ParamBuffer
    from tacotron_amd.tf_import import check_names, import_tf_variables, tf_name_map
    V, r = 33, 2
    shape = built_lib.make_shape(2, 8, 4, r, V, S)
    p = on.init_params(V, r, seed=2, perturb=0.3, num_speakers=S)
    table = tf_name_map(S)
    assert set(table) == set(p) and len(set(table.values())) == len(table)          # total and injective
    assert table['encoder/cbhg/bank_16/kernel'] == 'encoder/cbhg/conv1d_15/kernel'
    assert table['post/cbhg/proj2/kernel'] == 'post-process/cbhg/conv1d_9/kernel'
    assert table['post/cbhg/highway_0/adapt/kernel'] == 'post-process/cbhg/highway_0/dense/kernel'
    assert table['post/cbhg/highway_0/H/kernel'] == 'post-process/cbhg/highway_0/dense_2/kernel'
    assert table['encoder/cbhg/highway_2/H/kernel'] == ('encoder/cbhg/highway_2/dense_%d/kernel' % (3 if S > 1 else 1))
    rng = np.random.default_rng(0)
    ckpt = {}
    for n, a in p.items():
        ckpt[table[n] + ':0'] = a.astype(np.float32)
        ckpt[table[n] + '/Adam'] = rng.standard_normal(a.shape).astype(np.float32)
        ckpt[table[n] + '/Adam_1'] = rng.random(a.shape).astype(np.float32)
    ckpt['encoder/cbhg/batch_normalization/moving_mean'] = np.zeros(2048, np.float32)
    ckpt['global_step'] = np.int64(12345)
    ckpt['beta1_power'] = np.float32(0.5)
    ckpt['stft_mean'] = rng.standard_normal(1025 * r).astype(np.float32)
    ckpt['stft_std'] = rng.random(1025 * r).astype(np.float32)
    assert check_names(ckpt.keys(), shape) == ([], [])
    sd = import_tf_variables(ckpt, shape)
    want = ParamBuffer(shape).load_dict_(p).flat
    assert torch.equal(sd['params'], want) and sd['global_step'] == 12345
    assert sd['adam_m'].shape == want.shape and torch.equal(sd['stft_mean'], torch.from_numpy(ckpt['stft_mean']))
    # a renamed / missing variable is reported by name
    bad = dict(ckpt)
    bad['decoder/attention_v_renamed'] = bad.pop(table['decoder/attention_v'] + ':0')
    missing, extra = check_names(bad.keys(), shape)
    assert missing == [table['decoder/attention_v']] and extra == ['decoder/attention_v_renamed']
    with pytest.raises(KeyError):
        import_tf_variables(bad, shape)


def test_device_feeder_rotation_and_order():
    """tacotron_amd.data.DeviceFeeder on the CPU path (no pinning, synchronous copies): batches arrive in draw order, the buffer
    set handed out last is not overwritten until the next call, and the worker never runs more than
    depth + 1 batches ahead of the consumer (the slot gate that keeps a set in use from being refilled)."""
    import time
    import numpy as np
    from tacotron_amd.data import DeviceFeeder
    n, B = 50, 4
    data = {'text': np.arange(n * 3, dtype=np.int32).reshape(n, 3), 'mel': np.arange(n * 2, dtype=np.float32).reshape(n, 2, 1)}
    drawn = []

    def draw(step):
        idx = (np.arange(B) * 7 + step * 3) % n
        drawn.append(step)
        return idx
    f = DeviceFeeder(data, B, device='cpu', depth=2, draw=draw)
    try:
        time.sleep(0.3)
        assert max(drawn) <= 2, 'worker ran %d batches ahead with nothing consumed (3 buffer sets)' % max(drawn)
        for step in range(12):
            b = f.next()
            idx = (np.arange(B) * 7 + step * 3) % n
            assert np.array_equal(b['text'].numpy(), data['text'][idx]) and np.array_equal(b['mel'].numpy(), data['mel'][idx])
            time.sleep(0.02)   # (the worker has time to run ahead: the current set must survive it)
            assert np.array_equal(b['text'].numpy(), data['text'][idx])
            assert max(drawn) <= step + 3
    finally:
        f.close()


def test_crc32c_and_snappy_primitives():
    """Known answers of the two primitives the bundle reader rests on: CRC-32C("123456789") = 0xE3069283 (the Castagnoli check
    value), the table magic, and a snappy stream with a literal and an overlapping back-reference."""
    from tacotron_amd import tf_bundle as tb
    assert tb.crc32c(b'123456789') == 0xE3069283
    assert tb.mask_crc(0) == 0xa282ead8
    # "abcabcabcabcX": literal 'abc' (tag 0x08), copy-1 len 9 off 3 (tag = 1 | (9 - 4) << 2 | (3 >> 8) << 5 = 0x15, byte 3), literal 'X'
    stream = bytes([13, 0x08]) + b'abc' + bytes([0x15, 3, 0x00]) + b'X'
    assert tb.snappy_decompress(stream) == b'abcabcabcabcX'


@pytest.mark.parametrize('snappy,block_size', [(False, 4096), (False, 300), (True, 700)], ids=['plain', 'tiny-blocks', 'snappy'])
def test_tf_bundle_reader_feeds_the_importer(built_lib, tmp_path, snappy, block_size):
    """VERDICT r4 #8b: `tf_import.import_tf_variables` fed by the TensorFlow-free bundle reader.  A checkpoint with the reference's
    variable names (weights, Adam slots, BN moving statistics, global_step, stft statistics) is written as `<prefix>.index` +
    `<prefix>.data-00000-of-00001` by the independent writer of tests/bundle_writer.py -- several data blocks (prefix-compressed
    keys across restart points), optionally snappy-framed -- read back with tf_bundle.load_checkpoint (index CRCs and tensor CRCs
    verified) and imported: the parameter buffer equals the one the variables were made from; a flipped byte is detected."""
    from oracle import taco_numpy as on
    from tacotron_amd import tf_bundle as tb
    from tacotron_amd.params import ParamBuffer
    from tacotron_amd.tf_import import import_tf_variables, tf_name_map
    from tests.bundle_writer import write_bundle
    V, r, S = 33, 2, 1
    shape = built_lib.make_shape(2, 8, 4, r, V, S)
    p = on.init_params(V, r, seed=5, perturb=0.3, num_speakers=S)
    table = tf_name_map(S)
    rng = np.random.default_rng(1)
    ckpt = {}
    with_slots = not snappy and block_size == 4096   # (the CRCs are pure Python, ~10 MB/s: the 2 x 27 MB of Adam slots in one case only)
    for n, a in p.items():
        ckpt[table[n]] = a.astype(np.float32)
        if with_slots:
            ckpt[table[n] + '/Adam'] = rng.standard_normal(a.shape).astype(np.float32)
            ckpt[table[n] + '/Adam_1'] = rng.random(a.shape).astype(np.float32)
    ckpt['encoder/cbhg/batch_normalization/moving_mean'] = np.zeros(2048, np.float32)
    ckpt['global_step'] = np.array(54321, dtype=np.int64)
    ckpt['stft_mean'] = rng.standard_normal(1025 * r).astype(np.float32)
    ckpt['stft_std'] = rng.random(1025 * r).astype(np.float32)
    prefix = str(tmp_path / 'tacotron-54321')
    write_bundle(prefix, ckpt, block_size=block_size, snappy=snappy)
    listed = tb.list_variables(prefix)
    assert set(listed) == set(ckpt) and listed['global_step'] == (np.int64, ())
    assert listed[table['decoder/attention_v']] == (np.float32, (256,))
    got = tb.load_checkpoint(prefix, verify_tensors=True)
    assert set(got) == set(ckpt) and all(np.array_equal(got[k], ckpt[k]) and got[k].dtype == ckpt[k].dtype for k in ckpt)
    sd = import_tf_variables(got, shape)
    assert torch.equal(sd['params'], ParamBuffer(shape).load_dict_(p).flat) and sd['global_step'] == 54321
    assert ('adam_m' in sd) == with_slots and torch.equal(sd['stft_std'], torch.from_numpy(ckpt['stft_std']))
    only = tb.load_checkpoint(prefix, names={'global_step', 'stft_mean'})
    assert set(only) == {'global_step', 'stft_mean'}
    # corruption is detected: one byte of a tensor, one byte of the index
    data = bytearray(open(prefix + '.data-00000-of-00001', 'rb').read())
    data[100] ^= 0x40
    open(prefix + '.data-00000-of-00001', 'wb').write(bytes(data))
    with pytest.raises(ValueError, match='CRC'):
        tb.load_checkpoint(prefix, verify_tensors=True)
    idx = bytearray(open(prefix + '.index', 'rb').read())
    idx[10] ^= 0x01
    open(prefix + '.index', 'wb').write(bytes(idx))
    with pytest.raises(ValueError):
        tb.load_checkpoint(prefix)


def test_bench_self_launch_command(monkeypatch):
    """bench.py --gpus N (N > 1) without a torchrun environment re-executes itself under torch.distributed.run on 127.0.0.1
    (VERDICT r5 #1); with fewer GPUs than ranks and no --rehearse-shared-device it refuses with exit code 2."""
    import argparse
    import importlib.util
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('bench_mod', os.path.join(root, 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    seen = {}

    def fake_call(cmd, env=None):
        seen['cmd'], seen['env'] = cmd, env
        return 0
    monkeypatch.setattr(subprocess, 'call', fake_call)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '2', '--rehearse-shared-device', '--steps', '3'])
    assert bench.self_launch(argparse.Namespace(gpus=2, rehearse_shared_device=True)) == 0
    cmd = seen['cmd']
    assert cmd[1:4] == ['-m', 'torch.distributed.run', '--nnodes=1']
    assert cmd[cmd.index('--nproc-per-node') + 1] == '2' and cmd[cmd.index('--master-addr') + 1] == '127.0.0.1'
    assert cmd[-5:] == ['--gpus', '2', '--rehearse-shared-device', '--steps', '3'] and cmd[-6].endswith('bench.py')
    assert seen['env']['GPU_MAX_HW_QUEUES'] == os.environ.get('GPU_MAX_HW_QUEUES', '8')
    assert seen['env']['HSA_ENABLE_IPC_MODE_LEGACY'] == os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    if not __import__('torch').cuda.is_available():
        assert bench.self_launch(argparse.Namespace(gpus=8, rehearse_shared_device=False)) == 2


def test_bench_dump_outputs_fits_budget_and_is_repeatable(tmp_path, monkeypatch):
    """bench.py --dump-outputs: the last timed step's outputs as float32 .npy, at most 64 MB in all at the S1 shape (B=32, Tt=200,
    Td=180, r=2: 111 MB whole); arrays over their share of the budget are a fixed sample that depends on the shape only."""
    import importlib.util
    import types
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('bench_mod', os.path.join(root, 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    monkeypatch.setattr(torch.cuda, 'synchronize', lambda: None)
    B, Tt, Td, n = 32, 200, 180, 6926609
    g = torch.Generator().manual_seed(0)
    model = types.SimpleNamespace(_loss=torch.rand(3, generator=g), _gnorm=torch.rand(1, generator=g),
                                  seq2seq_output=torch.rand(B, Td, 160, generator=g), output=torch.rand(B, Td, 2050, generator=g),
                                  alignments=torch.rand(B, Td, Tt, generator=g), grads=torch.rand(n, generator=g),
                                  params=types.SimpleNamespace(flat=torch.rand(n, generator=g)))
    names = ['loss', 'global_gradient_norm', 'seq2seq_output', 'output', 'alignments', 'grads', 'params']
    for d in ('a', 'b'):
        bench.dump_outputs(model, str(tmp_path / d))
    assert sorted(os.listdir(tmp_path / 'a')) == sorted(k + '.npy' for k in names)
    assert sum(os.path.getsize(tmp_path / 'a' / f) for f in os.listdir(tmp_path / 'a')) <= 64e6
    for k in names:
        a, b = np.load(tmp_path / 'a' / (k + '.npy')), np.load(tmp_path / 'b' / (k + '.npy'))
        assert a.dtype == np.float32 and np.array_equal(a, b), k
    for k, t in (('loss', model._loss), ('global_gradient_norm', model._gnorm), ('seq2seq_output', model.seq2seq_output),
                 ('alignments', model.alignments)):
        assert np.array_equal(np.load(tmp_path / 'a' / (k + '.npy')), t.numpy()), k   # whole, in its own shape
    out = np.load(tmp_path / 'a' / 'output.npy')
    full = model.output.numpy().reshape(-1)
    assert out.ndim == 1 and out.size < full.size
    assert np.array_equal(out, full[np.sort(np.random.default_rng(0).choice(full.size, out.size, replace=False))])


def test_bench_time_steps_runs_the_restart_hook_before_the_last_timed_step(built_lib, monkeypatch):
    """--dump-outputs: time_steps calls its `before_last` hook once, after the warm-up and the first steps-1 timed steps, right
    before the last one; --steps sets the number of timed steps."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('bench_mod', os.path.join(root, 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    monkeypatch.setattr(torch.cuda, 'synchronize', lambda: None)
    monkeypatch.setattr(built_lib, 'profile_enable', lambda bits: None)
    monkeypatch.setattr(built_lib, 'profile_read', lambda which, with_flops=False: [])
    monkeypatch.setattr(torch, 'tensor', lambda x, dtype=None, device=None: torch.as_tensor(x, dtype=dtype))   # (no device here)
    log = []

    class Model:
        def step(self):
            log.append('step')
    bench.time_steps(Model(), 4, 2, lambda: None, 1, before_last=lambda: log.append('restart'))
    assert log == ['step'] * 5 + ['restart', 'step']
    log.clear()
    bench.time_steps(Model(), 3, 0, lambda: None, 1)
    assert log == ['step'] * 3


def test_device_feeder_keeps_raising_after_its_worker_died():
    """once the DeviceFeeder worker has died with an exception, EVERY later next() re-raises it (the first form raised once
    and then blocked forever on the empty queue); close() still returns."""
    import time
    from tacotron_amd.data import DeviceFeeder
    data = {'x': np.arange(40, dtype=np.float32).reshape(20, 2)}
    calls = {'n': 0}

    def draw(step):
        calls['n'] += 1
        if step >= 2:
            raise RuntimeError('corpus went away at step %d' % step)
        return np.arange(4) + step

    f = DeviceFeeder(data, 4, device='cpu', depth=1, draw=draw)
    a = f.next()['x'].clone()
    b = f.next()['x'].clone()
    assert a[0, 0] == 0 and b[0, 0] == 2          # rows 0.. and rows 1.. of the (20, 2) ramp
    # a worker that is merely SLOW (longer than next()'s 1 s liveness poll) is waited for, not mistaken for a dead one
    slow = {'n': 0}

    def slow_draw(step):
        slow['n'] += 1
        if step == 1:
            time.sleep(1.6)
        return np.arange(4) + step
    g = DeviceFeeder(data, 4, device='cpu', depth=1, draw=slow_draw)
    assert g.next()['x'][0, 0] == 0 and g.next()['x'][0, 0] == 2
    g.close()
    t0 = time.perf_counter()
    for _ in range(3):
        with pytest.raises(RuntimeError, match='corpus went away'):
            f.next()
    assert time.perf_counter() - t0 < 5.0          # (promptly: no blocking get on a queue nobody fills any more)
    f.close()
