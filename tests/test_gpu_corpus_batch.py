"""GPU: taco_corpus_batch (the batch gather with the corpus standardisation fused in) and the feeders / train driver on top of it.

The reference is NumPy on fp32: out[b] = (x[index[b]].astype(float32) - mean) / std -- one IEEE subtraction and one correctly
rounded division per element, which the kernel must reproduce bit for bit (compared as int32 views; all values finite, so no
NaN payload is involved).  Every call here reads a source that lies between two rows of NaN and writes an output that lies
between two bands of a sentinel value: a read or a write outside the tensors shows as a wrong value, never as a fault."""
import ctypes

import numpy as np
import pytest
import torch

from tests.corpus_ref import bits, standardise, write_corpus

pytestmark = pytest.mark.gpu

N = 5
WIDTHS = (7, 80, 160, 1025, 2050, 5125)
STEPS = (1, 3, 4)
SENTINEL = 12345.0
BAND = 64   # floats either side of the output: 256 bytes, so the band itself does not change the output's alignment


def source(C, Td, dtype, seed):
    """(N, Td, C) values of `dtype`, all representable in fp16: ordinary log-magnitudes plus +-0, fp16 subnormals (the smallest, the
    largest), the smallest normal and +-65504, placed so that every row, the first and last elements included, holds some."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((N, Td, C)) * 3.0 - 5.0).astype(np.float16)
    special = np.array([0.0, -0.0, 5.96e-8, -5.96e-8, 6.0976e-5, -6.0976e-5, 6.104e-5, 65504.0, -65504.0], dtype=np.float16)
    flat = x.reshape(N, -1)
    for n in range(N):
        pos = np.unique(np.concatenate([[0, flat.shape[1] - 1], rng.integers(flat.shape[1], size=12)]))
        flat[n, pos] = special[(np.arange(len(pos)) + n) % len(special)]
    return x.astype(dtype)


def stats(C, seed):
    rng = np.random.default_rng(seed)
    mean = (rng.standard_normal(C) * 4.0).astype(np.float32)                  # either sign
    std = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), C)).astype(np.float32)   # [1e-3, 1e3], never 0
    return mean, std


def run(lib, x, mean, std, index, src_off=0, out_off=0, n_bad=False):
    """lib.corpus_batch on x (N, Td, C; NumPy) -> (out as NumPy, width, n_bad or None).  The source is the middle N rows of an
    allocation of N + 2 rows whose first and last rows are NaN and which starts `src_off` elements into its buffer; the output
    starts `out_off` floats behind a sentinel band and is followed by another, both checked afterwards."""
    n, Td, C = x.shape
    row = Td * C
    tdt = torch.float16 if x.dtype == np.float16 else torch.float32
    sbuf = torch.full(((n + 2) * row + src_off,), float('nan'), dtype=tdt, device='cuda')
    rows = sbuf[src_off:].view(n + 2, Td, C)
    src = rows[1:n + 1]
    src.copy_(torch.from_numpy(x))
    B = n if index is None else len(index)
    obuf = torch.full((B * row + 2 * BAND + out_off,), SENTINEL, dtype=torch.float32, device='cuda')
    out = obuf[BAND + out_off:BAND + out_off + B * row].view(B, Td, C)
    idx = None if index is None else torch.as_tensor(np.asarray(index, dtype=np.int64)).cuda()
    dm, ds = (None, None) if mean is None else (torch.from_numpy(mean).cuda(), torch.from_numpy(std).cuda())
    bad = torch.full((1,), 77, dtype=torch.int32, device='cuda') if n_bad else None
    got = lib.corpus_batch(src, dm, ds, index=idx, out=out, n_bad=bad)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    whole = obuf.cpu().numpy()
    assert (whole[:BAND + out_off] == SENTINEL).all() and (whole[BAND + out_off + B * row:] == SENTINEL).all(), 'wrote outside out'
    width = lib.corpus_batch_width(src.data_ptr(), out.data_ptr(), row, tdt == torch.float16)
    return whole[BAND + out_off:BAND + out_off + B * row].reshape(B, Td, C), width, (int(bad.item()) if n_bad else None)


@pytest.mark.parametrize('dtype', [np.float16, np.float32], ids=['fp16', 'fp32'])
@pytest.mark.parametrize('Td', STEPS)
@pytest.mark.parametrize('C', WIDTHS)
def test_bit_parity_with_numpy(built_lib, C, Td, dtype):
    x = source(C, Td, dtype, seed=C + Td)
    mean, std = stats(C, seed=C)
    for B in (1, 3, 9):   # 9 > N: repeated rows
        index = np.random.default_rng(B).integers(N, size=B)
        for m, s in ((mean, std), (None, None)):
            got, width, _ = run(built_lib, x, m, s, index)
            want = standardise(x, m, s)[index]
            assert np.isfinite(want).all()
            diff = bits(got) != bits(want)
            assert not diff.any(), 'C=%d Td=%d %s B=%d stats=%s width=%d: %d elements differ, first at %s: got %r want %r' % (
                C, Td, x.dtype, B, m is not None, width, diff.sum(), np.argwhere(diff)[0], got[diff][0], want[diff][0])
    got, _, _ = run(built_lib, x, mean, std, None)   # identity form (the feeder's): row b of src
    assert np.array_equal(bits(got), bits(standardise(x, mean, std)))


def test_shapes_cover_every_path(built_lib):
    """The widths the host picks over the shapes above (fresh allocations are at least 16-byte aligned, and run() keeps that):
    fp16 row pitches on 2-, 4-, 8- and 16-byte boundaries take V = 1, 2, 4 and the 16-byte vector path V = 8; fp32 V = 1, 2, 4."""
    seen = {np.float16: set(), np.float32: set()}
    for dtype in seen:
        for C in WIDTHS:
            for Td in STEPS:
                x = np.zeros((N, Td, C), dtype=dtype)
                seen[dtype].add(run(built_lib, x, None, None, [0])[1])
    assert seen[np.float16] == {8, 4, 2, 1} and seen[np.float32] == {4, 2, 1}, seen


@pytest.mark.parametrize('dtype', [np.float16, np.float32], ids=['fp16', 'fp32'])
@pytest.mark.parametrize('C,Td', [(160, 4), (2050, 4), (1025, 3)])
def test_misaligned_bases(built_lib, C, Td, dtype):
    """src one element into its allocation and / or out one float into its own: narrower paths, the same bits."""
    x = source(C, Td, dtype, seed=11)
    mean, std = stats(C, seed=12)
    index = [4, 0, 0, 3, 1, 2, 4]
    want = bits(standardise(x, mean, std)[index])
    widths = {}
    for src_off in (0, 1):
        for out_off in (0, 1):
            got, widths[src_off, out_off], _ = run(built_lib, x, mean, std, index, src_off, out_off)
            assert np.array_equal(bits(got), want), (src_off, out_off, widths)
    # one element (2 or 4 bytes) or one float off a 16-byte boundary leaves only the scalar path; at the base the row decides
    fp16 = dtype == np.float16
    assert widths[0, 0] == built_lib.corpus_batch_width(0, 0, Td * C, fp16) == {640: 8 if fp16 else 4, 8200: 8 if fp16 else 4, 3075: 1}[Td * C]
    assert widths[0, 1] == widths[1, 0] == widths[1, 1] == 1


@pytest.mark.parametrize('dtype', [np.float16, np.float32], ids=['fp16', 'fp32'])
@pytest.mark.parametrize('C,Td', [(160, 4), (1025, 3), (7, 1)])
def test_bad_indices_are_zero_rows_and_counted(built_lib, C, Td, dtype):
    x = source(C, Td, dtype, seed=21)
    mean, std = stats(C, seed=22)
    for m, s in ((mean, std), (None, None)):
        got, _, n_bad = run(built_lib, x, m, s, [-1, 2, N, 0], n_bad=True)
        want = standardise(x, m, s)
        assert n_bad == 2
        assert not np.isnan(got).any(), 'a NaN guard row was read'
        assert (bits(got[0]) == 0).all() and (bits(got[2]) == 0).all()
        assert np.array_equal(bits(got[1]), bits(want[2])) and np.array_equal(bits(got[3]), bits(want[0]))
    got, _, n_bad = run(built_lib, x, mean, std, [1, 3], n_bad=True)
    assert n_bad == 0 and np.array_equal(bits(got), bits(standardise(x, mean, std)[[1, 3]]))
    got, _, n_bad = run(built_lib, x, mean, std, [np.iinfo(np.int64).min, np.iinfo(np.int64).max, 1 << 32], n_bad=True)
    assert n_bad == 3 and (bits(got) == 0).all()


def test_rows_beyond_two_to_the_31_elements(built_lib):
    """A source of more than 2^31 elements (5900 utterances at the Nancy shape, 4.4 GB of fp16; only the rows read are filled):
    the row offset index * row must be formed in 64 bits."""
    Td, C, n = 180, 2050, 5900
    row = Td * C
    pick = [n - 1, 0, 5820]
    assert pick[2] * row > 1 << 31
    rng = np.random.default_rng(31)
    rows = (rng.standard_normal((3, Td, C)) * 3.0 - 5.0).astype(np.float16)
    mean, std = stats(C, seed=32)
    src = torch.empty((n, Td, C), dtype=torch.float16, device='cuda')
    for r, i in enumerate(pick):
        src[i].copy_(torch.from_numpy(rows[r]))
    out = built_lib.corpus_batch(src, torch.from_numpy(mean).cuda(), torch.from_numpy(std).cuda(),
                                 index=torch.as_tensor(pick, dtype=torch.int64).cuda())
    got = out.cpu().numpy()
    del src, out
    torch.cuda.empty_cache()
    assert np.array_equal(bits(got), bits(standardise(rows, mean, std)))


def test_einval_before_anything_is_enqueued(built_lib):
    """Every refusal of include/taco_hip.h's list: TACO_EINVAL, a message that names the argument, and neither the output nor
    *n_bad (which an accepted call zeroes first) touched."""
    lib = built_lib
    Td, C, B = 3, 14, 4
    row = Td * C
    # every pointer below lies inside this one allocation: B rows of room, the N source rows, B rows of room
    room = torch.zeros((N + 2 * B) * row, dtype=torch.float32, device='cuda')
    src = room[B * row:(B + N) * row]
    out = torch.full((B * row,), SENTINEL, dtype=torch.float32, device='cuda')
    mean, std = torch.zeros(C, device='cuda'), torch.ones(C, device='cuda')
    index = torch.zeros(B, dtype=torch.int64, device='cuda')
    bad = torch.full((1,), 77, dtype=torch.int32, device='cuda')
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    ok = dict(src=p(src), fp16=0, index=p(index), mean=p(mean), std=p(std), out=p(out), n_bad=p(bad), N=N, B=B, row=row, C=C)
    cases = [
        (dict(src=None), 'src'), (dict(out=None), 'out'), (dict(N=0), 'N='), (dict(N=-3), 'N='), (dict(B=0), 'B='),
        (dict(B=-1), 'B='), (dict(row=0), 'row='), (dict(row=-row), 'row='), (dict(C=0), 'C='), (dict(C=-C), 'C='),
        (dict(C=C - 1), 'multiple of C'), (dict(index=None, B=N + 1), 'index'),
        (dict(mean=None), 'mean and std'), (dict(std=None), 'mean and std'),
        (dict(out=ctypes.c_void_p(src.data_ptr() + 4 * row)), 'overlaps'),              # out inside src
        (dict(out=ctypes.c_void_p(src.data_ptr() - 4 * (B * row - 1))), 'overlaps'),   # out's last float is src's first
        (dict(fp16=1, out=ctypes.c_void_p(src.data_ptr() + 2 * N * row - 4)), 'overlaps'),   # ... an fp16 src's last two halves
    ]
    for change, word in cases:
        a = dict(ok, **change)
        rc = lib._lib.taco_corpus_batch(a['src'], a['fp16'], a['index'], a['mean'], a['std'], a['out'], a['n_bad'], a['N'], a['B'],
                                        a['row'], a['C'], lib.stream_ptr())
        assert rc == -1 and word in lib.last_error(), (change, rc, lib.last_error())
    torch.cuda.synchronize()
    assert int(bad.item()) == 77 and bool((out == SENTINEL).all()) and bool((room == 0).all())
    a = ok   # and the same arguments unchanged are accepted; adjacent tensors do not overlap
    assert lib._lib.taco_corpus_batch(a['src'], 0, a['index'], a['mean'], a['std'], a['out'], a['n_bad'], N, B, row, C, lib.stream_ptr()) == 0
    for o in (src.data_ptr() - 4 * B * row, src.data_ptr() + 4 * N * row):   # out ends where src begins / begins where it ends
        assert lib._lib.taco_corpus_batch(a['src'], 0, a['index'], a['mean'], a['std'], ctypes.c_void_p(o), None, N, B, row, C,
                                          lib.stream_ptr()) == 0, lib.last_error()
    torch.cuda.synchronize()
    assert int(bad.item()) == 0 and bool((out == 0).all())


def test_graph_replay_follows_the_index(built_lib):
    """Captured once, replayed with other contents in `index`: the call reads nothing from it on the host."""
    Td, C, B = 4, 160, 6
    x = source(C, Td, np.float16, seed=41)
    mean, std = stats(C, seed=42)
    src, dm, ds = torch.from_numpy(x).cuda(), torch.from_numpy(mean).cuda(), torch.from_numpy(std).cuda()
    index = torch.zeros(B, dtype=torch.int64, device='cuda')
    out = torch.empty((B, Td, C), dtype=torch.float32, device='cuda')
    bad = torch.zeros(1, dtype=torch.int32, device='cuda')
    call = lambda: built_lib.corpus_batch(src, dm, ds, index=index, out=out, n_bad=bad)   # noqa: E731
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            call()
    torch.cuda.synchronize()
    want = standardise(x, mean, std)
    for idx in ([4, 3, 2, 1, 0, 0], [1, 9, 1, -2, 3, 3], [0, 0, 0, 0, 0, 4]):
        index.copy_(torch.as_tensor(idx, dtype=torch.int64))
        out.fill_(SENTINEL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        valid = [0 <= i < N for i in idx]
        assert int(bad.item()) == valid.count(False)
        for b, i in enumerate(idx):
            assert np.array_equal(bits(got[b]), bits(want[i]) if valid[b] else np.zeros_like(bits(got[b]))), (idx, b)


# ---- feeders and the train driver ------------------------------------------------------------------------------------------

def corpus_on_disk(tmp_path, n=40, Td=10, Tt=24):
    """-> (data, norm as train.open_corpus returns them, {name: the standardised fp32 array NumPy gives})."""
    from tacotron_amd import train
    write_corpus(tmp_path / 'c', N=n, Td=Td, r=2, Tt=Tt)
    meta, data, norm = train.open_corpus(str(tmp_path / 'c'))
    ref = {k: (standardise(v, *norm[k]) if k in norm else np.asarray(v)) for k, v in data.items()}
    return meta, data, norm, ref


@pytest.mark.parametrize('kind', ['DeviceFeeder', 'DeviceCorpus'])
def test_feeders_with_norm_hand_out_numpys_batches(built_lib, kind, tmp_path):
    from tacotron_amd import data as data_mod
    _, data, norm, ref = corpus_on_disk(tmp_path)
    B = 4
    draws = [np.random.default_rng(100 + s).integers(40, size=B) for s in range(12)]
    kw = {'depth': 2} if kind == 'DeviceFeeder' else {'chunk_rows': 16}   # (40 rows: three staged chunks, the last one short)
    feeder = getattr(data_mod, kind)(data, B, device='cuda', draw=lambda step: draws[step] if step < 12 else draws[0], norm=norm, **kw)
    try:
        if kind == 'DeviceCorpus':
            assert feeder.data['stft'].dtype == torch.float16 and feeder.data['mel'].dtype == torch.float16
            assert np.array_equal(feeder.data['stft'].cpu().numpy(), np.asarray(data['stft']))
        else:
            assert feeder._dev[0]['stft'].dtype == torch.float16 and feeder._pinned[0]['mel'].dtype == torch.float16
        for s in range(12):
            batch = feeder.next()
            torch.cuda.synchronize()
            assert set(batch) == set(ref)
            for k, v in ref.items():
                got = batch[k].cpu().numpy()
                assert got.dtype == v.dtype and got.shape == v[draws[s]].shape, (s, k)
                assert np.array_equal(bits(got), bits(v[draws[s]])) if k in norm else np.array_equal(got, v[draws[s]]), (s, k)
    finally:
        feeder.close()


def test_device_feeder_with_norm_feeds_the_train_step(built_lib, tmp_path, monkeypatch):
    """The shape of test_gpu_frontend.test_device_feeder_feeds_the_train_step with norm=: 12 Tacotron.step()s on the feeder's
    tensors, never synchronised in between, end in the parameters that 12 steps on plainly copied batches of NumPy's standardised
    arrays end in, bit for bit -- no slot (fp16 or fp32) is recycled under a running step."""
    from tacotron_amd.config import Config
    from tacotron_amd.data import DeviceFeeder
    from tacotron_amd.model import Tacotron
    monkeypatch.setenv('TACO_DETERMINISTIC', '1')
    meta, data, norm, ref = corpus_on_disk(tmp_path)
    c = Config()
    c.r, c.vocab_size = meta['r'], len(meta['vocab'])
    B = 4
    draws = [np.random.default_rng(100 + s).integers(40, size=B) for s in range(12)]
    plain = lambda s: {k: torch.from_numpy(np.ascontiguousarray(v[draws[s]])) for k, v in ref.items()}   # noqa: E731
    feeder = DeviceFeeder(data, B, device='cuda', depth=2, draw=lambda step: draws[step] if step < 12 else draws[0], norm=norm)
    ma = Tacotron(c, plain(0), train=True, seed=1)
    mb = Tacotron(c, plain(0), train=True, seed=1)
    try:
        for s in range(12):
            dev_batch = feeder.next()
            ma.set_inputs(dev_batch)
            assert ma.inputs['stft'].data_ptr() == dev_batch['stft'].data_ptr(), 'set_inputs copied a device tensor'
            ma.step(lr=1e-3)
            mb.set_inputs(plain(s))
            mb.step(lr=1e-3)
        torch.cuda.synchronize()
    finally:
        feeder.close()
    ma.check(); mb.check()
    assert torch.equal(ma.params.flat, mb.params.flat)


def test_train_driver_default_equals_corpus_fp32(built_lib, tmp_path, monkeypatch):
    """train.train() for 3 steps on a corpus on disk: the default (corpus as stored + norm=) and corpus_fp32=True (load_corpus)
    end in the same parameters bit for bit, and both carry the statistics for the checkpoint."""
    from tacotron_amd.config import Config
    from tacotron_amd.train import train as run_train
    monkeypatch.setenv('TACO_DETERMINISTIC', '1')
    monkeypatch.chdir(tmp_path)
    write_corpus(tmp_path / 'c', N=12, Td=8, r=2, Tt=16)
    models = []
    for fp32 in (False, True):
        c = Config()
        c.batch_size, c.max_decode_iter, c.data_path, c.save_path = 4, 8, str(tmp_path / 'c'), 'debug'
        models.append(run_train(c, num_steps=3, corpus_fp32=fp32))
    a, b = models
    assert a.global_step == 3 and b.global_step == 3
    assert torch.equal(a.params.flat, b.params.flat)
    assert np.array_equal(bits(a.stft_mean), bits(b.stft_mean)) and np.array_equal(bits(a.stft_std), bits(b.stft_std))
