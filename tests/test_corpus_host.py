"""CPU: the corpus stays as stored (fp16) until the batch gather.  train.open_corpus memory-maps the npy files and returns the
statistics train.load_corpus computes; DeviceFeeder(norm=) hands out the batches load_corpus's standardised arrays give, bit for
bit; lib.corpus_batch refuses bad arguments before it calls the library."""
import numpy as np
import pytest
import torch

from tests.corpus_ref import bits, write_corpus


@pytest.mark.parametrize('dtype', [np.float16, np.float32])
def test_open_corpus_keeps_the_stored_dtype_and_load_corpus_statistics(tmp_path, dtype):
    from tacotron_amd import train
    stft, mel = write_corpus(tmp_path / 'c', dtype=dtype, speakers=3)
    assert train.open_corpus(str(tmp_path / 'nothing')) is None
    meta, data, norm = train.open_corpus(str(tmp_path / 'c'))
    meta0, data0, stft_mean, stft_std = train.load_corpus(str(tmp_path / 'c'))
    assert meta == meta0 and set(data) == set(data0)
    for k, stored in (('stft', stft), ('mel', mel)):
        assert isinstance(data[k], np.memmap) and data[k].dtype == dtype and np.array_equal(data[k], stored)
    for k in ('text', 'text_length', 'speaker'):
        assert data[k].dtype == np.int32 and np.array_equal(data[k], data0[k])
    assert set(norm) == {'stft', 'mel'} and all(a.dtype == np.float32 for pair in norm.values() for a in pair)
    assert np.array_equal(bits(norm['stft'][0]), bits(stft_mean)) and np.array_equal(bits(norm['stft'][1]), bits(stft_std))
    # load_corpus returns the stft pair only: the mel pair by its formula (the same seeded draw of 100 rows)
    m32 = mel.astype(np.float32)
    idx = np.random.default_rng(0).integers(len(m32), size=100)
    assert np.array_equal(bits(norm['mel'][0]), bits(m32[idx].mean((0, 1))))
    assert np.array_equal(bits(norm['mel'][1]), bits(m32[idx].std((0, 1))))
    # the map the feeders apply gives load_corpus's standardised arrays
    for k in ('stft', 'mel'):
        assert np.array_equal(bits((np.asarray(data[k]).astype(np.float32) - norm[k][0]) / norm[k][1]), bits(data0[k]))


def test_device_feeder_norm_on_the_cpu_matches_load_corpus(tmp_path):
    from tacotron_amd import train
    from tacotron_amd.data import DeviceFeeder
    write_corpus(tmp_path / 'c')
    _, data, norm = train.open_corpus(str(tmp_path / 'c'))
    _, data0, _, _ = train.load_corpus(str(tmp_path / 'c'))
    B = 5
    draws = [np.random.default_rng(40 + s).integers(12, size=B) for s in range(7)]
    feeder = DeviceFeeder(data, B, device='cpu', depth=2, draw=lambda step: draws[step] if step < 7 else draws[0], norm=norm)
    try:
        for s in range(7):
            batch = feeder.next()
            assert set(batch) == set(data0)
            for k in data0:
                got = batch[k].numpy()
                assert got.dtype == data0[k].dtype, k
                want = data0[k][draws[s]]
                assert np.array_equal(bits(got), bits(want)) if got.dtype == np.float32 else np.array_equal(got, want), (s, k)
    finally:
        feeder.close()
    with pytest.raises(ValueError, match='length'):
        DeviceFeeder(data, B, device='cpu', norm={'stft': (norm['stft'][0][:-1], norm['stft'][1][:-1])})


def test_device_feeder_without_norm_is_unchanged():
    """norm=None: the slots keep the dtype they are given and the tensors handed out are the device slots themselves."""
    from tacotron_amd.data import DeviceFeeder, synthetic_corpus
    corpus = synthetic_corpus(8, 6, 4, 2, 20, seed=3)
    feeder = DeviceFeeder(corpus, 3, device='cpu', depth=1, draw=lambda step: [step % 8, 1, 2])
    try:
        batch = feeder.next()
        assert batch is feeder._dev[0] and torch.equal(batch['stft'], corpus['stft'][[0, 1, 2]])
    finally:
        feeder.close()


def test_corpus_batch_width_rule(built_lib):
    w = built_lib.corpus_batch_width
    assert w(4096, 8192, 2050 * 4, True) == 8 and w(4096, 8192, 2050 * 4, False) == 4
    assert w(4096, 8192, 1025 * 4, True) == 4 and w(4096, 8192, 2050 * 3, True) == 2 and w(4096, 8192, 1025 * 3, True) == 1
    assert w(4096 + 2, 8192, 160, True) == 1 and w(4096 + 4, 8192, 160, True) == 2 and w(4096 + 8, 8192, 160, True) == 4
    assert w(4096, 8192 + 4, 160, True) == 1 and w(4096, 8192 + 8, 160, True) == 2 and w(4096, 8192 + 4, 160, False) == 1


def test_corpus_batch_refuses_bad_arguments_before_the_library(built_lib, monkeypatch):
    lib = built_lib

    def no_call(*a):
        raise AssertionError('the library was called')
    monkeypatch.setattr(lib, '_lib', type('NoLib', (), {'taco_corpus_batch': staticmethod(no_call)})())
    src = torch.zeros(5, 3, 14, dtype=torch.float16)
    mean, std = torch.zeros(14), torch.ones(14)
    with pytest.raises(ValueError, match='float16 or float32'):
        lib.corpus_batch(src.to(torch.bfloat16), mean, std)
    with pytest.raises(ValueError, match='float16 or float32'):
        lib.corpus_batch(src.double(), mean, std)
    with pytest.raises(ValueError, match='contiguous'):
        lib.corpus_batch(torch.zeros(5, 3, 28, dtype=torch.float16)[:, :, ::2], mean, std)
    with pytest.raises(ValueError, match='contiguous'):
        lib.corpus_batch(src.transpose(0, 1), mean, std)
    with pytest.raises(ValueError, match=r'mean must be .* shape \(14,\)'):
        lib.corpus_batch(src, torch.zeros(13), std)
    with pytest.raises(ValueError, match=r'std must be .* shape \(14,\)'):
        lib.corpus_batch(src, mean, torch.ones(7))
    with pytest.raises(ValueError, match='both'):
        lib.corpus_batch(src, mean, None)
    with pytest.raises(ValueError, match='index must be .* int64'):
        lib.corpus_batch(src, mean, std, index=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match=r'\(N, Td, C\)'):
        lib.corpus_batch(src.reshape(5, 42), mean, std)
    with pytest.raises(ValueError, match='GPU'):   # everything else right, but host memory: refused as well
        lib.corpus_batch(src, mean, std, index=torch.zeros(4, dtype=torch.int64))
