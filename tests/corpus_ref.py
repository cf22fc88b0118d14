"""Shared by the corpus tests: a small corpus in tacotron_amd.preprocess's file format, and the NumPy statement of the map the
feeders apply, (x.astype(float32) - mean) / std, compared as bits."""
import pickle as pkl

import numpy as np


def write_corpus(path, N=12, Td=4, r=2, Tt=9, dtype=np.float16, seed=5, speakers=0):
    """A small corpus in tacotron_amd.preprocess's file format: log-magnitude-like values stored as `dtype`."""
    rng = np.random.default_rng(seed)
    path.mkdir(parents=True, exist_ok=True)
    stft = (rng.standard_normal((N, Td, 1025 * r)) * 2.5 - 4.0).astype(dtype)
    mel = (rng.standard_normal((N, Td, 80 * r)) * 2.0 - 3.0).astype(dtype)
    lens = rng.integers(3, Tt + 1, size=N)
    text = rng.integers(1, 20, size=(N, Tt))
    text[np.arange(Tt)[None, :] >= lens[:, None]] = 0
    np.save(path / 'stfts.npy', stft)
    np.save(path / 'mels.npy', mel)
    np.save(path / 'texts.npy', text)
    np.save(path / 'text_lens.npy', lens)
    if speakers:
        np.save(path / 'speakers.npy', rng.integers(0, speakers, size=N))
    with open(path / 'meta.pkl', 'wb') as f:
        pkl.dump({'r': r, 'vocab': {i: chr(96 + i) for i in range(20)}}, f)
    return stft, mel


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def standardise(x, mean=None, std=None):
    """What taco_corpus_batch computes for the rows of x: the widening alone, or NumPy's fp32 (x - mean) / std."""
    x = np.asarray(x).astype(np.float32)
    return x if mean is None else (x - mean) / std
