"""preprocess.py -- builds data/<set>/ from a downloaded corpus, the first step of the reference's workflow (README "Usage",
preprocess.py): `python -m tacotron_amd.preprocess {nancy,arctic,vctk} [--data-dir data/]`.

The listing functions restate prepare_arctic / prepare_nancy / prepare_vctk (preprocess.py:42-123) with the same file layouts
and text slicing (VCTK's speaker table is read without pandas).  The vocabulary grows in first-seen order over ALL prompts,
dropped utterances included (preprocess.py:130-135, data.Vocab).  The features are audio.process_audio on the GPU
(csrc/features.hip) for batches of 64 utterances, read by a small thread pool; fp16 results leave the device through pinned
buffers into np.lib.format.open_memmap arrays, so host memory does not grow with the corpus (Nancy's stfts.npy is ~9 GB).

Written, as train.load_corpus reads them: texts.npy (pad_to_dense), text_lens.npy, mels.npy (N, Td, 80 r) and stfts.npy
(N, Td, 1025 r) in float16, speech_lens.npy, meta.pkl = {'vocab': ivocab, 'r': r, 'sr': sr} (pickle protocol 2) and, for VCTK,
speakers.npy.  Differences from the reference, on purpose:
  - speakers.npy holds the speakers of the KEPT utterances; the reference saved one per listed utterance (preprocess.py:202-203),
    which misaligns it with the other arrays as soon as one utterance is dropped;
  - meta.pkl records the rate the corpus was read at; the reference's save_vocab(name) left it at its default of 16000 for VCTK;
  - WAV files are read with the standard library's `wave`.  With resample='host' (the default) audio.load_wav decodes on the reader
    threads and resamples a file of another rate with scipy's resample_poly -- a polyphase FIR with scipy's own Kaiser design,
    NOT the reference's filter; with resample='device' (--resample device) the reader threads hand over the files' bytes and the
    GPU decodes and resamples them (audio.load_batch_device, taco_wave_resample) with resampy's 'kaiser_best' windowed sinc, the
    filter behind the reference's librosa.load, and scipy is not needed.  Only VCTK (48 kHz files read at 24 kHz) is resampled;
    for a corpus stored at its own rate both paths decode to the same bits.
"""
from __future__ import annotations

import argparse
import glob
import os
import pickle as pkl
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import audio
from .data import Vocab, pad_to_dense

BATCH = 64


def prepare_arctic(data_dir):
    """preprocess.prepare_arctic: lines `( arctic_a0001 "Author of the danger trail." )` of arctic/etc/arctic.data."""
    prompts, audio_files = [], []
    with open(os.path.join(data_dir, 'arctic', 'etc', 'arctic.data')) as tff:
        for line in tff:
            spl = line.split()
            text = ' '.join(spl[2:-1])[1:-1]
            prompts.append(text)
            audio_files.append(os.path.join(data_dir, 'arctic', 'wav', '%s.wav' % spl[1]))
    return {'prompts': prompts, 'audio_files': audio_files}


def prepare_nancy(data_dir):
    """preprocess.prepare_nancy: lines `( nancy001 "Text." )` of nancy/prompts.data; the text slice ends one character before the
    last quote (`rfind('"') - 1`), as the reference's does."""
    prompts, audio_files = [], []
    with open(os.path.join(data_dir, 'nancy', 'prompts.data')) as ttf:
        for line in ttf:
            uid = line.split()[1]
            prompts.append(line[line.find('"') + 1:line.rfind('"') - 1])
            audio_files.append(os.path.join(data_dir, 'nancy', 'wavn', uid + '.wav'))
    return {'prompts': prompts, 'audio_files': audio_files}


def _vctk_speaker_ids(path):
    """The ID column of vctk/speaker-info.txt (whitespace separated, header row), as pandas.read_table(usecols=['ID'])."""
    with open(path) as f:
        rows = [ln.split() for ln in f if ln.strip()]
    col = rows[0].index('ID')
    return [r[col] for r in rows[1:] if len(r) > col]


def prepare_vctk(data_dir):
    """preprocess.prepare_vctk: speakers in speaker-info.txt order get ids 0, 1, ...; per speaker the sorted vctk/txt/p<ID>/*.txt
    give the utterances (text stripped) and vctk/wav48/p<ID>/<utt>.wav the audio."""
    ids = _vctk_speaker_ids(os.path.join(data_dir, 'vctk', 'speaker-info.txt'))
    speaker_ids = {uid: i for i, uid in enumerate(ids)}
    file_ids = []
    for uid in ids:
        file_ids.extend(os.path.basename(f)[:-4] for f in sorted(glob.glob(os.path.join(data_dir, 'vctk', 'txt', 'p%s' % uid, '*.txt'))))
    prompts, audio_files, speakers = [], [], []
    for f in file_ids:
        with open(os.path.join(data_dir, 'vctk', 'txt', f[:4], f + '.txt')) as tff:
            prompts.append(tff.read().strip())
        audio_files.append(os.path.join(data_dir, 'vctk', 'wav48', f[:4], f + '.wav'))
        speakers.append(speaker_ids[f[1:4]])
    return {'prompts': prompts, 'audio_files': audio_files, 'speakers': speakers}


prepare_functions = {'arctic': prepare_arctic, 'nancy': prepare_nancy, 'vctk': prepare_vctk}


def _reader_threads():
    """At most 16 file readers, fewer when OMP_NUM_THREADS says so (not os.cpu_count(): a shared host's core count is not ours)."""
    try:
        n = int(os.environ.get('OMP_NUM_THREADS', '16'))
    except ValueError:
        n = 16
    return max(1, min(16, n))


def _truncate_npy(path, rows):
    """Shrink an .npy file written through open_memmap to its first `rows` rows: rewrite the shape in the header (same length,
    space padded) and cut the data."""
    with open(path, 'r+b') as f:
        version = np.lib.format.read_magic(f)
        read = np.lib.format.read_array_header_1_0 if version == (1, 0) else np.lib.format.read_array_header_2_0
        shape, fortran, dtype = read(f)
        offset = f.tell()
        new_shape = (rows,) + tuple(shape[1:])
        hdr = "{'descr': %r, 'fortran_order': %r, 'shape': %r, }" % (np.lib.format.dtype_to_descr(dtype), fortran, new_shape)
        prefix = 8 + (2 if version == (1, 0) else 4)
        room = offset - prefix
        assert len(hdr) + 1 <= room, 'npy header grew'
        f.seek(prefix)
        f.write((hdr + ' ' * (room - len(hdr) - 1) + '\n').encode('latin1'))
        f.truncate(offset + rows * int(np.prod(new_shape[1:], dtype=np.int64)) * dtype.itemsize)


RESAMPLE_PATHS = ('host', 'device')


def preprocess(data, out_dir, sr=16000, r=2, max_len=audio.MAXIMUM_AUDIO_LENGTH, batch=BATCH, verbose=True, resample='host'):
    """preprocess.preprocess (preprocess.py:161-204) with the features from the GPU.  resample: where the files are decoded and
    brought to `sr` -- 'host' (audio.load_wav) or 'device' (audio.load_batch_device: resampy's kaiser_best filter).  Returns the
    number of kept utterances."""
    import torch

    if resample not in RESAMPLE_PATHS:
        raise ValueError('preprocess: resample must be one of %s, got %r' % (', '.join(RESAMPLE_PATHS), resample))

    os.makedirs(out_dir, exist_ok=True)
    prompts, files = data['prompts'], data['audio_files']
    n = len(prompts)
    vocab = Vocab()
    encoded = [np.array(vocab.encode(p)) for p in prompts]   # every prompt, dropped ones too (first-seen order)
    Td = ((1 + max_len // 300) // (4 * r)) * 4
    mels = np.lib.format.open_memmap(os.path.join(out_dir, 'mels.npy'), 'w+', np.float16, (n, Td, 80 * r))
    stfts = np.lib.format.open_memmap(os.path.join(out_dir, 'stfts.npy'), 'w+', np.float16, (n, Td, 1025 * r))
    pin = torch.cuda.is_available()
    h_mel = torch.empty(batch, Td, 80 * r, dtype=torch.float16, pin_memory=pin)
    h_stft = torch.empty(batch, Td, 1025 * r, dtype=torch.float16, pin_memory=pin)
    kept_idx = []
    count = 0
    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=_reader_threads()) as pool:
        if resample == 'device':
            load = lambda lo: [pool.submit(audio.read_wav_raw, f) for f in files[lo:lo + batch]]   # noqa: E731
        else:
            load = lambda lo: [pool.submit(audio.load_wav, f, sr) for f in files[lo:lo + batch]]   # noqa: E731
        pending = load(0)
        for lo in range(0, n, batch):
            waves = [fut.result() for fut in pending]
            pending = load(lo + batch) if lo + batch < n else []   # the next batch is read while this one runs on the GPU
            nb = len(waves)
            lengths = None
            if resample == 'device':
                waves, lengths = audio.load_batch_device(waves, sr)
            mel, stft, kept, _ = audio.process_audio(waves, lengths, r, max_len, torch.float16)
            h_mel[:nb].copy_(mel, non_blocking=True)
            h_stft[:nb].copy_(stft, non_blocking=True)
            k = kept.cpu().numpy()                          # (synchronises the stream: the pinned copies are complete)
            rows = np.flatnonzero(k)
            if len(rows):
                mels[count:count + len(rows)] = h_mel.numpy()[rows]
                stfts[count:count + len(rows)] = h_stft.numpy()[rows]
            kept_idx.extend(lo + rows)
            count += len(rows)
            if verbose:
                print('%d / %d utterances, %d kept, %.1f utt/s' % (lo + nb, n, count, (lo + nb) / (time.perf_counter() - t0)))
    mels.flush()
    stfts.flush()
    del mels, stfts
    if count == 0:
        raise RuntimeError('no utterance is at most %d samples long after trimming' % max_len)
    for name in ('mels', 'stfts'):
        _truncate_npy(os.path.join(out_dir, name + '.npy'), count)
    texts = [encoded[i] for i in kept_idx]
    out = {'texts': pad_to_dense(texts), 'text_lens': np.array([len(t) for t in texts]),
           'speech_lens': np.full(count, Td, dtype=np.int64)}
    if 'speakers' in data:
        out['speakers'] = np.asarray(data['speakers'])[np.asarray(kept_idx, dtype=np.int64)]
    for name, arr in out.items():
        np.save(os.path.join(out_dir, name + '.npy'), arr, allow_pickle=False)
    with open(os.path.join(out_dir, 'meta.pkl'), 'wb') as vf:
        pkl.dump({'vocab': vocab.ivocab, 'r': r, 'sr': sr}, vf, protocol=2)
    if verbose:
        for name in ('texts', 'text_lens', 'mels', 'stfts', 'speech_lens') + (('speakers',) if 'speakers' in out else ()):
            print(os.path.join(out_dir, name), np.load(os.path.join(out_dir, name + '.npy'), mmap_mode='r').shape)
    return count


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description='Preprocess a corpus into data/<set>/ (features on the GPU)')
    ap.add_argument('dataset', help='name of the dataset to preprocess: ' + ', '.join(sorted(prepare_functions)))
    ap.add_argument('--data-dir', default='data/')
    ap.add_argument('--r', type=int, default=2, help='decoder frames per step (audio.r)')
    ap.add_argument('--resample', choices=RESAMPLE_PATHS, default='host',
                    help="where WAV files are decoded and resampled: 'host' (scipy's resample_poly) or 'device' (the GPU, with "
                         "resampy's kaiser_best filter, the reference's)")
    return ap.parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    if a.dataset not in prepare_functions:
        raise NotImplementedError('No prepare function exists for the %s dataset' % a.dataset)
    sr = 24000 if a.dataset == 'vctk' else 16000
    data = prepare_functions[a.dataset](a.data_dir)
    return preprocess(data, os.path.join(a.data_dir, a.dataset), sr=sr, r=a.r, resample=a.resample)


if __name__ == '__main__':
    main()
