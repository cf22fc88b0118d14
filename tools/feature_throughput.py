"""Throughput of the feature front end (csrc/features.hip) on the GPU: utterances per second kernel-only (device events around
taco_audio_features on batches already in HBM) and end to end (tacotron_amd.preprocess on a synthetic Nancy-format corpus of
16-bit WAV files written to a temporary directory: file reads, upload, kernel, fp16 download, memmap writes).

    python tools/feature_throughput.py [--utts 512] [--batch 64] [--out DIR]

Prints one JSON line; with --out also writes it to DIR/feature_throughput.json."""
import argparse
import json
import os
import sys
import tempfile
import time
import wave

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')

import torch  # noqa: E402

from tacotron_amd import audio, preprocess  # noqa: E402


def _utterance(rng, n):
    t = np.arange(n) / 16000.0
    f0 = rng.uniform(90, 250)
    y = sum(0.25 / k * np.sin(2 * np.pi * k * f0 * t + rng.uniform(0, 6.3)) for k in range(1, 16))
    return (y + 0.01 * rng.standard_normal(n)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--utts', type=int, default=512)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'feature_throughput needs a GPU'
    rng = np.random.default_rng(0)
    lens = rng.integers(24000, 100000, size=a.utts)            # 1.5 .. 6.25 s at 16 kHz (Nancy-like)
    waves = [_utterance(rng, int(n)) for n in lens]

    # kernel only: batches resident on the device, fp16 outputs
    dev_batches = []
    for lo in range(0, a.utts, a.batch):
        chunk = waves[lo:lo + a.batch]
        host = np.zeros((len(chunk), max(len(w) for w in chunk)), np.float32)
        for i, w in enumerate(chunk):
            host[i, :len(w)] = w
        dev_batches.append((torch.from_numpy(host).cuda(), [len(w) for w in chunk]))
    for wv, ln in dev_batches[:2]:
        audio.process_audio(wv, ln, 2)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 3
    s.record()
    for _ in range(reps):
        for wv, ln in dev_batches:
            audio.process_audio(wv, ln, 2)
    e.record()
    torch.cuda.synchronize()
    kernel_s = s.elapsed_time(e) / 1e3 / reps
    kernel_ups = a.utts / kernel_s

    # end to end through the CLI's pipeline
    with tempfile.TemporaryDirectory() as d:
        wd = os.path.join(d, 'nancy', 'wavn')
        os.makedirs(wd)
        with open(os.path.join(d, 'nancy', 'prompts.data'), 'w') as f:
            for i, w in enumerate(waves):
                f.write('( nancy%05d "utterance number %d." )\n' % (i, i))
                with wave.open(os.path.join(wd, 'nancy%05d.wav' % i), 'wb') as wf:
                    wf.setnchannels(1)
                    wf.setsampwidth(2)
                    wf.setframerate(16000)
                    wf.writeframes(np.clip(np.round(w * 32767), -32768, 32767).astype('<i2').tobytes())
        data = preprocess.prepare_nancy(d)
        t0 = time.perf_counter()
        kept = preprocess.preprocess(data, os.path.join(d, 'nancy'), sr=16000, r=2, batch=a.batch, verbose=False)
        e2e_s = time.perf_counter() - t0
    res = {'metric': 'feature_throughput', 'utterances': a.utts, 'batch': a.batch, 'kept': int(kept),
           'mean_seconds_of_audio': float(lens.mean() / 16000.0),
           'kernel_only_utt_per_s': round(kernel_ups, 1), 'kernel_only_ms_per_batch': round(kernel_s / len(dev_batches) * 1e3, 3),
           'end_to_end_utt_per_s': round(a.utts / e2e_s, 1), 'reader_threads': preprocess._reader_threads()}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, 'feature_throughput.json'), 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
