"""What a training batch costs to gather, before and after the corpus stays in HBM as stored: today's form, two torch.index_select
calls over the fp32 standardised corpus (stft and mel), against taco_corpus_batch twice over the fp16 corpus (the standardisation
inside the gather).  Nancy shape: B = 32, Td = 180, r = 2, a synthetic resident corpus of 512 utterances.

Both forms are timed with device events around --batches (>= 200) batches of fresh indices after warm-up, and ALTERNATE --reps
(>= 5) times in the one process; reported per batch: the median over the repetitions and their spread (max - min).  Two figures each:
  enqueued  the calls as the feeder makes them, timed from the first to the last: what the stream sees, including any stretch in
            which the host is the slower side (a batch is tens of microseconds of HBM time, a Python call is of the same order);
  device    the same calls enqueued behind a kernel that holds the stream for --hold-ms, so that they are all queued when the clock
            starts: the device's own time.
The bytes each form moves come from the shapes (old: fp32 read + fp32 written; new: fp16 read + fp32 written, statistics aside).
`not_slower` states the condition of the change: the new median does not exceed the old one by more than the spread between the
old form's own repetitions.

Then the upload: seconds per GB of DeviceCorpus's pageable chunked copy (fp32 array) against the pinned-staged one (fp16 array).

With --train-steps K (> 10) the train driver is run on a synthetic corpus written to a temporary directory, default against
corpus_fp32=True, alternated --train-reps times, and its own "ms/step" is recorded (driver loop = bench rate).

    python tools/corpus_batch_timing.py [--reps 7] [--batches 200] [--train-steps 300] [--out DIR]

Prints one JSON line; with --out also writes it to DIR/corpus_batch_timing.json.  No pass mark: exit status 0 unless a call fails."""
import argparse
import json
import os
import pickle as pkl
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tacotron_amd import lib  # noqa: E402
from tacotron_amd.data import DeviceCorpus  # noqa: E402

B, TD, R, N_UTT = 32, 180, 2, 512


def med_spread(v):
    return {'median': float(np.median(v)), 'spread': float(np.max(v) - np.min(v)), 'all': [float(x) for x in v]}


def time_batches(fn, indices, hold_ms):
    """ms per batch of fn(idx) over `indices`, between one pair of device events (behind a stream-holding kernel when hold_ms > 0)"""
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if hold_ms > 0:
        lib.debug_spin(1, 64, 0, int(hold_ms * 1000))
    s.record()
    for idx in indices:
        fn(idx)
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / len(indices)


def gather_timing(a, dev):
    rng = np.random.default_rng(7)
    widths = {'stft': 1025 * R, 'mel': 80 * R}
    half = {k: torch.from_numpy((rng.standard_normal((N_UTT, TD, w), dtype=np.float32) * 2.0 - 4.0).astype(np.float16)).to(dev)
            for k, w in widths.items()}
    norm = {k: (torch.from_numpy(rng.standard_normal(w, dtype=np.float32)).to(dev),
                torch.from_numpy(rng.uniform(0.5, 3.0, w).astype(np.float32)).to(dev)) for k, w in widths.items()}
    full = {k: lib.corpus_batch(v, *norm[k]) for k, v in half.items()}   # the fp32 standardised corpus of the old form
    indices = [torch.from_numpy(rng.integers(N_UTT, size=B)).to(dev) for _ in range(a.batches)]
    for k in widths:   # the two forms hand out the same batch
        assert torch.equal(torch.index_select(full[k], 0, indices[0]), lib.corpus_batch(half[k], *norm[k], index=indices[0])), k

    def old(idx):
        return [torch.index_select(full[k], 0, idx) for k in widths]

    def new(idx):
        return [lib.corpus_batch(half[k], *norm[k], index=idx) for k in widths]

    forms = {'index_select_fp32': old, 'corpus_batch_fp16': new}
    ts = {m: {k: [] for k in forms} for m in ('enqueued', 'device')}
    for _ in range(a.warmup):
        for fn in forms.values():
            time_batches(fn, indices, 0.0)
    for _ in range(a.reps):
        for mode, hold in (('enqueued', 0.0), ('device', a.hold_ms)):
            for k, fn in forms.items():
                ts[mode][k].append(time_batches(fn, indices, hold))
    row_elems = B * TD * sum(widths.values())
    nbytes = {'index_select_fp32': row_elems * 8, 'corpus_batch_fp16': row_elems * 6}
    out = {'bytes_per_batch': nbytes, 'unit': 'ms per batch'}
    for mode in ts:
        res = {k: med_spread(v) for k, v in ts[mode].items()}
        for k in res:
            res[k]['gb_per_s'] = nbytes[k] / (res[k]['median'] * 1e-3) / 1e9
        o, n = res['index_select_fp32'], res['corpus_batch_fp16']
        res['new_over_old'] = n['median'] / o['median']
        res['not_slower'] = bool(n['median'] - o['median'] <= o['spread'])
        out[mode] = res
    return out


def upload_timing(a, dev):
    rng = np.random.default_rng(8)
    x16 = (rng.standard_normal((N_UTT, TD, 1025 * R), dtype=np.float32) * 2.0 - 4.0).astype(np.float16)
    x32 = x16.astype(np.float32)
    stat = (np.zeros(1025 * R, np.float32), np.ones(1025 * R, np.float32))
    ts = {'pageable_chunked_fp32': [], 'pinned_staged_fp16': []}
    for _ in range(1 + a.upload_reps):   # (the first round is the warm-up)
        for k, make in (('pageable_chunked_fp32', lambda: DeviceCorpus({'stft': x32}, B, device=dev)),
                        ('pinned_staged_fp16', lambda: DeviceCorpus({'stft': x16}, B, device=dev, norm={'stft': stat}))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            c = make()
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t0) / (c.data['stft'].numel() * c.data['stft'].element_size() / 1e9))
            del c
    return {'unit': 's per GB uploaded (64-row chunks; the pinned form includes allocating its two staging chunks)',
            **{k: med_spread(v[1:]) for k, v in ts.items()}}


def train_timing(a):
    from tacotron_amd.config import Config
    from tacotron_amd.train import train
    rng = np.random.default_rng(9)
    n, Tt, V = 256, 200, 60
    res = {'steps': a.train_steps, 'unit': 'ms per step of the driver loop (its own report, steps 10..)', 'default': [], 'corpus_fp32': []}
    with tempfile.TemporaryDirectory() as d:
        np.save(os.path.join(d, 'stfts.npy'), (rng.standard_normal((n, TD, 1025 * R), dtype=np.float32) * 2.0 - 4.0).astype(np.float16))
        np.save(os.path.join(d, 'mels.npy'), (rng.standard_normal((n, TD, 80 * R), dtype=np.float32) * 2.0 - 3.0).astype(np.float16))
        lens = rng.integers(50, Tt + 1, size=n)
        text = rng.integers(1, V, size=(n, Tt))
        text[np.arange(Tt)[None, :] >= lens[:, None]] = 0
        np.save(os.path.join(d, 'texts.npy'), text)
        np.save(os.path.join(d, 'text_lens.npy'), lens)
        with open(os.path.join(d, 'meta.pkl'), 'wb') as f:
            pkl.dump({'r': R, 'vocab': {i: str(i) for i in range(V)}}, f)
        cwd = os.getcwd()
        os.chdir(d)   # (the driver writes under weights/ and log/)
        try:
            for _ in range(a.train_reps):
                for name, fp32 in (('default', False), ('corpus_fp32', True)):
                    c = Config()
                    c.batch_size, c.max_decode_iter, c.data_path, c.save_path = B, TD, d, 'timing'
                    m = train(c, num_steps=a.train_steps, log_every=10 ** 9, save_every=10 ** 9, corpus_fp32=fp32)
                    res[name].append(B * R * TD / m.host_loop_frames_per_s * 1e3)
                    del m
                    torch.cuda.empty_cache()
        finally:
            os.chdir(cwd)
    for name in ('default', 'corpus_fp32'):
        res[name] = med_spread(res[name])
    res['default_over_corpus_fp32'] = res['default']['median'] / res['corpus_fp32']['median']
    res['within_spread_of_corpus_fp32'] = bool(abs(res['default']['median'] - res['corpus_fp32']['median']) <= res['corpus_fp32']['spread'])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--batches', type=int, default=200)
    ap.add_argument('--hold-ms', type=float, default=40.0)
    ap.add_argument('--upload-reps', type=int, default=3)
    ap.add_argument('--train-steps', type=int, default=0)
    ap.add_argument('--train-reps', type=int, default=2)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'corpus_batch_timing needs a GPU'
    assert a.reps >= 5 and a.batches >= 200, 'at least 5 alternations of at least 200 batches'
    dev = torch.device('cuda', torch.cuda.current_device())
    res = {'tool': 'corpus_batch_timing', 'B': B, 'Td': TD, 'r': R, 'utterances': N_UTT, 'reps': a.reps, 'warmup': a.warmup,
           'batches': a.batches, 'hold_ms': a.hold_ms, 'version': lib.version(), 'device': torch.cuda.get_device_name(dev)}
    res['gather'] = gather_timing(a, dev)
    torch.cuda.empty_cache()
    res['upload'] = upload_timing(a, dev)
    torch.cuda.empty_cache()
    if a.train_steps > 10:
        res['train'] = train_timing(a)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, 'corpus_batch_timing.json'), 'w') as f:
            f.write(line + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
