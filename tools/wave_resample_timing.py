"""Wall time of bringing one batch of VCTK-shaped files to the corpus rate: 64 utterances, 48 kHz, PCM16 mono, about 4 s each, read at
24 kHz (what `python -m tacotron_amd.preprocess vctk` does per batch), on the two paths of preprocess(..., resample=...):

  host    audio.load_wav on the reader threads (decode + scipy.signal.resample_poly), the batch packed into one fp32 array and uploaded
          -- what preprocess(resample='host') does up to process_audio's first kernel;
  device  audio.read_wav_raw on the reader threads, then audio.load_batch_device: the raw bytes packed, uploaded, and one
          taco_wave_resample call (decode + resampy's kaiser_best filter);
  kernel  taco_wave_resample alone on the uploaded bytes: one call between two events, and per call of 20 back to back.

host and device are host-clock times around work that ends in a device synchronise (files in the page cache; the two alternate
inside each repetition, medians); kernel times come from device events.  The two paths apply different filters, so their results
differ on purpose; the relative L2 difference is recorded, not judged.

    python tools/wave_resample_timing.py [--reps 10] [--warmup 2] [--out DIR]

Prints one JSON line; with --out also writes it to DIR/wave_resample_timing.json.  No pass mark: the exit status is 0 unless a call fails."""
import argparse
import json
import os
import sys
import tempfile
import time
import wave as wavefile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tacotron_amd import audio, lib, preprocess  # noqa: E402
from tools.griffinlim_timing import alternate  # noqa: E402

B, SR_FILE, SR, SECONDS, BURST = 64, 48000, 24000, 4.0, 20


def write_files(folder):
    """64 seeded speech-band signals of 3.5 .. 4.5 s: a few drifting tones under an envelope plus a little noise"""
    rng = np.random.default_rng(48)
    paths = []
    for i in range(B):
        n = int(SR_FILE * rng.uniform(SECONDS - 0.5, SECONDS + 0.5))
        t = np.arange(n) / SR_FILE
        x = sum(a * np.sin(2 * np.pi * f * t * (1 + 0.02 * np.sin(2 * np.pi * 0.7 * t)) + p)
                for a, f, p in zip((0.3, 0.2, 0.1, 0.05), rng.uniform(100, 6000, 4), rng.uniform(0, 6, 4)))
        x = x * (0.6 + 0.4 * np.sin(2 * np.pi * 3.1 * t)) + 0.01 * rng.standard_normal(n)
        path = os.path.join(folder, 'u%02d.wav' % i)
        with wavefile.open(path, 'wb') as f:
            f.setnchannels(1)
            f.setsampwidth(2)
            f.setframerate(SR_FILE)
            f.writeframes(np.round(np.clip(x, -1, 1) * 32767.0).astype('<i2').tobytes())
        paths.append(path)
    return paths


def wall(fns, reps, warmup):
    """{name: median ms} on the host clock; every callable ends in its own device synchronise; they alternate inside a repetition"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[k].append(1e3 * (time.perf_counter() - t0))
    return {k: float(np.median(v)) for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'wave_resample_timing needs a GPU'
    threads = preprocess._reader_threads()
    keep = {}
    with tempfile.TemporaryDirectory() as folder, ThreadPoolExecutor(max_workers=threads) as pool:
        paths = write_files(folder)

        def host_path():
            waves = list(pool.map(lambda p: audio.load_wav(p, SR), paths))
            packed = np.zeros((B, max(len(w) for w in waves)), dtype=np.float32)
            for i, w in enumerate(waves):
                packed[i, :len(w)] = w
            keep['host'] = (torch.from_numpy(packed).to('cuda'), [len(w) for w in waves])

        def device_path():
            keep['device'] = audio.load_batch_device(list(pool.map(audio.read_wav_raw, paths)), SR)

        res = {'tool': 'wave_resample_timing', 'B': B, 'sr_file': SR_FILE, 'sr': SR, 'reader_threads': threads, 'reps': a.reps,
               'warmup': a.warmup, 'version': lib.version(), 'tile': lib.WAVE_RESAMPLE_TILE,
               'unit': 'ms per batch (median; host and device alternate inside each repetition)'}
        res.update(wall({'host_path': host_path, 'device_path': device_path}, a.reps, a.warmup))
        # the kernel alone, on the bytes the device path uploads
        raws = [audio.read_wav_raw(p) for p in paths]
    frames = [r[4] for r in raws]
    counts = [audio.resample_lengths(n, SR_FILE, SR) for n in frames]
    P, Q, n_left, n_right, table = audio.resample_filter(SR_FILE, SR)
    host = np.zeros((B, 2 * max(frames)), dtype=np.uint8)
    for i, r in enumerate(raws):
        host[i, :len(r[0])] = r[0]
    pcm = torch.from_numpy(host).to('cuda')
    rows = torch.tensor([[n, c[0]] for n, c in zip(frames, counts)], dtype=torch.int32, device='cuda')
    taps = torch.from_numpy(table.astype(np.float32)).to('cuda')
    out = torch.empty(B, max(c[1] for c in counts), device='cuda')

    def kernel():
        lib.wave_resample(pcm, rows, taps, 2, 1, P, Q, n_left, n_right, out=out)

    def kernel_burst():
        for _ in range(BURST):
            kernel()

    k = alternate({'taco_wave_resample': kernel, 'burst': kernel_burst}, max(a.reps, 20), a.warmup + 1)
    res['taco_wave_resample'] = k['taco_wave_resample']
    res['taco_wave_resample_steady'] = k['burst'] / BURST
    torch.cuda.synchronize()
    dw, dl = keep['device']
    hw, hl = keep['host']
    assert dl == hl == [c[1] for c in counts] and torch.equal(dw, out)
    d = (dw.double() - hw.double())
    fma = float(sum(c[0] for c in counts)) * (n_left + n_right)
    res.update({'frames_mean': float(np.mean(frames)), 'samples_out_mean': float(np.mean(dl)), 'taps': n_left + n_right,
                'upload_bytes_host_path': int(hw.numel() * 4), 'upload_bytes_device_path': int(host.size),
                'device_over_host': res['device_path'] / res['host_path'],
                'kernel_gflop_per_s_steady': 2.0 * fma / (res['taco_wave_resample_steady'] * 1e-3) / 1e9,
                'rel_l2_device_vs_host': float(d.norm() / hw.double().norm())})
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, 'wave_resample_timing.json'), 'w') as f:
            f.write(line + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
