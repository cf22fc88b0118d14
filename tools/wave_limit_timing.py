"""Wall time of the true-peak limiter (taco_wave_limit: envelope through the polyphase interpolator, required gain, sliding minimum,
smoothing, fp32 / PCM16 emit) next to the loudness call it follows, a device-to-device copy of the same floats and the host path it
replaces, at two shapes: 32 x 107,700 samples (one S1 inference batch at 16 kHz) and 8 x 480,000 (10 s rows at 48 kHz).

In the manner of tools/wave_loudness_timing.py: every variant is timed with device events around one call, the variants ALTERNATE
inside each repetition and the median over --reps repetitions is reported, all in the same run.  The rotation:
  taco_wave_limit measure-only (the dBTP meter; P = 4, T = 12);
  taco_wave_limit with pcm and with out and pcm, at W = 24 and at W = 72 (1.5 ms at 16 and at 48 kHz);
  taco_wave_limit with out being the wave itself at W = 24 (the third launch: the halo copy), on a scratch copy of the rows;
  taco_wave_loudness with pcm on the same rows;
  a device-to-device copy of the B x L floats.
The host path -- copy the rows back, then the float32 restatement of tests/limiter_ref.py row by row at W = 24 -- is timed with the
host's clock, --host-reps times, median.  The input is noise under a slow envelope with a gain of 26 dB against a ceiling of -1 dB,
so that about 30 per cent of the samples are limited.  Recorded next to the medians: the ratios to the loudness call and to the copy.
No time is fixed in advance.

    python tools/wave_limit_timing.py [--reps 20] [--warmup 3] [--host-reps 2] [--out DIR]

Prints one JSON line; with --out also writes it to DIR/wave_limit_timing.json.  No pass mark: the exit status is 0 unless a call fails."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tacotron_amd import lib  # noqa: E402
from tests import limiter_ref  # noqa: E402
from tools.griffinlim_timing import alternate  # noqa: E402

TARGET, CEILING, GAIN = -23.0, 10.0 ** (-1.0 / 20.0), 20.0
SHAPES = ((32, 107700, 16000), (8, 480000, 48000))
WS = (24, 72)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--host-reps', type=int, default=2)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'wave_limit_timing needs a GPU'
    dev = torch.device('cuda', torch.cuda.current_device())
    res = {'tool': 'wave_limit_timing', 'ceiling': CEILING, 'gain': GAIN, 'P': lib.LIMIT_P, 'T': lib.LIMIT_T, 'beta': lib.LIMIT_BETA,
           'reps': a.reps, 'warmup': a.warmup, 'host_reps': a.host_reps, 'version': lib.version(), 'chunk': lib.LIMIT_CHUNK,
           'unit': 'ms per call (median; device variants alternate inside each repetition; host_path by the host clock)', 'rows': [],
           'checks': []}
    taps_host = lib.true_peak_taps()
    taps = torch.from_numpy(taps_host).to(dev)
    for B, L, sr in SHAPES:
        g = torch.Generator(device='cpu').manual_seed(B)
        env = 0.5 + 0.5 * torch.sin(2.0 * np.pi * 0.7 * torch.arange(L) / sr)
        fin = (0.02 * torch.randn((B, L), generator=g) * env).to(dev)
        gain = torch.full((B,), GAIN, device=dev)
        out = torch.empty(B, L, device=dev)
        pcm = torch.empty(B, L, dtype=torch.int16, device=dev)
        peaks = torch.empty(B, 4, device=dev)
        counts = torch.empty(B, 2, dtype=torch.int32, device=dev)
        work = torch.empty(lib.wave_limit_workspace_floats(B, L, max(WS)), device=dev)
        loud = torch.empty(B, 4, device=dev)
        blocks = torch.empty(B, 4, dtype=torch.int32, device=dev)
        work_loud = torch.empty(lib.wave_loudness_workspace_floats(B, L, sr), device=dev)
        copy = torch.empty(B, L, device=dev)
        scratch = fin.clone()   # (limited in place over and over: its values drift under the ceiling, its time does not depend on them)
        windows = {W: torch.from_numpy(lib.limit_window(W)).to(dev) for W in WS}

        def limit(W, o, p, x=fin):
            wk = work[:lib.wave_limit_workspace_floats(B, L, W)]
            return lambda: lib.wave_limit(x, None, gain, ceiling=CEILING, taps=taps, window=windows[W], out=o, pcm=p, peaks=peaks,
                                          counts=counts, work=wk)

        work0 = work[:lib.wave_limit_workspace_floats(B, L, 0)]
        fns = {'limit_measure': lambda: lib.wave_limit(fin, None, taps=taps, peaks=peaks, counts=counts, work=work0)}
        for W in WS:
            fns['limit_pcm_w%d' % W] = limit(W, None, pcm)
            fns['limit_out_pcm_w%d' % W] = limit(W, out, pcm)
        fns['limit_in_place_w%d' % WS[0]] = limit(WS[0], scratch, None, scratch)
        fns['loudness_pcm'] = lambda: lib.wave_loudness(fin, None, sr=sr, target=TARGET, ceiling=CEILING, want_out=False, pcm=pcm, loud=loud,
                                                        blocks=blocks, work=work_loud)
        fns['copy_d2d'] = lambda: copy.copy_(fin)
        row = {'B': B, 'L': L, 'sr': sr}
        row.update(alternate(fns, a.reps, a.warmup))
        limit(WS[0], out, pcm)()
        torch.cuda.synchronize()
        row['limited_share'] = float(counts[:, 1].sum()) / float(counts[:, 0].sum())
        row['g_min_db'] = float(20.0 * torch.log10(peaks[:, 2].min()))
        host = []
        win = lib.limit_window(WS[0])
        for _ in range(a.host_reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rows = fin.cpu().numpy()
            got = [limiter_ref.limit(r, GAIN, CEILING, taps_host, win) for r in rows]
            host.append((time.perf_counter() - t0) * 1e3)
        row['host_path_w%d' % WS[0]] = float(np.median(host))
        row['host_equals_device'] = bool(np.array_equal(np.stack([r['pcm'] for r in got]), pcm.cpu().numpy()))
        res['rows'].append(row)
        keys = [k for k in row if k.startswith('limit_') and k != 'limited_share']
        res['checks'].append({'B': B, 'L': L, 'over_loudness_pcm': {k: row[k] / row['loudness_pcm'] for k in keys},
                              'over_copy_d2d': {k: row[k] / row['copy_d2d'] for k in keys},
                              'host_path_over_limit_pcm': row['host_path_w%d' % WS[0]] / row['limit_pcm_w%d' % WS[0]],
                              'bytes_read_once': 4.0 * B * L})
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, 'wave_limit_timing.json'), 'w') as f:
            f.write(line + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
