"""Wall time of the loudness call (taco_wave_loudness: K-weighting, hop sums, gates, gain, fp32 / PCM16 emit) next to the finishing call
in front of it, a device-to-device copy of the same bytes and the host path it replaces, at two shapes: 32 x 107,700 samples (one
S1 inference batch: F = 360 frames) and 8 x 480,000 (joined long prompts of 30 s).

In the manner of tools/wave_finish_timing.py: every variant is timed with device events around one call, the variants ALTERNATE inside
each repetition and the median over --reps repetitions is reported.  The rotation:
  taco_wave_finish (de-emphasis 0.97, no trim, fp32 out) on a fixed waveform: the call in front;
  taco_wave_loudness on its output, measure-only / with out / with pcm / with both, one call each;
  taco_wave_loudness with pcm, 20 calls back to back between one pair of events, per call (the steady rate: a single call carries the
  launch latency of an idle queue);
  a device-to-device copy of the B x L floats.
The host path -- copy the rows back, then the fp64 restatement of tests/loudness_ref.py (scipy's lfilter) row by row -- is timed with
the host's clock, --host-reps times, median.  The input is noise under a slow envelope at about -25 LUFS, so the gain is a real one.
Recorded next to the medians: the ratios to the finishing call and to the copy.  No time is fixed in advance.

    python tools/wave_loudness_timing.py [--reps 20] [--warmup 3] [--host-reps 3] [--out DIR]

Prints one JSON line; with --out also writes it to DIR/wave_loudness_timing.json.  No pass mark: the exit status is 0 unless a call fails."""
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
from tests import loudness_ref  # noqa: E402
from tools.griffinlim_timing import alternate  # noqa: E402

SR, TARGET, CEILING, DEEMPH, BURST = 16000, -23.0, 10.0 ** (-1.0 / 20.0), 0.97, 20
SHAPES = ((32, 107700), (8, 480000))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--host-reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'wave_loudness_timing needs a GPU'
    dev = torch.device('cuda', torch.cuda.current_device())
    res = {'tool': 'wave_loudness_timing', 'sr': SR, 'target_lufs': TARGET, 'ceiling': CEILING, 'deemphasis': DEEMPH, 'reps': a.reps,
           'warmup': a.warmup, 'host_reps': a.host_reps, 'version': lib.version(), 'chunk': lib.LOUD_CHUNK,
           'unit': 'ms per call (median; device variants alternate inside each repetition; host_path by the host clock)', 'rows': [],
           'checks': []}
    for B, L in SHAPES:
        g = torch.Generator(device='cpu').manual_seed(B)
        env = 0.5 + 0.5 * torch.sin(2.0 * np.pi * 0.7 * torch.arange(L) / SR)
        raw = (0.02 * torch.randn((B, L), generator=g) * env).to(dev)
        fin = torch.empty(B, L, device=dev)
        bounds = torch.empty(B, 2, dtype=torch.int32, device=dev)
        peak = torch.empty(B, device=dev)
        work_fin = torch.empty(lib.wave_finish_workspace_floats(B, L), device=dev)
        out = torch.empty(B, L, device=dev)
        pcm = torch.empty(B, L, dtype=torch.int16, device=dev)
        loud = torch.empty(B, 4, device=dev)
        blocks = torch.empty(B, 4, dtype=torch.int32, device=dev)
        work = torch.empty(lib.wave_loudness_workspace_floats(B, L, SR), device=dev)
        copy = torch.empty(B, L, device=dev)

        def finish():
            lib.wave_finish(raw, None, deemphasis=DEEMPH, trim_top_db=0.0, want_pcm=False, out=fin, bounds=bounds, peak=peak, work=work_fin)

        def level(o, p):
            if o is None and p is None:
                return lambda: lib.wave_loudness(fin, None, sr=SR, loud=loud, blocks=blocks, work=work)
            return lambda: lib.wave_loudness(fin, None, sr=SR, target=TARGET, ceiling=CEILING, want_out=o is not None, want_pcm=p is not None,
                                             out=o, pcm=p, loud=loud, blocks=blocks, work=work)

        with_pcm = level(None, pcm)

        def burst():
            for _ in range(BURST):
                with_pcm()

        finish()
        fns = {'taco_wave_finish': finish, 'loudness_measure': level(None, None), 'loudness_out': level(out, None), 'loudness_pcm': with_pcm,
               'loudness_out_pcm': level(out, pcm), 'loudness_pcm_x%d' % BURST: burst, 'copy_d2d': lambda: copy.copy_(fin)}
        row = {'B': B, 'L': L}
        row.update(alternate(fns, a.reps, a.warmup))
        row['loudness_pcm_steady'] = row.pop('loudness_pcm_x%d' % BURST) / BURST
        torch.cuda.synchronize()
        row['I_mean'] = float(loud[:, 0].mean())
        row['gain_db_mean'] = float((20.0 * torch.log10(loud[:, 2])).mean())
        row['limited_rows'] = int(blocks[:, 3].sum())
        host = []
        for _ in range(a.host_reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rows = fin.cpu().numpy()
            got = [loudness_ref.level(r, SR, TARGET, CEILING) for r in rows]
            host.append((time.perf_counter() - t0) * 1e3)
        row['host_path'] = float(np.median(host))
        row['host_I_mean'] = float(np.mean([r['I'] for r in got]))
        res['rows'].append(row)
        res['checks'].append({'B': B, 'L': L,
                              'over_wave_finish': {k: row[k] / row['taco_wave_finish'] for k in
                                                   ('loudness_measure', 'loudness_out', 'loudness_pcm', 'loudness_out_pcm', 'loudness_pcm_steady')},
                              'over_copy_d2d': {k: row[k] / row['copy_d2d'] for k in ('loudness_measure', 'loudness_pcm', 'loudness_pcm_steady')},
                              'host_path_over_loudness_pcm': row['host_path'] / row['loudness_pcm'],
                              'bytes_read_once': 4.0 * B * L})
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, 'wave_loudness_timing.json'), 'w') as f:
            f.write(line + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
