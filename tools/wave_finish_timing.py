"""Wall time of waveform finishing (taco_wave_finish: de-emphasis 0.97, trim at 40 dB, fp32 and PCM16 outputs) next to the vocoder
call it follows, at the flagship inference shape: F = 360 frames, L = 300 (F - 1) = 107,700 samples, B = 1 and 32.

In the manner of tools/griffinlim_timing.py: every variant is timed with device events around one call, the variants ALTERNATE inside
each repetition and the median over --reps repetitions is reported.  The rotation:
  taco_griffinlim_fast, 30 rounds, momentum 0.99 (the call whose waveform is finished);
  taco_wave_finish on that waveform, one call;
  taco_wave_finish, 20 calls back to back between one pair of events, per call (one call is tens of microseconds: the single-call
  figure carries the launch latency of an idle queue, this one the steady rate);
  taco_griffinlim, 50 rounds.
The input of the finishing call is the Griffin-Lim waveform of random magnitudes scaled to a peak of 0.5, with a quiet head and tail
(1e-4 of the level) so that the trim has something to cut.  Recorded next to the medians: the share of the vocoder call, the bytes the
call has to move and the rate that gives, and -- when profiles/griffinlim_fast_timing.json is there -- the medians the parent commit
recorded for the two Griffin-Lim calls, which this change must not move.

    python tools/wave_finish_timing.py [--reps 20] [--warmup 3] [--out DIR]

Prints one JSON line; with --out also writes it to DIR/wave_finish_timing.json.  No pass mark: the exit status is 0 unless a call fails."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')

import torch  # noqa: E402

from tacotron_amd import lib  # noqa: E402
from tools.griffinlim_timing import alternate  # noqa: E402

F, N_PLAIN, N_FAST, MOMENTUM, DEEMPH, TRIM_DB, BURST = 360, 50, 30, 0.99, 0.97, 40.0, 20


def parent_medians():
    """{B: {name: ms}} of the committed measurement of the parent commit, or None"""
    path = os.path.join(ROOT, 'profiles', 'griffinlim_fast_timing.json')
    if not os.path.exists(path):
        return None
    rec = json.load(open(path))
    return {r['B']: {'taco_griffinlim_fast_30': r['fast_m099_30'], 'taco_griffinlim_50': 0.5 * (r['taco_griffinlim_a'] + r['taco_griffinlim_b'])}
            for r in rec['rows']}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'wave_finish_timing needs a GPU'
    dev = torch.device('cuda', torch.cuda.current_device())
    L = 300 * (F - 1)
    parent = parent_medians()
    res = {'tool': 'wave_finish_timing', 'F': F, 'L': L, 'n_fast': N_FAST, 'n_plain': N_PLAIN, 'momentum': MOMENTUM, 'deemphasis': DEEMPH,
           'trim_top_db': TRIM_DB, 'reps': a.reps, 'warmup': a.warmup, 'version': lib.version(),
           'unit': 'ms per call (median; variants alternate inside each repetition)', 'rows': [], 'checks': []}
    for B in (1, 32):
        g = torch.Generator(device='cpu').manual_seed(B)
        mag = (torch.rand((B, 1025, F), generator=g) + 1e-3).to(dev)
        ph = (2.0 * math.pi * torch.rand((B, 1025, F), generator=g)).to(dev)
        wave = torch.empty(B, L, device=dev)
        work = torch.empty(lib.griffinlim_workspace_floats(B, F), device=dev)
        work_fast = torch.empty(lib.griffinlim_fast_workspace_floats(B, F), device=dev)
        # the finishing call's own input: a fixed copy of the vocoder's waveform, scaled, quiet at both ends
        x = lib.griffinlim_fast(mag, None, phase0=ph, n_iter=2, momentum=MOMENTUM, work=work_fast).clone()
        x *= 0.5 / x.abs().amax(dim=1, keepdim=True).clamp_min(1e-20)
        x[:, :15000] *= 1e-4
        x[:, 90000:] *= 1e-4
        out = torch.empty(B, L, device=dev)
        pcm = torch.empty(B, L, dtype=torch.int16, device=dev)
        bounds = torch.empty(B, 2, dtype=torch.int32, device=dev)
        peak = torch.empty(B, device=dev)
        work_fin = torch.empty(lib.wave_finish_workspace_floats(B, L), device=dev)

        def finish():
            lib.wave_finish(x, None, deemphasis=DEEMPH, trim_top_db=TRIM_DB, out=out, pcm=pcm, bounds=bounds, peak=peak, work=work_fin)

        def finish_burst():
            for _ in range(BURST):
                finish()

        fns = {'taco_griffinlim_fast_30': lambda: lib.griffinlim_fast(mag, None, phase0=ph, n_iter=N_FAST, momentum=MOMENTUM, out=wave, work=work_fast),
               'taco_wave_finish': finish,
               'taco_wave_finish_x%d' % BURST: finish_burst,
               'taco_griffinlim_50': lambda: lib.griffinlim(mag, ph, N_PLAIN, out=wave, work=work)}
        row = {'B': B}
        row.update(alternate(fns, a.reps, a.warmup))
        row['taco_wave_finish_steady'] = row.pop('taco_wave_finish_x%d' % BURST) / BURST
        torch.cuda.synchronize()
        b = bounds.cpu()
        row['kept_samples_mean'] = float((b[:, 1] - b[:, 0]).float().mean())
        row['peak_max'] = float(peak.max())
        res['rows'].append(row)
        # bytes the call has to move: x read twice (aggregates, scan), y written, y read for the frame energies and once more by
        # the emit pass (the kept part), fp32 and int16 written over the full length
        kept = row['kept_samples_mean']
        nbytes = B * (4.0 * L * 3 + 4.0 * L + 4.0 * kept + 6.0 * L)
        chk = {'B': B, 'share_of_griffinlim_fast_30': row['taco_wave_finish'] / row['taco_griffinlim_fast_30'],
               'steady_share_of_griffinlim_fast_30': row['taco_wave_finish_steady'] / row['taco_griffinlim_fast_30'],
               'bytes_moved': nbytes, 'steady_gb_per_s': nbytes / (row['taco_wave_finish_steady'] * 1e-3) / 1e9}
        if parent and B in parent:
            chk['parent_recorded'] = parent[B]
            chk['over_parent_recorded'] = {k: row[k] / v for k, v in parent[B].items()}
        res['checks'].append(chk)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, 'wave_finish_timing.json'), 'w') as f:
            f.write(line + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
