"""Wall time of one inference call, taco_infer against taco_infer_stop, at B = 1 and B = 32 (Tt = 140 as test.py pads, Td = 180,
r = 2, random weights).  The stop rules are synthetic: end_offset >= Tt makes every step count (target 0), so with hold = 1 the
rule fires on step min_steps - 1 for every row, at about 25 / 50 / 100 % of Td.  Times are device events around each call on the
default decoder (decoder3.hip), median over --reps calls after --warmup.

    python tools/infer_stop_timing.py [--reps 30] [--warmup 5] [--out DIR]

Prints one JSON line; with --out also writes it to DIR/infer_stop_timing.json."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tacotron_amd import lib  # noqa: E402
from tacotron_amd.config import Config  # noqa: E402
from tacotron_amd.data import synthetic_batch  # noqa: E402
from tacotron_amd.model import Tacotron  # noqa: E402


def time_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ts.append(s.elapsed_time(e))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'infer_stop_timing needs a GPU'
    Tt, Td = 140, 180
    res = {'tool': 'infer_stop_timing', 'Tt': Tt, 'Td': Td, 'r': 2, 'decoder_mode': lib.decoder_mode(), 'reps': a.reps,
           'unit': 'ms per call (median)', 'rows': []}
    for B in (1, 32):
        c = Config()
        c.r, c.vocab_size, c.max_decode_iter = 2, 60, Td
        m = Tacotron(c, synthetic_batch(B, Tt, Td, 2, 60, seed=7, min_len=20), train=False, seed=0)
        row = {'B': B, 'taco_infer': time_ms(m.run, a.reps, a.warmup)}
        m.check()
        for frac in (0.25, 0.5, 1.0):
            ms = int(round(frac * Td))
            rule = lib.TacoStopRule(end_offset=Tt, hold=1, min_steps=ms)
            t = time_ms(lambda: m.run(stop=rule), a.reps, a.warmup)
            m.check()
            ln = m.lengths.cpu().numpy()
            assert (ln == min(Td, 4 * ((ms + 3) // 4))).all(), ln
            row['stop_len_%d' % int(ln[0])] = t
        res['rows'].append(row)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, 'infer_stop_timing.json'), 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
