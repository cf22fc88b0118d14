"""evaluate.py -- held-out evaluation of a checkpoint (no counterpart in the reference, which never scores one): for the last N
utterances of the corpus, the ones `train --holdout N` never draws,
  (a) the teacher-forced loss: taco_forward through a train=True Tacotron on the checkpoint's parameters with masks=None, i.e. no
      dropout and no sampling -- the three numbers the train log prints, on utterances the optimiser has not seen;
  (b) a free-running score: the prompt's text is decoded with end detection (run(stop=TacoStopRule())), the predicted and the
      recorded mel frames are put in chronological order on the device, and their mel-cepstral distortion is taken over a dynamic-
      time-warping path (Tacotron.mel_distortion -> lib.frame_dtw; the warp because a free-running decoder does not keep the
      recording's timing).  The recorded frame count is read off the frames (lib.frames_active): the corpus pads every recording
      with frames of log(1e-8) and stores no length.
Only cost, steps, na, nb and the three losses of each batch travel to the host.

    python -m tacotron_amd.evaluate -t nancy [--checkpoint P] [--holdout N] [--speaker S] [--cepstra 13] [--out-dir log/eval] [--f0 | --f0-aligned] [--f0-smooth] [--durations] [--gv [--gv-lifter Q] [--sharpen BETA]] [--ema]

prints one line per batch and a final line with the mean teacher-forced loss and the mean and worst MCD, and writes
eval_<step>.npy, one row per utterance: index, na, nb, steps, cost, mcd (float64; COLUMNS).

WHAT THIS MCD IS: MCD_DB * cost / steps, where cost sums the Euclidean distance of DCT coefficients 1 .. cepstra (c0 left out) of
the model's OWN 80-band natural-log mel frames along the path, and steps counts the path's cells.  It is comparable between
checkpoints of this project on the same held-out set.  It is NOT comparable with figures published from other feature extractors
(mel-generalised cepstra of a vocoder analysis, other band counts, log bases, frame rates or path-length conventions).

--f0 (opt-in): the pitch of the free-running output and of the recording, the standard companions of MCD.  The predicted
magnitude frames (the decoder's output de-normalised, over each row's own frames) and the recorded ones (the corpus `stft` as
stored, through lib.corpus_batch + lib.denorm_unframe as `mel` is) are tracked on the device (lib.frames_f0) and summarised there
(lib.f0_stats); each utterance's row gains F0_COLUMNS: the mean of log2 F0 over its voiced frames, its standard deviation, the
voiced share of its frames, and the same three of the recording.  The batch line and the final line add the mean difference of
the pitch level in cents and of the voiced share.  There is NO alignment between the two tracks: lib.frame_dtw returns a cost and
no path, so these are statistics per utterance, not an F0 error along the warp.  The pick's ratio 0.9 and threshold 0.3 are untuned.
The sample rate of the lag tables and of the Hz columns is the corpus' own (meta.pkl 'sr', as preprocess records it; 16000 without one),
and the predicted share is taken over the frames tracked, min(na, F) with F = (max_decode_iter // 4) 4 r.

--f0-aligned (opt-in, implies the tracking of --f0): the F0 error ALONG the warp.  The warp is taken with its path
(Tacotron.mel_distortion(want_path=True) -> lib.frame_dtw_path; the same cost and steps), and the two period tracks are compared
cell by cell of that path on the device (lib.path_f0_scores); only its counts and means travel to the host.  Each row gains
ALIGNED_COLUMNS behind F0_COLUMNS: the cells voiced in both tracks, the F0 RMSE and the F0 bias (predicted above recorded: positive)
in cents over those cells, the voicing decision error (cells voiced in one track only / cells) and the gross pitch error (both-voiced
cells whose periods differ by more than a factor GROSS / both-voiced cells); a column is NaN where its denominator is 0.  One more
line per batch and one final line give their means over the utterances.  --f0 alone prints and saves exactly what it did.

--f0-smooth (opt-in, implies --f0, combines with --f0-aligned): both tracks are smoothed across frames on the device
(lib.f0_viterbi, taco_f0_viterbi: lib.F0_CANDIDATES candidates per frame, one of them or "unvoiced" per frame by the best path under
lib.f0_viterbi_tables' bias and costs at the corpus' sample rate -- Praat's numbers, UNTUNED) in front of lib.f0_stats and
lib.path_f0_scores, so F0_COLUMNS and ALIGNED_COLUMNS are those of the smoothed tracks.  Each row gains SMOOTH_COLUMNS behind every
other column: the share of the frames tracked whose choice the smoothing moved away from the frame's own best, predicted and recorded.
One more line per batch and one final line give their means.  Without it every mode prints and saves exactly what it did.

--durations [--path-jump J] (opt-in): duration, the third of the usual prosody measures next to MCD and F0.  The best monotone path
through the attention (Tacotron.alignment_path, taco_alignment_path; a step advances by at most J characters, default
lib.PATH_JUMP = 4, untuned) gives every character a duration in decoder steps, twice: the PREDICTED one from the free-running
alignments over free.lengths, and the RECORDED one from the teacher-forced alignments of forced.forward(None) over the recording's
own steps, min(Td, 4 ceil(nb / (4 r))), formed on the device from nb.  Each row gains DUR_COLUMNS behind whatever the other options
append: the mean absolute difference of the two durations per character in ms (a step is r frames of 300 samples), the bias
(predicted longer: positive) in ms, and the attention mass per step on both paths.  One more line per batch and one final line give
their means.  The other modes print and save exactly what they did.  On an untrained model the attention follows no text and the
numbers mean nothing; and a boundary is exact at multiples of 4 steps only (alignment.py).

--gv [--gv-lifter Q] [--sharpen BETA] (opt-in): global variance, the standard measure of over-smoothed spectral envelopes.  The
predicted and the recorded magnitude frames are built as for --f0 (and shared with it), and per utterance the sums over its frames of
every cepstral coefficient and of its square are taken on the device (lib.frames_cepstats, taco_frames_cepstats; the predicted frames
counted by the stop rule, the recorded ones by lib.frames_active); only those sums travel to the host, where
var[n] = sums[n, 1] / count - (sums[n, 0] / count)^2 and the GV ratio = exp(mean over n = 1 .. Q of log(var_pred[n] / var_rec[n])),
Q = 32 by default.  Well below 1: the prediction's envelopes are over-smoothed.  An utterance with fewer than 2 frames on either side
has NaN.  Each row gains GV_COLUMNS behind every other column, and one more line per batch and one final line give the mean ratio and
the share of utterances below GV_LOW = 0.8.  With --sharpen BETA the predicted magnitudes are also passed through the post-filter of
`test --sharpen BETA` at its default lifter (lib.frames_sharpen) and scored again: a second column (GV_SHARPEN_COLUMNS) and both
numbers on the lines, so one run shows what the filter does to the measure.  Sharpening here touches the GV columns only: MCD, F0 and
durations are computed on what they were computed on.  The ratio is over this model's LINEAR-frequency cepstra, quefrencies 1 .. Q: it
is comparable between checkpoints here, NOT with published mel-cepstral GV figures.  BETA has no tuned default, and on an untrained
model the numbers mean nothing.  Without --gv every mode prints and saves exactly what it did.

--ema: both passes run on the checkpoint's AVERAGED weights (`train --ema DECAY` keeps an exponential moving average of the parameters
and saves it with them) instead of the ones the last minibatch left; a checkpoint that holds none is refused before anything is
scored.  Every column means what it meant: two runs on one checkpoint, with and without the flag, show what averaging buys there.

The final batch is padded to the batch size by repeating its last utterance; the copies are left out of the per-utterance rows and
of the MCD statistics.  The teacher-forced loss is one number per batch (and the CBHG's batch normalisation sees the whole batch),
so the padded batch enters the mean loss weighted by its share of real rows.  Without a corpus on disk the synthetic pool of
train.py stands in, as there."""
from __future__ import annotations

import argparse
import os

import numpy as np
import torch

from . import lib
from .config import Config
from .data import DeviceCorpus, synthetic_corpus
from .model import Tacotron
from .params import ParamBuffer
from .train import latest_checkpoint, open_corpus

COLUMNS = ('index', 'na', 'nb', 'steps', 'cost', 'mcd')
F0_COLUMNS = ('f0_mean', 'f0_sd', 'voiced', 'rec_f0_mean', 'rec_f0_sd', 'rec_voiced')   # appended with --f0; the first two in log2 Hz
ALIGNED_COLUMNS = ('path_voiced', 'f0_rmse_cents', 'f0_bias_cents', 'vuv_error', 'gross_error')   # appended with --f0-aligned
DUR_COLUMNS = ('dur_mae_ms', 'dur_bias_ms', 'path_mass', 'rec_path_mass')   # appended with --durations
SMOOTH_COLUMNS = ('f0_moved', 'rec_f0_moved')   # appended with --f0-smooth (last): shares of the frames tracked
GV_COLUMNS = ('gv_ratio',)   # appended with --gv (behind every other column); with --sharpen: GV_SHARPEN_COLUMNS
GV_SHARPEN_COLUMNS = ('gv_ratio', 'gv_ratio_sharpened')
GV_LOW = 0.8   # the final line gives the share of utterances whose GV ratio lies below this
GROSS = 1.2  # a both-voiced cell is a gross pitch error when one period is above GROSS times the other (the usual 20 %)
SR = 16000   # of a corpus whose meta.pkl records no 'sr', and of the synthetic pool
PAD_FLOOR = float(np.float16(np.log(1e-8)))   # the value preprocess stores in the padding frames (fp16 of log(1e-8))


def holdout_batches(n, holdout, batch_size, keep=None):
    """The last `holdout` of n utterances in batches of batch_size -> [(index (batch_size,) int64, valid)]: the first `valid` entries
    of a batch are its utterances, in corpus order; the rest of the final batch repeats its last utterance.  keep: a boolean mask over
    the n utterances (e.g. one speaker's); held-out utterances outside it are skipped."""
    n, holdout, batch_size = int(n), int(holdout), int(batch_size)
    if not 0 < holdout <= n:
        raise ValueError('holdout must be in 1..%d (the corpus size), got %d' % (n, holdout))
    if batch_size < 1:
        raise ValueError('batch_size must be >= 1, got %d' % batch_size)
    idx = np.arange(n - holdout, n, dtype=np.int64)
    if keep is not None:
        idx = idx[np.asarray(keep, dtype=bool)[idx]]
    out = []
    for lo in range(0, len(idx), batch_size):
        part = idx[lo:lo + batch_size]
        valid = len(part)
        if valid < batch_size:
            part = np.concatenate([part, np.full(batch_size - valid, part[-1], dtype=np.int64)])
        out.append((part, valid))
    return out


def unpad(batches, per_batch):
    """per_batch[i] (batch_size, ...) host arrays of batch i -> the rows of the real utterances, concatenated in corpus order"""
    return np.concatenate([np.asarray(x)[:valid] for (_, valid), x in zip(batches, per_batch)])


def mcd_rows(index, na, nb, steps, cost):
    """host arrays of the utterances -> (n, 6) float64 in the order COLUMNS; mcd is NaN for an utterance without a path (steps 0)"""
    steps = np.asarray(steps, dtype=np.float64)
    cost = np.asarray(cost, dtype=np.float64)
    mcd = np.full(len(steps), np.nan)
    np.divide(lib.MCD_DB * cost, steps, out=mcd, where=steps > 0)
    return np.stack([np.asarray(index, dtype=np.float64), np.asarray(na, dtype=np.float64), np.asarray(nb, dtype=np.float64), steps,
                     cost, mcd], axis=1)


def f0_columns(stats, frames, sr=SR):
    """lib.f0_stats rows (n, 3) (count, mean and deviation of log2(period in samples)) and the n frame counts they were taken over ->
    (n, 3) float64: mean log2 F0 in Hz, its deviation, voiced share.  An utterance without a voiced frame has NaN for the first two;
    one without frames NaN for the share too."""
    stats = np.asarray(stats, dtype=np.float64).reshape(-1, 3)
    frames = np.asarray(frames, dtype=np.float64)
    out = np.full((len(stats), 3), np.nan)
    some = stats[:, 0] > 0
    out[some, 0] = np.log2(float(sr)) - stats[some, 1]
    out[some, 1] = stats[some, 2]
    np.divide(stats[:, 0], frames, out=out[:, 2], where=frames > 0)
    return out


def f0_rows(rows, stats, na, rec_stats, nb, sr=SR):
    """rows (n, 6) in the order COLUMNS -> (n, 12): F0_COLUMNS appended.  na / nb: the frames the two tracks were taken over"""
    return np.concatenate([np.asarray(rows, dtype=np.float64), f0_columns(stats, na, sr), f0_columns(rec_stats, nb, sr)], axis=1)


def f0_summary(cols):
    """(n, 6) in the order F0_COLUMNS -> (mean difference of the pitch level in cents, mean difference of the voiced share), predicted
    minus recorded, over the utterances that have both; NaN without any"""
    cols = np.asarray(cols, dtype=np.float64).reshape(-1, 6)
    level, share = 1200.0 * (cols[:, 0] - cols[:, 3]), cols[:, 2] - cols[:, 5]
    return (float(np.nanmean(level)) if np.isfinite(level).any() else float('nan'),
            float(np.nanmean(share)) if np.isfinite(share).any() else float('nan'))


def aligned_columns(counts, means):
    """lib.path_f0_scores' counts (n, 5) and means (n, 2), a the predicted track and b the recorded one -> (n, 5) float64 in the order
    ALIGNED_COLUMNS; NaN where the denominator (the both-voiced cells; for vuv_error the cells) is 0"""
    counts = np.asarray(counts, dtype=np.float64).reshape(-1, 5)
    means = np.asarray(means, dtype=np.float64).reshape(-1, 2)
    cells, both = counts[:, 0], counts[:, 1]
    out = np.full((len(counts), 5), np.nan)
    out[:, 0] = both
    some = both > 0
    out[some, 1] = 1200.0 * means[some, 1]
    out[some, 2] = 1200.0 * means[some, 0]    # (log2 period_recorded - log2 period_predicted: predicted higher in pitch -> positive)
    np.divide(counts[:, 2] + counts[:, 3], cells, out=out[:, 3], where=cells > 0)
    np.divide(counts[:, 4], both, out=out[:, 4], where=some)
    return out


def aligned_summary(cols):
    """(n, 5) in the order ALIGNED_COLUMNS -> (mean F0 RMSE in cents, mean V/UV error, mean gross error) over the utterances that have
    one; NaN without any"""
    cols = np.asarray(cols, dtype=np.float64).reshape(-1, 5)
    return tuple(float(np.nanmean(cols[:, k])) if np.isfinite(cols[:, k]).any() else float('nan') for k in (1, 3, 4))


def duration_columns(dur, rec_dur, text_length, counts, mass, rec_counts, rec_mass, step_ms):
    """lib.alignment_path's dur (n, Tt), counts (n, 3) and mass (n) of the free-running and of the teacher-forced alignments, the n
    text lengths and the milliseconds of a decoder step -> (n, 4) float64 in the order DUR_COLUMNS: mean |dur - rec_dur| and mean
    (dur - rec_dur) over the utterance's characters, in ms, and mass / n of both paths (NaN for a path of 0 steps)"""
    dur, rec_dur = np.asarray(dur, dtype=np.float64), np.asarray(rec_dur, dtype=np.float64)
    L = np.clip(np.asarray(text_length, dtype=np.int64).reshape(-1), 1, dur.shape[1])
    own = np.arange(dur.shape[1])[None, :] < L[:, None]
    diff = np.where(own, dur - rec_dur, 0.0)
    out = np.full((len(L), 4), np.nan)
    out[:, 0] = np.abs(diff).sum(1) / L * float(step_ms)
    out[:, 1] = diff.sum(1) / L * float(step_ms)
    for k, (c, m) in enumerate(((counts, mass), (rec_counts, rec_mass))):
        n = np.asarray(c, dtype=np.float64).reshape(-1, 3)[:, 0]
        np.divide(np.asarray(m, dtype=np.float64).reshape(-1), n, out=out[:, 2 + k], where=n > 0)
    return out


def duration_summary(cols):
    """(n, 4) in the order DUR_COLUMNS -> their means over the utterances that have one; NaN without any"""
    cols = np.asarray(cols, dtype=np.float64).reshape(-1, 4)
    return tuple(float(np.nanmean(cols[:, k])) if np.isfinite(cols[:, k]).any() else float('nan') for k in range(4))


DUR_LINE = 'duration error %.0f ms per character (bias %+.0f ms), path mass per step %.3f free-running / %.3f teacher-forced'


def smooth_columns(counts, rec_counts):
    """lib.f0_viterbi's counts (n, 4) of the predicted and of the recorded track -> (n, 2) float64 in the order SMOOTH_COLUMNS: moved /
    F_b, NaN for a row without frames"""
    out = np.full((len(counts), 2), np.nan)
    for k, c in enumerate((np.asarray(counts, dtype=np.float64), np.asarray(rec_counts, dtype=np.float64))):
        has = c[:, 0] > 0
        out[has, k] = c[has, 2] / c[has, 0]
    return out


def smooth_summary(cols):
    """(n, 2) in the order SMOOTH_COLUMNS -> their means over the utterances that have one; NaN without any"""
    cols = np.asarray(cols, dtype=np.float64)
    return tuple(float(np.nanmean(cols[:, k])) if np.isfinite(cols[:, k]).any() else float('nan') for k in range(2))


SMOOTH_LINE = 'smoothing moved %.3f of the predicted and %.3f of the recorded frames'


def gv_columns(sums_pred, n_pred, sums_rec, n_rec, sums_sharp=None):
    """lib.frames_cepstats' sums (n, Q + 1, 2) and counts (n) of the predicted and of the recorded frames, and optionally the sums of
    the sharpened predicted frames (same counts) -> (n, 1) float64 in the order GV_COLUMNS, or (n, 2) in the order GV_SHARPEN_COLUMNS:
    lib.gv_ratio; NaN for an utterance with fewer than 2 frames on either side"""
    cols = [lib.gv_ratio(sums_pred, n_pred, sums_rec, n_rec)]
    if sums_sharp is not None:
        cols.append(lib.gv_ratio(sums_sharp, n_pred, sums_rec, n_rec))
    return np.stack([np.asarray(c, dtype=np.float64).reshape(-1) for c in cols], axis=1)


def gv_summary(cols):
    """(n, 1 | 2) in the order GV_COLUMNS / GV_SHARPEN_COLUMNS -> per column (mean ratio, share of the utterances below GV_LOW) over the
    utterances that have one, flattened: 2 or 4 numbers; NaN without any"""
    cols = np.asarray(cols, dtype=np.float64)
    cols = cols.reshape(len(cols), -1)
    out = []
    for k in range(cols.shape[1]):
        have = cols[np.isfinite(cols[:, k]), k]
        out += [float(have.mean()), float((have < GV_LOW).mean())] if len(have) else [float('nan'), float('nan')]
    return tuple(out)


def gv_line(summary, sharpen=None):
    """gv_summary's numbers -> 'GV ratio 0.61 (0.750 of the utterances below 0.8)', with --sharpen 'GV ratio 0.61, with --sharpen
    0.40: 0.97 (... below 0.8: 0.750, 0.000)'"""
    if len(summary) == 2:
        return 'GV ratio %.2f (%.3f of the utterances below %g)' % (summary[0], summary[1], GV_LOW)
    return 'GV ratio %.2f, with --sharpen %.2f: %.2f (share of the utterances below %g: %.3f, %.3f)' % (
        summary[0], float(sharpen), summary[2], GV_LOW, summary[1], summary[3])


def evaluate(config, holdout=64, checkpoint=None, speaker=None, cepstra=13, out_dir='log/eval', stop=None, device=0, trace=None,
             f0=False, f0_aligned=False, durations=False, path_jump=lib.PATH_JUMP, f0_smooth=False, gv=False, gv_lifter=lib.SHARPEN_LIFTER,
             sharpen=None, ema=False):
    """-> (rows (n, 6) float64 in the order COLUMNS, mean teacher-forced loss).  Module docstring.  f0: rows (n, 12), F0_COLUMNS behind
    COLUMNS.  f0_aligned (implies f0): rows (n, 17), ALIGNED_COLUMNS behind those.  durations: DUR_COLUMNS behind all of them (path_jump: the max_jump of the two paths).  stop: the lib.TacoStopRule of the
    free-running decode (default: TacoStopRule()).  trace: a list that receives, per batch, host copies of what the warp was given
    ({'predicted', 'recorded', 'na', 'nb'}: an extra copy per batch, for tests and inspection; with f0_aligned also the two period
    tracks 'period' and 'rec_period').  f0_smooth (implies f0): both tracks go through lib.f0_viterbi in front of the statistics and the
    path scores, SMOOTH_COLUMNS behind every other column; trace then also receives the per-frame tracks 'period_raw' and
    'rec_period_raw' and the smoothed ones 'period' and 'rec_period'.  gv / gv_lifter / sharpen (needs gv): the global-variance ratio
    over the quefrencies 1 .. gv_lifter, GV_COLUMNS behind every other column -- with a sharpen beta other than None and 0,
    GV_SHARPEN_COLUMNS; trace then also receives the magnitudes the sums were taken over, 'pred_mags' and 'rec_mags' (B, C, F), with
    sharpen also 'sharp_mags', and 'lengths', the decoder steps of the predicted rows.  ema (--ema; needs a checkpoint): both passes
    run on the checkpoint's AVERAGED weights (train --ema; Tacotron.load_state_dict(use_ema=True)) instead of the live ones;
    lib.TacoError before anything is scored when the checkpoint holds none.  Every column means what it meant."""
    f0 = bool(f0 or f0_aligned or f0_smooth)
    if sharpen is not None and not gv:
        raise ValueError('evaluate: sharpen (--sharpen) scores the post-filter by the global variance: it needs gv (--gv)')
    if gv:
        gv_lifter = lib.int_arg('evaluate', 'gv_lifter (--gv-lifter)', gv_lifter, lib.SHARPEN_FIRST, lib.PITCH_MAX_LIFTER)
        sharpen = None if sharpen is None else lib.float_arg('evaluate', 'sharpen (--sharpen)', sharpen, lib.SHARPEN_MIN_BETA,
                                                             lib.SHARPEN_MAX_BETA)
        sharpen = None if sharpen == 0.0 else sharpen
    torch.cuda.set_device(device)
    dev = torch.device('cuda', device)
    corpus = open_corpus(config.data_path)
    norm = None
    sr = SR
    if corpus is not None:
        meta, data, norm = corpus
        sr = int(meta.get('sr', SR))
        config.r, config.vocab_size = meta['r'], len(meta['vocab'])
        if 'speaker' in data:
            config.num_speakers = int(data['speaker'].max()) + 1
    else:
        print('no corpus under %s -- synthetic Nancy-shaped utterances' % config.data_path)
        data = synthetic_corpus(max(256, 4 * config.batch_size), 200, config.max_decode_iter, config.r, config.vocab_size, seed=1234,
                                num_speakers=config.num_speakers)
    n = len(data['text'])
    keep = None
    if speaker is not None:
        if 'speaker' not in data:
            raise ValueError('--speaker %d: the corpus under %s has no speakers.npy' % (speaker, config.data_path))
        keep = np.asarray(data['speaker']) == int(speaker)
    B = config.batch_size
    batches = holdout_batches(n, holdout, B, keep)
    if not batches:
        raise ValueError('none of the last %d utterances belongs to speaker %d' % (holdout, speaker))
    first = n - int(holdout)
    held = {k: v[first:] for k, v in data.items()}   # (a memmap stays one: only the held-out rows are read and uploaded)
    feeder = DeviceCorpus(held, B, device=dev, norm=norm, draw=lambda step: batches[step][0] - first)
    ckpt = torch.load(checkpoint) if checkpoint else None
    if ema and (ckpt is None or 'ema' not in ckpt):   # (before anything is built)
        raise lib.TacoError('ema (--ema): %s' % ('there is no checkpoint to take averaged weights from' if ckpt is None else
                                                 'the checkpoint %s holds no averaged weights (written without `train --ema`, or imported): '
                                                 'its keys are %s' % (checkpoint, ', '.join(sorted(map(str, ckpt))))))
    batch = feeder.next()
    shape = lib.make_shape(B, batch['text'].shape[1], batch['mel'].shape[1], config.r, config.vocab_size, config.num_speakers)
    params = ParamBuffer(shape, dev).init_(0)
    forced = Tacotron(config, batch, train=True, device=dev, params=params)   # (a): shares `params` with the decoder below
    text = {k: batch[k] for k in ('text', 'text_length', 'speaker') if k in batch}
    free = Tacotron(config, text, train=False, device=dev, params=params)    # (b): max_decode_iter free-running steps at the most
    if ckpt is not None:
        if ema:
            forced.load_state_dict(ckpt, use_ema=True)
            print('scoring the averaged weights (decay %s, %s updates)' % (ckpt.get('ema_decay', '?'), ckpt.get('ema_updates', '?')))
        else:
            forced.load_state_dict(ckpt)
        free.global_step = forced.global_step
    else:
        print('no checkpoint -- scoring the seed-0 initialisation')
    if norm is not None:
        free.mel_mean, free.mel_std = norm['mel']
    stop = stop if stop is not None else lib.TacoStopRule()
    r, Td = config.r, batch['mel'].shape[1]
    recorded = torch.empty(B, (Td // 4) * 4 * r, 80, device=dev)
    raw = torch.empty(B, Td, 80 * r, device=dev)
    nb = torch.empty(B, dtype=torch.int32, device=dev)
    zeros, ones = torch.zeros(80 * r, device=dev), torch.ones(80 * r, device=dev)
    per = {k: [] for k in ('na', 'nb', 'steps', 'cost') + (('f0', 'rec_f0', 'f0_frames') if f0 else ())
           + (('path_counts', 'path_means') if f0_aligned else ()) + (('smooth',) if f0_smooth else ()) + (('gv',) if gv else ())}
    if f0 or gv:   # the magnitudes of both sides, built once for the two of them
        Cs = batch['stft'].shape[2] // r
        raw_stft = torch.empty(B, Td, Cs * r, device=dev)
        mags = torch.empty(B, Cs, (Td // 4) * 4 * r, device=dev)
        szeros, sones = torch.zeros(Cs * r, device=dev), torch.ones(Cs * r, device=dev)
        smean, sstd = norm['stft'] if norm is not None and 'stft' in norm else (forced.stft_mean, forced.stft_std)
        smean = szeros if smean is None else torch.as_tensor(smean, dtype=torch.float32).to(dev)
        sstd = sones if sstd is None else torch.as_tensor(sstd, dtype=torch.float32).to(dev)
    if f0:
        w, g, lag_min, lag_max = lib.f0_tables(sr, C=Cs)
        f0_opt = dict(weight=torch.from_numpy(w).to(dev), gain=torch.from_numpy(g).to(dev), lag_min=lag_min, lag_max=lag_max)
        if f0_smooth:
            bias, lg = lib.f0_viterbi_lag_tables(lag_min, lag_max)
            _, _, jump, switch = lib.f0_viterbi_tables(sr, hop=300)
            smooth_opt = dict(lag_min=lag_min, lag_max=lag_max, bias=torch.from_numpy(bias).to(dev), lg=torch.from_numpy(lg).to(dev),
                              jump_cost=jump, switch_cost=switch)
    if durations:
        path_jump = lib.int_arg('evaluate', 'path_jump (--path-jump)', path_jump, 1, lib.PATH_MAX_JUMP)
        per.update(dur=[])
        step_ms = 1000.0 * r * 300 / sr
    losses = []
    for i, (index, valid) in enumerate(batches):
        if i:
            batch = feeder.next()
            forced.set_inputs(batch)
            free.set_inputs({k: batch[k] for k in text})
        forced.forward(None)
        free.run(stop=stop)
        # the recording as stored (a pure widening gather: no standardisation to undo), in chronological order
        lib.corpus_batch(feeder.data['mel'], None, None, index=torch.as_tensor(index - first).to(dev), out=raw)
        lib.denorm_unframe(raw, zeros, ones, r, spec=recorded)
        lib.frames_active(recorded, PAD_FLOOR, nb)
        if f0_aligned:
            cost, steps, na, path_a, path_b = free.mel_distortion(recorded, nb, cepstra, want_path=True)
        else:
            cost, steps, na = free.mel_distortion(recorded, nb, cepstra)
        if f0 or gv:   # the decoder's own frames over lengths * r (max_decode_iter steps wide), and the recording's over nb
            pmags = lib.denorm_unframe(free.output, smean, sstd, r, want_spec=False, want_mag_t=True)
            Fp = pmags.shape[2]   # (the tracker counts over clamp(lengths r, 0, Fp); na is lengths r unclamped)
            lib.corpus_batch(feeder.data['stft'], None, None, index=torch.as_tensor(index - first).to(dev), out=raw_stft)
            lib.denorm_unframe(raw_stft, szeros, sones, r, want_spec=False, want_mag_t=True, mag_t=mags)
        if gv:   # sharpening stays inside this block: every other score is taken on pmags as it is
            gv_pred, gv_rec = lib.frames_cepstats(pmags, gv_lifter, free.lengths, r), lib.frames_cepstats(mags, gv_lifter, nb, 1)
            gv_sharp = None
            if sharpen is not None:
                sharp_mags = lib.frames_sharpen(pmags, sharpen, lib.SHARPEN_LIFTER, free.lengths, r)
                gv_sharp = lib.frames_cepstats(sharp_mags, gv_lifter, free.lengths, r)
        if f0:
            if f0_smooth:
                pred_raw, _, acf = lib.frames_f0(pmags, free.lengths, r, want_acf=True, **f0_opt)
                pred_period, _, pred_moved, _ = lib.f0_viterbi(acf, free.lengths, r, **smooth_opt)
            else:
                pred_period = lib.frames_f0(pmags, free.lengths, r, **f0_opt)[0]
            pred_stats = lib.f0_stats(pred_period, None, free.lengths, r)
            if f0_smooth:
                rec_raw, _, acf = lib.frames_f0(mags, nb, 1, want_acf=True, **f0_opt)
                rec_period, _, rec_moved, _ = lib.f0_viterbi(acf, nb, 1, **smooth_opt)
            else:
                rec_period = lib.frames_f0(mags, nb, 1, **f0_opt)[0]
            rec_stats = lib.f0_stats(rec_period, None, nb, 1)
        if f0_aligned:   # the two tracks cell by cell of the warp's path; the path indexes the predicted mel frames
            Fm = path_a.shape[1] - recorded.shape[1] + 1
            if Fp != Fm:
                raise ValueError('evaluate --f0-aligned: the predicted pitch track is %d frames wide and the predicted mel frames %d: '
                                 'the path of one does not index the other' % (Fp, Fm))
            path_counts, path_means = lib.path_f0_scores(pred_period, rec_period, path_a, path_b, steps, GROSS)
        if durations:   # the recording's own steps, on the device: its nb frames in blocks of 4 steps of r frames
            rec_steps = torch.clamp((nb + (4 * r - 1)) // (4 * r) * 4, max=Td).to(torch.int32)
            free_path = free.alignment_path(path_jump)
            rec_path = forced.alignment_path(path_jump, steps=rec_steps)
        loss = forced._loss.cpu().numpy().astype(np.float64)       # the host synchronisation of the batch
        forced.check()
        free.check()
        got = {'na': na.cpu().numpy(), 'nb': nb.cpu().numpy(), 'steps': steps.cpu().numpy(), 'cost': cost.cpu().numpy()}
        if f0:
            got['f0'], got['rec_f0'] = pred_stats.cpu().numpy(), rec_stats.cpu().numpy()
            got['f0_frames'] = np.minimum(got['na'], Fp)
            if f0_aligned:
                got['path_counts'], got['path_means'] = path_counts.cpu().numpy(), path_means.cpu().numpy()
            if f0_smooth:
                got['smooth'] = smooth_columns(pred_moved.cpu().numpy(), rec_moved.cpu().numpy())
            cents, share = f0_summary(np.concatenate([f0_columns(got['f0'][:valid], got['f0_frames'][:valid], sr),
                                                      f0_columns(got['rec_f0'][:valid], got['nb'][:valid], sr)], axis=1))
        if gv:
            got['gv'] = gv_columns(gv_pred[0].cpu().numpy(), gv_pred[1].cpu().numpy(), gv_rec[0].cpu().numpy(), gv_rec[1].cpu().numpy(),
                                   None if gv_sharp is None else gv_sharp[0].cpu().numpy())
        if durations:
            got['dur'] = duration_columns(free_path[1].cpu().numpy(), rec_path[1].cpu().numpy(), batch['text_length'].cpu().numpy(),
                                          free_path[2].cpu().numpy(), free_path[3].cpu().numpy(), rec_path[2].cpu().numpy(),
                                          rec_path[3].cpu().numpy(), step_ms)
        if trace is not None and durations:
            trace_dur = {'alignments': free.alignments.cpu().numpy(), 'lengths': free.lengths.cpu().numpy(),
                         'rec_alignments': forced.alignments.cpu().numpy(), 'rec_steps': rec_steps.cpu().numpy(),
                         'text_length': batch['text_length'].cpu().numpy()}
        if trace is not None:
            trace.append({'predicted': free.predicted_mel()[0].cpu().numpy(), 'recorded': recorded.cpu().numpy(), 'na': got['na'].copy(),
                          'nb': got['nb'].copy()})
            if f0_aligned or f0_smooth:
                trace[-1].update(period=pred_period.cpu().numpy(), rec_period=rec_period.cpu().numpy())
            if f0_smooth:
                trace[-1].update(period_raw=pred_raw.cpu().numpy(), rec_period_raw=rec_raw.cpu().numpy())
            if durations:
                trace[-1].update(trace_dur)
            if gv:
                trace[-1].update(pred_mags=pmags.cpu().numpy(), rec_mags=mags.cpu().numpy(), lengths=free.lengths.cpu().numpy())
                if sharpen is not None:
                    trace[-1].update(sharp_mags=sharp_mags.cpu().numpy())
        for k, v in got.items():
            per[k].append(v)
        losses.append(loss)
        mcd = mcd_rows(index[:valid], *(got[k][:valid] for k in ('na', 'nb', 'steps', 'cost')))[:, 5]
        print('batch %d (%d utterances) loss %.1f (seq2seq %.1f + output %.1f) mcd mean %.3f dB worst %.3f dB frames %d / %d'
              % (i, valid, loss[0], loss[1], loss[2], np.nanmean(mcd), np.nanmax(mcd), int(got['na'][:valid].sum()),
                 int(got['nb'][:valid].sum())))
        if f0:
            print('batch %d pitch level %+.0f cents, voiced share %+.3f against the recordings (per utterance, not aligned)' % (i, cents, share))
        if f0_aligned:
            print('batch %d F0 RMSE %.0f cents, V/UV error %.3f, gross error %.3f along the warping path (aligned)'
                  % ((i,) + aligned_summary(aligned_columns(got['path_counts'][:valid], got['path_means'][:valid]))))
        if durations:
            print(('batch %d ' % i) + DUR_LINE % duration_summary(got['dur'][:valid]))
        if f0_smooth:
            print(('batch %d ' % i) + SMOOTH_LINE % smooth_summary(got['smooth'][:valid]))
        if gv:
            print(('batch %d ' % i) + gv_line(gv_summary(got['gv'][:valid]), sharpen))
    feeder.close()
    rows = mcd_rows(unpad(batches, [b[0] for b in batches]), *(unpad(batches, per[k]) for k in ('na', 'nb', 'steps', 'cost')))
    if f0:
        rows = f0_rows(rows, unpad(batches, per['f0']), unpad(batches, per['f0_frames']), unpad(batches, per['rec_f0']), rows[:, 2], sr)
        print('held out: pitch level %+.0f cents, voiced share %+.3f against the recordings (untuned tracker, per utterance, not aligned)'
              % f0_summary(rows[:, 6:]))
    if f0_aligned:
        rows = np.concatenate([rows, aligned_columns(unpad(batches, per['path_counts']), unpad(batches, per['path_means']))], axis=1)
        print('held out: F0 RMSE %.0f cents, V/UV error %.3f, gross error %.3f along the warping path (untuned tracker, aligned)'
              % aligned_summary(rows[:, 12:]))
    if durations:
        rows = np.concatenate([rows, unpad(batches, per['dur'])], axis=1)
        print('held out: ' + DUR_LINE % duration_summary(rows[:, -4:]) + ' (untuned max_jump %d; meaningless on an untrained model)' % path_jump)
    if f0_smooth:
        rows = np.concatenate([rows, unpad(batches, per['smooth'])], axis=1)
        print('held out: ' + SMOOTH_LINE % smooth_summary(rows[:, -2:]) + ' (untuned costs, %d candidates per frame)' % lib.F0_CANDIDATES)
    if gv:
        rows = np.concatenate([rows, unpad(batches, per['gv'])], axis=1)
        print('held out: ' + gv_line(gv_summary(rows[:, -per['gv'][0].shape[1]:]), sharpen)
              + ' (linear-frequency cepstra 1 .. %d; untuned; meaningless on an untrained model)' % gv_lifter)
    weight = np.array([valid for _, valid in batches], dtype=np.float64)
    mean_loss = float((np.stack(losses)[:, 0] * weight).sum() / weight.sum())
    print('held out: %d utterances, teacher-forced loss %.1f, MCD-DTW mean %.3f dB worst %.3f dB (utterance %d) over %d cepstra of '
          'the model\'s own mel frames' % (len(rows), mean_loss, np.nanmean(rows[:, 5]), np.nanmax(rows[:, 5]),
                                         int(rows[int(np.nanargmax(rows[:, 5])), 0]), cepstra))
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, 'eval_%d.npy' % forced.global_step), rows)
    return rows, mean_loss


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('-t', '--train-set', default='nancy')
    ap.add_argument('--checkpoint', default=None, help='default: the latest weights/<set>/tacotron-<step>')
    ap.add_argument('--holdout', type=int, default=64, help='the last N utterances of the corpus (train --holdout N never draws them)')
    ap.add_argument('--speaker', type=int, default=None, help='multi-speaker corpus: only the held-out utterances of this speaker')
    ap.add_argument('--cepstra', type=int, default=13, help='DCT coefficients 1 .. N of the 80 mel bands the distance is taken over')
    ap.add_argument('--out-dir', default='log/eval')
    ap.add_argument('--f0', action='store_true',
                    help='also track the pitch of the predicted and of the recorded magnitude frames on the device and append '
                         'F0_COLUMNS to every row (untuned tracker; statistics per utterance, no alignment)')
    ap.add_argument('--f0-aligned', action='store_true',
                    help='--f0, and the F0 error along the warping path: ALIGNED_COLUMNS (F0 RMSE and bias in cents, voicing decision '
                         'error, gross pitch error) behind F0_COLUMNS')
    ap.add_argument('--f0-smooth', action='store_true',
                    help='--f0, with both tracks smoothed across frames on the device (a Viterbi path over the candidates of every '
                         'frame, untuned costs) in front of the statistics and of --f0-aligned; SMOOTH_COLUMNS behind every other column')
    ap.add_argument('--durations', action='store_true',
                    help='per-character durations from the best monotone attention path, free-running against teacher-forced: '
                         'DUR_COLUMNS (mean absolute difference and bias in ms, path mass per step of both) behind the other columns')
    ap.add_argument('--path-jump', type=int, default=lib.PATH_JUMP, metavar='J',
                    help='--durations: characters a decoder step may advance on the path, 1 <= J <= 15 (default %d, untuned)' % lib.PATH_JUMP)
    ap.add_argument('--gv', action='store_true',
                    help='the global-variance ratio of the predicted against the recorded magnitude frames, per utterance: GV_COLUMNS '
                         'behind every other column; well below 1 means over-smoothed envelopes.  Taken over this model\'s '
                         'linear-frequency cepstra, quefrencies 1 .. Q: comparable between checkpoints here, not with published '
                         'mel-cepstral GV figures; meaningless on an untrained model')
    ap.add_argument('--gv-lifter', type=int, default=None, metavar='Q', help='--gv: the highest quefrency measured, 2 <= Q <= 64 (default %d)'
                    % lib.SHARPEN_LIFTER)
    ap.add_argument('--sharpen', type=float, default=None, metavar='BETA',
                    help='--gv: also pass the predicted magnitudes through the post-filter of `test --sharpen BETA`, -1 <= BETA <= 1, and '
                         'score them again (a second column; the GV columns only -- MCD, F0 and durations do not change).  BETA has no '
                         'tuned default')
    ap.add_argument('--ema', action='store_true',
                    help='score the averaged weights of a checkpoint written by `train --ema DECAY` instead of the live ones; an error '
                         'when the checkpoint holds none.  Run it with and without the flag to see what averaging buys')
    a = ap.parse_args(argv)
    if (a.gv_lifter is not None or a.sharpen is not None) and not a.gv:
        ap.error('--gv-lifter and --sharpen need --gv')
    a.gv_lifter = lib.SHARPEN_LIFTER if a.gv_lifter is None else a.gv_lifter
    return a


def main(argv=None, config=None):
    """config: a Config to start from instead of the defaults (its data_path is kept)"""
    a = parse_args(argv)
    c = config if config is not None else Config()
    if config is None:
        c.data_path = 'data/%s/' % a.train_set
    checkpoint = a.checkpoint or latest_checkpoint(os.path.join('weights', '%s/tacotron' % a.train_set))
    return evaluate(c, a.holdout, checkpoint, a.speaker, a.cepstra, a.out_dir, f0=a.f0, f0_aligned=a.f0_aligned, durations=a.durations,
                    path_jump=a.path_jump, f0_smooth=a.f0_smooth, gv=a.gv, gv_lifter=a.gv_lifter, sharpen=a.sharpen, ema=a.ema)


if __name__ == '__main__':
    main()
