"""train.py -- host driver with the reference's CLI and loop contract (train.py:16-126): -t/--train-set, -d/--debug,
-r/--restore; LR annealing every 1000 steps, loss-explosion guard, checkpoint + listening sample every SAVE_EVERY steps
(train.py:85-103; the TensorBoard wrapping is out of scope, the sample is written as .wav / .npy under log/<save_path>/).
Without a preprocessed corpus under data/<set>/ it trains on synthetic Nancy-shaped batches.
--align-log (opt-in): the alignment monitor.  At every log step the batch's attention is scored on the device
(Tacotron.alignment_scores) and a second line gives the batch means of focus, covered / L, back, skip and pad_mass and the number of
rows alignment.flags marks; the listening sample gets attention_<step>.png and attention_<step>_scores.npy next to its .npy.
--monitor (opt-in): the training monitor.  The log steps also compute, on the device, statistics and log-bucket histograms of every
parameter, gradient and Adam slot and of the activations the reference histograms (Tacotron.step(monitor=True), lib.tensor_stats);
one more line names the largest gradient RMS and lr |grad| / |param|, the share of zeros behind the encoder pre-net and the tensors
that hold non-finite values, and monitor/monitor_<step>.npz keeps everything.
--holdout N (default 0): the last N utterances are never drawn, so that tacotron_amd.evaluate can score checkpoints on them.
--ema DECAY (opt-in, 0 < DECAY < 1, no default): weight averaging.  Behind every update one more pass on the device moves an
exponential moving average of the parameters towards the new weights (lib.param_ema; tf.train.ExponentialMovingAverage's rule and
num_updates warm-up, skipped when the Adam update is); the log steps print the decay in use and the distance of the weights from
their average, and checkpoints carry the average for `test --ema` and `evaluate --ema`.  Without it nothing changes."""
from __future__ import annotations

import argparse
import math
import os
import pickle as pkl

import numpy as np
import torch

from . import config as config_module
from .config import SAVE_EVERY, Config
from .data import DeviceCorpus, DeviceFeeder, synthetic_batch, synthetic_corpus
from .dist import GradReducer, init_from_env
from .model import Tacotron


def save_sample(model, out_dir, step, n_iter=50, align=False):
    """train.py:92-103: `ideal` = the target spectrogram of utterance 0 through Griffin-Lim, `sample` = the model's output for
    it, plus its alignment; both de-normalised with the corpus statistics (identity for synthetic data).
    align (--align-log): additionally attention_<step>.png, the reference's attention picture of utterance 0 (alignment.attention_png),
    and attention_<step>_scores.npy, its 8 alignment scores as float64 (lib.ALIGN_COUNTS, then lib.ALIGN_MEANS)."""
    from . import lib
    from .griffinlim import invert_spectrogram
    from .test import write_wav
    c = model.config
    os.makedirs(out_dir, exist_ok=True)
    dev = model.output.device
    mean = torch.as_tensor(model.stft_mean if model.stft_mean is not None else np.zeros(c.fft_size * c.r), dtype=torch.float32, device=dev)
    std = torch.as_tensor(model.stft_std if model.stft_std is not None else np.ones(c.fft_size * c.r), dtype=torch.float32, device=dev)
    pair = torch.stack([model.inputs['stft'][0], model.output[0]]).contiguous()       # (2, Td, 1025 r): ideal, sample
    wav = invert_spectrogram(pair, mean, std, c.r, n_iter=n_iter, seed=step).cpu().numpy()
    spec = lib.denorm_unframe(pair, mean, std, c.r).cpu().numpy()
    write_wav(os.path.join(out_dir, 'ideal_%d.wav' % step), wav[0])
    write_wav(os.path.join(out_dir, 'sample_%d.wav' % step), wav[1])
    np.save(os.path.join(out_dir, 'sample_%d_spec.npy' % step), spec[1])
    attention = model.alignments[0].cpu().numpy()
    np.save(os.path.join(out_dir, 'attention_%d.npy' % step), attention)
    if align:
        from .alignment import attention_png, scores_row
        counts, means = model.alignment_scores()
        attention_png(os.path.join(out_dir, 'attention_%d.png' % step), attention)
        np.save(os.path.join(out_dir, 'attention_%d_scores.npy' % step), scores_row(counts[0].cpu().numpy(), means[0].cpu().numpy()))


def align_line(counts, means, text_length, Tt):
    """The --align-log line of one batch from its host arrays: counts (B, 6), means (B, 2), text_length (B)."""
    from .alignment import flags
    counts, means = np.asarray(counts), np.asarray(means, dtype=np.float64)
    L = np.clip(np.asarray(text_length, dtype=np.int64), 1, Tt)
    flagged = sum(1 for c, m, l in zip(counts, means, L) if flags(c, m, l))
    return ('align focus %.3f covered %.3f back %.2f skip %.2f pad_mass %.4f flagged %d/%d' %
            (means[:, 0].mean(), (counts[:, 5] / L).mean(), counts[:, 3].mean(), counts[:, 4].mean(), means[:, 1].mean(), flagged, len(L)))


def monitor_nonfinite(names, counts):
    """The names of the monitor's tensors that hold a NaN or an infinity, in the monitor's order: counts (N, 6) as lib.STATS_COUNTS."""
    counts = np.asarray(counts)
    return [str(n) for n, c in zip(names, counts) if c[2] + c[3] + c[4] > 0]


def monitor_line(names, counts, moments, lr):
    """The --monitor line of one log step from host arrays: names (N), counts (N, 6) and moments (N, 5) of Tacotron.monitor_result
    (lib.STATS_COUNTS / lib.STATS_MOMENTS; sums over the finite elements).  It gives the largest per-tensor gradient RMS with its
    name; the largest lr |grad| / |param| with its name -- a PROXY for the update ratio: the true Adam update (m / (sqrt(v) + eps),
    clipped) is not computed; the share of exact zeros in pre_net_out (dropout and dead ReLUs alike); and the number of tensors that
    hold non-finite values with the first three names."""
    names = [str(n) for n in names]
    counts, moments = np.asarray(counts), np.asarray(moments, dtype=np.float64)
    row = {n: i for i, n in enumerate(names)}
    rms, ratio = (0.0, '-'), (0.0, '-')
    for n, i in row.items():
        if not n.startswith('grad/'):
            continue
        g2, fin = moments[i, 1], counts[i, 1]
        if fin > 0 and math.sqrt(g2 / fin) > rms[0]:
            rms = (math.sqrt(g2 / fin), n[5:])
        p = row.get('param/' + n[5:])
        if p is not None and moments[p, 1] > 0.0:
            q = lr * math.sqrt(g2 / moments[p, 1])
            if q > ratio[0]:
                ratio = (q, n[5:])
    zeros = '-'
    if 'pre_net_out' in row and counts[row['pre_net_out'], 0] > 0:
        zeros = '%.1f%%' % (100.0 * counts[row['pre_net_out'], 5] / counts[row['pre_net_out'], 0])
    bad = monitor_nonfinite(names, counts)
    return ('monitor grad-rms max %.3e (%s) lr|g|/|w| max %.3e (%s) pre_net_out zeros %s non-finite %d%s' %
            (rms[0], rms[1], ratio[0], ratio[1], zeros, len(bad), (': ' + ', '.join(bad[:3]) + (', ...' if len(bad) > 3 else '')) if bad else ''))


def save_monitor(model, out_dir, step, host=None):
    """monitor_<step>.npz under out_dir: names, counts, moments, hist of model.monitor_result, the NB + 1 bucket edges and the three
    bucket parameters.  host: the (counts, moments, hist) arrays when they have been read already."""
    from . import lib
    os.makedirs(out_dir, exist_ok=True)
    counts, moments, hist = host if host is not None else (t.cpu().numpy() for t in model.monitor_result)
    e_lo, e_hi, sub_bits = lib.STATS_E_LO, lib.STATS_E_HI, lib.STATS_SUB_BITS
    path = os.path.join(out_dir, 'monitor_%d.npz' % step)
    np.savez(path, names=np.array(model.monitor_names), counts=counts, moments=moments, hist=hist,
             edges=lib.tensor_stats_edges(e_lo, e_hi, sub_bits), e_lo=e_lo, e_hi=e_hi, sub_bits=sub_bits)
    return path


def ema_line(decay, k, stats):
    """The --ema line of one log step: decay the configured one, k the number of the update the step made (0 the first), stats the
    three host values of Tacotron.ema_stats (lib.param_ema).  It gives the decay the warm-up used and lag = |weights - average| /
    |weights|, the distance before the update over the norm of the weights; a skipped update says so."""
    from . import lib
    d2, p2, applied = (float(x) for x in stats)
    if applied != 1.0:
        return 'ema decay %.6f update skipped (decoder error words set)' % lib.ema_decay(decay, k)
    return 'ema decay %.6f lag %.3e' % (lib.ema_decay(decay, k), math.sqrt(d2 / p2) if p2 > 0.0 else float('nan'))


def load_corpus(data_path, seed=0):
    """data_input.load_meta + load_from_npy (data_input.py:43-85,110-113) when the npy files exist.  The normalisation
    statistics come from 100 utterances like the reference's (data_input.py:55-65) but from a SEEDED draw, so every rank
    (and a restarted run) standardises the targets identically; they are returned for the checkpoint (train.py:31-33)."""
    meta_path = os.path.join(data_path, 'meta.pkl')
    if not os.path.exists(meta_path):
        return None
    with open(meta_path, 'rb') as f:
        meta = pkl.load(f)
    arr = {n: np.load(os.path.join(data_path, n + '.npy')) for n in ('texts', 'text_lens', 'stfts', 'mels')}
    stft, mel = arr['stfts'].astype(np.float32), arr['mels'].astype(np.float32)
    idx = np.random.default_rng(seed).integers(len(stft), size=100)
    stft_mean, stft_std = stft[idx].mean((0, 1)), stft[idx].std((0, 1))
    mel_mean, mel_std = mel[idx].mean((0, 1)), mel[idx].std((0, 1))
    data = {'text': arr['texts'].astype(np.int32), 'text_length': arr['text_lens'].astype(np.int32),
            'stft': (stft - stft_mean) / stft_std, 'mel': (mel - mel_mean) / mel_std}
    spk_path = os.path.join(data_path, 'speakers.npy')   # data_input.py:76-83: present for multi-speaker corpora (VCTK)
    if os.path.exists(spk_path):
        data['speaker'] = np.load(spk_path).astype(np.int32)
    return meta, data, stft_mean, stft_std


def open_corpus(data_path, seed=0):
    """load_corpus without the widening: (meta, data, norm), or None when there is no meta.pkl.  data['stft'] / data['mel'] are
    the npy files memory-mapped AS STORED (fp16 from tacotron_amd.preprocess; fp32 files are accepted); norm = {'stft': (mean,
    std), 'mel': (mean, std)} holds load_corpus's statistics -- the same seeded 100-utterance draw, widened to fp32 after the rows
    are taken, which gives the same bits -- for the feeders to standardise in the batch gather (`norm=`, lib.corpus_batch).
    The host never holds an fp32 copy of the corpus."""
    meta_path = os.path.join(data_path, 'meta.pkl')
    if not os.path.exists(meta_path):
        return None
    with open(meta_path, 'rb') as f:
        meta = pkl.load(f)
    stft, mel = (np.load(os.path.join(data_path, n + '.npy'), mmap_mode='r') for n in ('stfts', 'mels'))
    idx = np.random.default_rng(seed).integers(len(stft), size=100)
    norm = {}
    for name, arr in (('stft', stft), ('mel', mel)):
        if arr.dtype not in (np.float16, np.float32):
            raise ValueError('%s: %ss.npy holds %s, expected float16 or float32' % (data_path, name, arr.dtype))
        rows = arr[idx].astype(np.float32)
        norm[name] = (rows.mean((0, 1)), rows.std((0, 1)))
    data = {'text': np.load(os.path.join(data_path, 'texts.npy')).astype(np.int32),
            'text_length': np.load(os.path.join(data_path, 'text_lens.npy')).astype(np.int32), 'stft': stft, 'mel': mel}
    spk_path = os.path.join(data_path, 'speakers.npy')   # data_input.py:76-83: present for multi-speaker corpora (VCTK)
    if os.path.exists(spk_path):
        data['speaker'] = np.load(spk_path).astype(np.int32)
    return meta, data, norm


def latest_checkpoint(ckpt_prefix):
    """tf.train.latest_checkpoint (train.py:49-52) for files named '<prefix>-<step>': the highest STEP, not the
    lexicographically last name ('tacotron-5000' sorts after 'tacotron-10000')."""
    d, base = os.path.dirname(ckpt_prefix) or '.', os.path.basename(ckpt_prefix)
    if not os.path.isdir(d):
        return None
    best, best_step = None, -1
    for f in os.listdir(d):
        head, sep, tail = f.rpartition('-')
        if sep and head == base and tail.isdigit() and int(tail) > best_step:
            best, best_step = os.path.join(d, f), int(tail)
    return best


def holdout_draw(n, holdout, batch_size, seed):
    """The minibatch draw that leaves the last `holdout` of n utterances alone: step -> batch_size indices ~ U{0 .. n - holdout - 1}
    from np.random.default_rng(seed), the generator and the call the feeders use on their own -- with holdout = 0 the same values."""
    n, holdout = int(n), int(holdout)
    if not 0 <= holdout < n:
        raise ValueError('--holdout %d: must be >= 0 and below the corpus size %d' % (holdout, n))
    rng = np.random.default_rng(seed)
    return lambda step: rng.integers(n - holdout, size=int(batch_size))


def train(config, num_steps=1000000, log_every=50, save_every=SAVE_EVERY, corpus_fp32=False, align_log=False, holdout=0, monitor=False,
          ema=None):
    """ema: None, or the decay of weight averaging, 0 < ema < 1 (Config.ema_decay).  Every step then ends with one more pass on the
    device (lib.param_ema) that moves an average of the parameters towards the new weights, under TF's num_updates warm-up; the log
    steps also reduce its statistics and print one more line (ema_line), read at the synchronisation point that is there already.
    Checkpoints carry the average (`test --ema`, `evaluate --ema`); the listening sample stays on the live weights.  No decay is
    tuned here and nobody has listened to a voice decoded from an average.  None: every step, file, line and checkpoint is what it
    was.
    monitor: the training monitor.  The log steps (global step a multiple of log_every) run with Tacotron.step(monitor=True):
    statistics and histograms of every parameter, gradient and Adam slot and of the reference's histogram sites, computed on the
    device (lib.tensor_stats).  Rank 0 reads them at the log step's synchronisation point, writes
    log/<save_path>/monitor/monitor_<step>.npz (save_monitor) and prints one more line (monitor_line); before `loss exploded` it
    names every tensor that holds a non-finite value.  With several ranks the gradients are the reduced ones, the activations
    rank 0's own.  No launch, copy or synchronisation is added to any other step.
    holdout: the last N utterances of the corpus are never drawn (tacotron_amd.evaluate scores a checkpoint on them); 0: every
    utterance is drawn, as before.
    align_log: score the batch's attention on the device at every log step and print a second line (module docstring); no launch,
    copy or synchronisation is added to any other step.
    corpus_fp32: standardise the whole corpus on the host and feed fp32 (load_corpus; A/B runs) instead of keeping it as stored
    and standardising in the batch gather (open_corpus + norm=, the default).  The batches are bit-identical either way."""
    if ema is not None:
        if not 0.0 < float(ema) < 1.0:   # (NaN fails)
            raise ValueError('ema (--ema) must be a decay in (0, 1), got %r' % (ema,))
        config.ema_decay = float(ema)
    rank, world, local = init_from_env()
    torch.cuda.set_device(local)
    corpus = load_corpus(config.data_path) if corpus_fp32 else open_corpus(config.data_path)
    stft_mean = stft_std = norm = None
    if corpus is not None:
        if corpus_fp32:
            meta, data, stft_mean, stft_std = corpus
        else:
            meta, data, norm = corpus
            stft_mean, stft_std = norm['stft']
        config.r, config.vocab_size = meta['r'], len(meta['vocab'])
        if 'speaker' in data:                       # train.py:29
            config.num_speakers = int(data['speaker'].max()) + 1
        n = len(data['text'])
    else:
        if rank == 0:
            print('no corpus under %s -- synthetic Nancy-shaped batches' % config.data_path)
        data, n = None, 0
    if data is None:   # a pool of synthetic utterances stands in for the npy corpus; batches are index draws from it either way
        data = synthetic_corpus(max(256, 4 * config.batch_size), 200, config.max_decode_iter, config.r, config.vocab_size,
                                seed=1234, rank=rank, num_speakers=config.num_speakers)
    # The reference's queue runners (train.py:44-45): the corpus lives in HBM and a batch is a device-side gather (DeviceCorpus);
    # a corpus beyond TACO_CORPUS_HBM_GB (default 64) is fed by a prefetching worker through pinned buffers and a copy stream
    # (DeviceFeeder).  Either way set_inputs() gets device tensors and is a pointer swap -- a blocking pageable copy of the 51 MB
    # batch alone would be ~2 x the 8.4 ms train step.
    dev = torch.device('cuda', local)
    budget = float(os.environ.get('TACO_CORPUS_HBM_GB', '64')) * (1 << 30)
    # --holdout: the same seeded generator over the first n - N utterances; 0 leaves the feeders' own draw in place
    draw = holdout_draw(len(data['text']), holdout, config.batch_size, 1000 + rank) if holdout else None
    if DeviceCorpus.nbytes(data) <= budget:
        feeder = DeviceCorpus(data, config.batch_size, device=dev, seed=1000 + rank, norm=norm, draw=draw)
    else:
        feeder = DeviceFeeder(data, config.batch_size, device=dev, depth=2, seed=1000 + rank, norm=norm, draw=draw)

    def next_batch(step):
        return feeder.next()

    # same initial parameters on every rank (seed 0); the dropout / sampling streams are offset by the reducer's rank
    # TACO_FORCE_DIST=1 at world size 1 takes every distributed branch too (as bench.py does): reducer, collectives, barriers
    forced = torch.distributed.is_initialized() and world == 1
    distributed = world > 1 or forced
    model = Tacotron(config, next_batch(0), train=True, seed=0, reducer=GradReducer(force=forced) if distributed else None)
    model.stft_mean, model.stft_std = stft_mean, stft_std
    ckpt_prefix = os.path.join('weights', config.save_path)   # 'weights/nancy/tacotron' or 'weights/debug'
    if config.restore:
        # train.py:49-58: the latest checkpoint, unless the module constant RESTORE_FROM names a step -- then exactly
        # '<prefix>-<RESTORE_FROM>' (a missing file is an error there as well: saver.restore raises)
        restore_from = config_module.RESTORE_FROM
        path = latest_checkpoint(ckpt_prefix) if restore_from is None else '%s-%s' % (ckpt_prefix, restore_from)
        if path is not None:
            if restore_from is not None and not os.path.exists(path):
                raise FileNotFoundError('RESTORE_FROM=%s: %s does not exist' % (restore_from, path))
            model.load_state_dict(torch.load(path))
            if rank == 0:
                print('restored %s (global_step %d)' % (path, model.global_step))
    lr = config.init_lr
    averaging = hasattr(model, 'ema')
    import time
    mon_step, mon_lr, mon_host = None, lr, None           # the step model.monitor_result belongs to, and its host copy once read
    t_mark, s_mark, step = None, 0, -1                    # throughput of the host loop itself (reported when the loop ends)
    try:
        for step in range(num_steps):
            model.set_inputs(next_batch(step))                # device tensors from the feeder: a pointer swap
            mon = monitor and (model.global_step + 1) % log_every == 0
            ema_log = averaging and (model.global_step + 1) % log_every == 0
            if ema_log:
                model.step(lr, monitor=mon, ema_stats=True)   # (the averaging pass of this step also reduces its statistics)
            else:
                model.step(lr, monitor=mon)
            gs = model.global_step
            if mon:
                mon_step, mon_lr = gs, lr
            if step == 10:                                    # (past the first steps' one-off costs: lazy allocations, LDS attribute calls)
                torch.cuda.synchronize()
                t_mark, s_mark = time.perf_counter(), step
            if gs % log_every == 0 or gs % save_every == 0:
                scores = model.alignment_scores() if align_log else None   # one launch, enqueued in front of the sync below
                loss = float(model.loss)                      # the only host sync, every log_every steps
                try:
                    model.check()                             # decoder exchange time-outs surface here (sticky flag; the
                except Exception as e:                        # guarded Adam update skipped itself in the meantime)
                    if not getattr(e, 'recoverable', False):
                        raise
                    print('WARNING (rank %d): %s -- continuing' % (rank, e))   # check() moved to a more conservative decoder mode
                if rank == 0:
                    # tacotron.py:162-164: the summaries 'loss', 'seq2seq_loss', 'output_loss' (the scalars; --monitor adds the histogram sites below)
                    s2s_l, out_l = (float(x) for x in model.loss_terms)
                    print('step %d loss %.1f (seq2seq %.1f + output %.1f) gnorm %.2f decoder-mode %d' %
                          (gs, loss, s2s_l, out_l, float(model.global_gradient_norm), model.decoder_mode))
                    if scores is not None:                    # (B, 6) + (B, 2) + (B) values, already computed: no alignment tensor travels
                        print('step %d %s' % (gs, align_line(scores[0].cpu().numpy(), scores[1].cpu().numpy(),
                                                             model.inputs['text_length'].cpu().numpy(), model.shape.Tt)))
                    if ema_log:                               # three doubles, behind the sync above
                        print('step %d %s' % (gs, ema_line(model.ema_decay, model.ema_updates - 1, model.ema_stats.tolist())))
                    if mon:                                   # three copies behind the sync above: (N, 6) + (N, 5) + (N, NB) values
                        mon_host = tuple(t.cpu().numpy() for t in model.monitor_result)
                        save_monitor(model, os.path.join('log', config.save_path, 'monitor'), gs, mon_host)
                        print('step %d %s' % (gs, monitor_line(model.monitor_names, mon_host[0], mon_host[1], mon_lr)))
                # train.py:77-80; `not isfinite` added: the bf16x3 GEMMs turn an Inf operand into NaN (inf - inf in the plane split),
                # and `NaN > 1e8` is False -- a diverged run must still stop here
                if (not math.isfinite(loss) or loss > 1e8) and gs > 500:
                    if rank == 0 and mon_step is not None:    # (the results are on the device already; this log step's, or the last one's)
                        if mon_host is None or not mon:
                            mon_host = tuple(t.cpu().numpy() for t in model.monitor_result)
                        bad = monitor_nonfinite(model.monitor_names, mon_host[0])
                        print('non-finite at step %d: %s' % (mon_step, ', '.join(bad) if bad else 'no monitored tensor'))
                    print('loss exploded')
                    break
            if gs % 1000 == 0:
                lr *= config.annealing_rate                   # train.py:82-83
            if gs % save_every == 0 and gs != 0:
                if rank == 0:
                    print('saving weights')
                    os.makedirs(os.path.dirname(ckpt_prefix) or '.', exist_ok=True)
                    torch.save(model.state_dict(), '%s-%d' % (ckpt_prefix, gs))
                    print('saving sample')
                    save_sample(model, os.path.join('log', config.save_path), gs, align=align_log)
                if distributed:
                    # rank 0 spent a while on the host; the others must not run ahead into the next step's collectives (and the
                    # persistent decoder kernels of a rank that waits inside a collective keep spinning on their peers)
                    torch.distributed.barrier()
    except BaseException:
        #  a non-recoverable TacoError from check(), a feeder failure, Ctrl-C: the worker thread must not be inside a
        # device call when the interpreter tears the runtime down, and the process group must not outlive the loop
        try:
            torch.cuda.synchronize()
        except Exception:   # noqa: BLE001 -- the original exception is the one to report
            pass
        feeder.close()
        if torch.distributed.is_initialized():
            torch.distributed.destroy_process_group()
        raise
    torch.cuda.synchronize()
    feeder.close()
    if t_mark is not None and step > s_mark:
        dt = time.perf_counter() - t_mark
        fps = (step - s_mark) * config.batch_size * config.r * config.max_decode_iter * max(world, 1) / dt
        model.host_loop_frames_per_s = fps
        if rank == 0:
            print('host loop: %d steps in %.2f s = %.3f ms/step, %.0f mel-frames/s (%d rank%s), data fed by %s' %
                  (step - s_mark, dt, dt / (step - s_mark) * 1e3, fps, world, '' if world == 1 else 's', type(feeder).__name__))
    if torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()
    return model


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('-t', '--train-set', default='nancy')
    ap.add_argument('-d', '--debug', type=bool, default=False)
    ap.add_argument('-r', '--restore', type=bool, default=False)
    ap.add_argument('--steps', type=int, default=1000000)
    ap.add_argument('--corpus-fp32', action='store_true',
                    help='standardise the corpus on the host and feed fp32 (the earlier path) instead of keeping it as stored')
    ap.add_argument('--align-log', action='store_true',
                    help='alignment monitor: a second log line with the batch means of the per-utterance attention scores (computed on '
                         'the device) and the rows the untuned thresholds of alignment.flags mark; attention_<step>.png with every sample')
    ap.add_argument('--monitor', action='store_true',
                    help='training monitor: at every log step, statistics and log-bucket histograms of every parameter, gradient and '
                         'Adam slot and of the reference\'s histogram sites, computed on the device -> one more log line and '
                         'log/<save_path>/monitor/monitor_<step>.npz; names the non-finite tensors before `loss exploded`')
    ap.add_argument('--holdout', type=int, default=0, metavar='N',
                    help='never draw the last N utterances of the corpus: the set `python -m tacotron_amd.evaluate --holdout N` scores')
    ap.add_argument('--ema', type=float, default=None, metavar='DECAY',
                    help='weight averaging: keep an exponential moving average of the parameters on the device, 0 < DECAY < 1 (e.g. '
                         '0.999; no default and none tuned here), with TF\'s num_updates warm-up; one more pass per step, one more log '
                         'line, and checkpoints that `test --ema` / `evaluate --ema` can decode from (not in the reference; nobody has '
                         'listened to the result)')
    a = ap.parse_args(argv)
    if a.ema is not None and not 0.0 < a.ema < 1.0:
        ap.error('--ema DECAY must be in (0, 1), got %r' % (a.ema,))
    return a


if __name__ == '__main__':
    a = parse_args()
    c = Config()
    c.data_path = 'data/%s/' % a.train_set
    c.restore = a.restore
    c.save_path = 'debug' if a.debug else '%s/tacotron' % a.train_set
    print('Building Tacotron')
    train(c, a.steps, corpus_fp32=a.corpus_fp32, align_log=a.align_log, holdout=a.holdout, monitor=a.monitor, ema=a.ema)
