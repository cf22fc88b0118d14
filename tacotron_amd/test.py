"""test.py -- inference driver with the reference's contract (test.py:13-89): prompts on stdin -> batches of <= 32 padded
to 140 chars -> always max_decode_iter steps -> normalised log-magnitude spectrogram (B, Td, 1025 r) + alignments ->
`audio.invert_spectrogram(out * stft_std + stft_mean)` per prompt (test.py:64).  The TensorBoard summary the reference
wraps each sample in (test.py:65-69) is out of scope; the sample itself is written as <out_dir>/prompt_NNN.wav (16 kHz, the
reference's sr) next to the de-normalised spectrogram and the alignment as .npy.
--stop (opt-in, not in the reference): end detection on the attention (lib.TacoStopRule, include/taco_hip.h); each prompt's
files are cut to its len_b decoder steps and prompt_NNN_len.npy holds len_b.  The rule's defaults are not tuned on a trained model.
--vocode-lengths (opt-in, with --stop): Griffin-Lim runs per prompt over its own len_b r frames (lib.griffinlim_rows) with phases
drawn on the device, so prompt_NNN.wav is the Griffin-Lim of that prompt alone.
--gl-momentum A (opt-in, not in the reference): fast Griffin-Lim rounds with momentum A in [0, 1) (lib.griffinlim_fast), phases drawn
on the device; prompt_NNN_conv.npy holds the prompt's n_iter + 1 spectral-convergence values and the batch's worst final value is
printed.  --gl-iters N: the number of rounds (default 50, the reference's).  Both combine with --stop / --vocode-lengths.
--gl-init {random,estimate} (opt-in, not in the reference; default random: every file is what it was): with `estimate` Griffin-Lim
starts from phases read off the magnitudes it is handed (lib.phase_estimate, taco_phase_estimate: every spectral peak a sinusoid
advanced by hop x its frequency, its lobe locked to it) instead of random ones.  --gl-iters 0 --gl-init estimate is the draft voice:
no Griffin-Lim round at all, one synthesis pass from the estimate.  Measured on fp64 restatements only; nobody has listened to it.  It
combines with everything the vocoder combines with; with --gl-momentum the convergence line is printed as it is.
--deemphasis [A] / --trim-db DB (opt-in, not in the reference): the waveform is finished on the device (griffinlim.finish_waveform,
taco_wave_finish): de-emphasis with A in [0, 1) (0.97 when A is left out: the inverse of the training features' pre-emphasis) and / or
the front end's energy trim at DB > 0 decibels below the loudest frame.  prompt_NNN.wav is then written from the device's int16
samples and holds e - s of them; prompt_NNN_trim.npy holds [s, e].  They combine with every option above.
--long (opt-in, with --stop; not in the reference): a line of more than 140 characters is cut where a speaker would pause
(data.split_prompt), its pieces run as rows of ordinary batches, each ending where its attention ends, every piece is finished on the
device (de-emphasis and trim stay off unless asked for) and the pieces of a prompt are joined there (griffinlim.join_waveform,
taco_wave_join): --pause-ms SENTENCE,CLAUSE,WORD of silence behind a piece by the kind of its cut, a linear ramp of --fade-ms at every
interior edge, PCM16 by the prompt's peak.  One prompt_NNN.wav per prompt; prompt_NNN_pieces.npy holds (offset, length, gap, kind) per
piece and the per-piece arrays are prompt_NNN_kMM_{spec,align,len,trim}.npy.  A prompt of one piece writes the files it writes without
--long.  Without --long a line of more than 140 characters is refused as before (ValueError from load_prompts).
--align-scores (opt-in; the reference draws the attention picture for TensorBoard instead, test.py:60-69): the per-utterance attention
scores are computed on the device (Tacotron.alignment_scores, taco_alignment_scores; over each prompt's own steps with --stop) and
prompt_NNN_ascore.npy holds the prompt's 8 values as float64 (lib.ALIGN_COUNTS, then lib.ALIGN_MEANS); prompt_NNN_align.png is the
attention picture over the kept steps (alignment.attention_png); a prompt that alignment.flags marks gets one `WARNING prompt N: ...`
line.  With --long a prompt of several pieces writes one pair per piece (prompt_NNN_kMM_*).  It combines with every option above.
--rate R (opt-in, not in the reference): the speaking rate, 1.0 the model's own, 0.8 slower, 1.25 faster, 0.25 <= R <= 4.  The magnitude
frames are resampled on the device between the de-normalisation and Griffin-Lim (lib.frames_stretch, taco_frames_stretch), which then
finds phases for the new length: the duration changes, the pitch does not.  prompt_NNN.wav holds the stretched audio, 300 (Fo_b - 1)
samples before any trim, and prompt_NNN_rate.npy holds (step_q, Fo_b) as int32; the spectrogram, alignment, length and score files
stay the model's own output.  With --stop the stretch and the vocoder run over each prompt's own len_b r frames, phases drawn on the
device.  Nobody has listened to the result.  It combines with every option above; with --long the pieces of a prompt inherit its rate.
--pitch SEMITONES [--lifter Q] (opt-in, not in the reference): the pitch, 0 the model's own, +3 higher, -3 lower, -12 <= SEMITONES <= 12.
Right behind the de-normalisation every magnitude frame is split on the device into a smooth log-envelope (the Q lowest quefrencies of
its cepstrum; default 32, untuned) and the rest; the rest alone -- the harmonics -- is moved along the bin axis and put back under the
unmoved envelope (lib.frames_pitch, taco_frames_pitch), so the formants and the duration stay.  prompt_NNN_pitch.npy holds (step_q,
lifter) as int32; every other file keeps its size, and the spectrogram, alignment, length, score and rate files stay the model's own.
--pitch 0 writes the audio of a run without --pitch.  Nobody has listened to the result.  It combines with every option above (it runs
in front of the stretch of --rate); with --long the pieces of a prompt inherit its pitch.
--f0 [--f0-range LO,HI] (opt-in, not in the reference): the pitch of every magnitude frame is measured on the device (lib.frames_f0,
taco_frames_f0: the autocorrelation of a frame is the cosine transform of its power spectrum, so no waveform is needed) between LO and
HI Hz (default 60,400) and prompt_NNN_f0.npy holds (period in samples, strength) as float32, one row per frame the vocoder was given;
0, 0 is an unvoiced frame, F0 = 16000 / period.  With --pitch one line per prompt gives the semitones asked for and the semitones
measured -- 12 x the mean over the frames voiced in both of log2(period unshifted / period shifted) (lib.f0_stats) -- and the count of
those frames; with --rate alone the line gives the change of the mean log-F0 in cents, which should be near 0 (unpaired: the frame
counts differ).  The pick's ratio 0.9 and threshold 0.3 are UNTUNED, and on an untrained model the frames have no pitch: the numbers
then mean nothing.  It is the objective stand-in for listening to --pitch and --rate, which nobody has done.  It combines with every
option above; with --long the files are per piece.
--f0-smooth [--f0-candidates K] (opt-in, implies --f0): the track is smoothed across frames on the device (lib.f0_viterbi,
taco_f0_viterbi: the K highest maxima of every frame's autocorrelation are kept, default lib.F0_CANDIDATES = 4, and one of them or
"unvoiced" is chosen per frame by the best path under Praat's costs for octave jumps and voicing switches -- UNTUNED).
prompt_NNN_f0.npy and the per-prompt line then use the smoothed track, and the line gains `, smoothing moved M of N frames`: the
frames whose choice differs from the frame's own best.  Without it every file and line is what it was.
--timings [--path-jump J] (opt-in, not in the reference): when each word is spoken.  The best monotone path through every prompt's
attention is found on the device (Tacotron.alignment_path, taco_alignment_path; over each prompt's own steps with --stop; a step may
advance by at most J characters, default lib.PATH_JUMP = 4, untuned) and only its durations, counts and mass come back with the other
results.  prompt_NNN_dur.npy holds the steps of each of the prompt's text_length characters as int32 and prompt_NNN_words.tsv one
`start_s<TAB>end_s<TAB>word` line per word of the written file (alignment.word_times: --rate, the trim of --deemphasis / --trim-db and,
with --long, the piece's offset in the joined file are applied; with --long each piece of a prompt of several writes
prompt_NNN_kMM_dur.npy and the prompt one _words.tsv).  One line per prompt gives the path's mass per step, its end against L - 1 and
the skipped characters, as a WARNING when the path ends more than end_offset characters before the text does.  A boundary is exact at
multiples of 4 decoder steps and nominal inside such a block (alignment.py): good for subtitles, not a phonetic aligner.  It combines
with every option above; without it every file is what it was.
--prosody FILE (opt-in, with --stop; not in the reference): rate and pitch per WORD.  FILE holds lines
`prompt<TAB>word<TAB>rate<TAB>semitones`, both indices 0-based, a word as --timings defines it, `-` in the rate or semitones field for
"leave"; words not listed take --rate / --pitch, or stay neutral.  The best monotone path through the attention says which decoder step
speaks which character (taco_alignment_path); two gathers turn the per-character durations and pitch steps into per-frame curves along
it (lib.path_curve, taco_path_curve), and the magnitudes go through the pitch curve (lib.frames_pitch_curve) and then the stretch curve
(lib.frames_stretch_curve) in front of Griffin-Lim -- inference, path, gathers, de-normalisation, pitch, stretch, Griffin-Lim and
finishing all on the device.  prompt_NNN.wav holds 300 (Fo_b - 1) samples before any trim, Fo_b the stretch's own frames_out;
prompt_NNN_prosody.npy holds the per-character (dur_q, step_q) as int32 (in place of _rate.npy / _pitch.npy); with --timings the word
rows go through the stretch's time map; with --f0 the line gives the drift of the mean log-F0 with no "asked" figure.  A word's
characters share one value and the curve steps at its edges: no ramps across word boundaries.  Refused with --long: the pieces
re-index the words of a prompt, which is out of scope here.  Nobody has listened to the result.  Without it every file is what it
was.
--loudness LUFS [--peak-db DB] (opt-in, not in the reference): the level.  The finished rows are measured on the device by ITU-R
BS.1770 -- K-weighting, 400 ms blocks, an absolute and a relative gate (griffinlim.level_waveform, taco_wave_loudness) -- and written
at LUFS, -70 <= LUFS <= 0 (-23: EBU R 128; -16 to -19: voice assistants and podcasts), with the sample peak at or below DB decibels re
full scale (default -1, <= 0); where the ceiling binds, the gain is what the ceiling allows.  It implies finishing, as --long does
(de-emphasis and trim stay off unless asked for).  prompt_NNN.wav holds the device's int16 samples, prompt_NNN_loud.npy holds
(I, M, g, peak_out, nb, past_abs, past_both, limited) as float64 and one line per prompt gives the loudness before and after.  A prompt
shorter than 400 ms is measured as one block (the standard leaves it unmeasured).  With --long the JOINED prompt is levelled, so its
pieces keep their relative levels.  It combines with every option above; without it every file is what it was.
--loudness LUFS --limit [--limit-ms MS] [--true-peak P] [--limit-passes N] (opt-in, not in the reference): the true-peak limiter.
Where the ceiling would hold the whole prompt under its target, the prompt gets the gain the target asks for and a look-ahead limiter
on the device (griffinlim.level_waveform(limit=True), taco_wave_limit) pulls down only the neighbourhood of a peak; DB then is the
ceiling on the TRUE peak (dBTP), read between the samples through a P-phase interpolator (default 4; 1: the sample peak).  MS is the
look-ahead (default 1.5 ms), N the passes (default 2: the second re-aims the gain at the target).  These defaults are untuned and
nobody has listened to a limited file.  prompt_NNN.wav holds the limited int16 samples, prompt_NNN_limit.npy holds (tp_in, G, g_min,
peak_out, n_b, n_limited, I_reached, tp_out) as float64 in place of _loud.npy, and one line per prompt gives the loudness before
and after, the true peak and how much was limited.  With --long the JOINED prompt is limited.  Without --limit no new code is reached."""
from __future__ import annotations

import argparse
import os
import pickle as pkl
import sys
import wave

import numpy as np
import torch

from .config import Config
from .alignment import attention_png, encoded_chars, flags, path_line, scores_row, word_times, word_values, words_tsv
from .data import KIND_NAMES, load_prompts, split_prompt
from .griffinlim import finish_waveform, invert_spectrogram, join_gaps, join_samples, join_waveform, level_waveform, limit_settings
from .model import Tacotron
from .params import ParamBuffer
from . import lib

SR = 16000   # test.py:11
PAUSE_MS = (300.0, 150.0, 0.0)   # --long: silence behind a SENTENCE / CLAUSE / WORD cut; choices, not tuned by anyone's ear
FADE_MS = 5.0                    # --long: the ramp at every interior edge; likewise
JOIN_GROUP = 256                 # --long: pieces per lib.wave_join call (a group ends at the first prompt boundary at or past it)
LIMIT_MS = 1.5                   # --limit: the look-ahead in milliseconds (untuned, as are lib.LIMIT_P / LIMIT_T / LIMIT_BETA)
LIMIT_PASSES = 2                 # --limit: limiter passes; every pass after the first re-aims the gain at the target
PEAK_DB = -1.0                   # --loudness: the ceiling on the sample peak, decibels re full scale


def write_wav(path, samples, sr=SR):
    """librosa.output.write_wav's role (audio.py:73-74): mono PCM16, peak-normalised only if the signal would clip."""
    x = np.asarray(samples, dtype=np.float64)
    peak = np.max(np.abs(x)) if x.size else 0.0
    if peak > 1.0:
        x = x / peak
    with wave.open(path, 'wb') as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(sr)
        f.writeframes((x * 32767.0).astype('<i2').tobytes())


def write_wav_pcm(path, int16_samples, sr=SR):
    """mono PCM16 from samples that already are int16 (the device's, lib.wave_finish): no arithmetic on the host."""
    x = np.ascontiguousarray(int16_samples)
    if x.dtype != np.int16 or x.ndim != 1:
        raise ValueError('write_wav_pcm: expected a 1-d int16 array, got %s %s' % (x.dtype, x.shape))
    with wave.open(path, 'wb') as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(sr)
        f.writeframes(x.astype('<i2', copy=False).tobytes())


def long_options(long):
    """`long` of test(): None / False (off), True (the defaults) or a dict with 'pause_ms' (SENTENCE, CLAUSE, WORD) and / or 'fade_ms'
    -> None or (pause_ms, fade_ms); ValueError"""
    if long is None or long is False:
        return None
    opt = {} if long is True else dict(long)
    unknown = set(opt) - {'pause_ms', 'fade_ms'}
    if unknown:
        raise ValueError('long (--long): unknown settings %s' % sorted(unknown))
    pause_ms = tuple(float(x) for x in opt.get('pause_ms', PAUSE_MS))
    fade_ms = float(opt.get('fade_ms', FADE_MS))
    join_gaps([], pause_ms)   # (their ranges)
    join_samples(fade_ms)
    return pause_ms, fade_ms


def _steps(name, values, to_step, n):
    """lib.steps_of for an option of test(), a single number repeated for every prompt; ValueError names the option"""
    try:
        steps = lib.steps_of(values, to_step, n)
    except ValueError as e:
        raise ValueError('%s (--%s): %s' % (name, name, e)) from None
    return [steps] * (1 if n is None else n) if isinstance(steps, int) else steps


def rate_steps(rate, n):
    """`rate` of test(): None, a number or a sequence of n numbers in [0.25, 4] -> None or the n step_q values (lib.stretch_step);
    ValueError"""
    return _steps('rate', rate, lib.stretch_step, n)


def pitch_steps(pitch, n):
    """`pitch` of test(): None, a number or a sequence of n numbers of semitones in [-12, 12] -> None or the n step_q values
    (lib.pitch_step); ValueError"""
    return _steps('pitch', pitch, lib.pitch_step, n)


def parse_prosody(text):
    """The text of a --prosody file -> [(prompt, word, rate | None, semitones | None)]: lines `prompt<TAB>word<TAB>rate<TAB>semitones`,
    both indices 0-based integers, `-` in the rate or semitones field for "leave"; empty lines and lines starting with # are skipped.
    ValueError names the line."""
    rows = []
    for k, line in enumerate(text.splitlines(), 1):
        if not line.strip() or line.lstrip().startswith('#'):
            continue
        parts = line.rstrip('\r\n').split('\t')
        try:
            if len(parts) != 4:
                raise ValueError('expected 4 fields, got %d' % len(parts))
            prompt, word = int(parts[0]), int(parts[1])
            rate = None if parts[2].strip() == '-' else float(parts[2])
            semitones = None if parts[3].strip() == '-' else float(parts[3])
        except ValueError as e:
            raise ValueError('prosody (--prosody): line %d %r: expected prompt<TAB>word<TAB>rate<TAB>semitones: %s' % (k, line, e)) from None
        rows.append((prompt, word, rate, semitones))
    return rows


def prosody_table(rows, prompts, ivocab, base_dur=None, base_step=None):
    """The rows of parse_prosody against the prompts -> per prompt an (L, 2) int32 array of (dur_q, step_q) per encoded character
    (alignment.word_values): the characters of a listed word take lib.stretch_dur(rate) / lib.pitch_step(semitones), everything else
    the prompt's base_dur / base_step (sequences with one value per prompt; None: 65536, neutral).  ValueError for a prompt or word
    index that does not exist, a rate outside [0.25, 4], semitones outside [-12, 12] and a word listed twice."""
    per = [({}, {}) for _ in prompts]
    for prompt, word, rate, semitones in rows:
        who = 'prosody (--prosody): prompt %d word %d' % (prompt, word)
        if not 0 <= prompt < len(prompts):
            raise ValueError('%s: there are the prompts 0 .. %d' % (who, len(prompts) - 1))
        durs, steps = per[prompt]
        if word in durs or word in steps:
            raise ValueError('%s is listed twice' % who)
        try:
            if rate is not None:
                durs[word] = lib.stretch_dur(rate)
            if semitones is not None:
                steps[word] = lib.pitch_step(semitones)
            if rate is None and semitones is None:
                durs[word] = None   # (listed, nothing asked: only the index is checked)
        except ValueError as e:
            raise ValueError('%s: %s' % (who, e)) from None
    out = []
    for p, line in enumerate(prompts):
        bd = lib.STRETCH_ONE if base_dur is None else int(base_dur[p])
        bs = lib.PITCH_ONE if base_step is None else int(base_step[p])
        try:
            d, _ = word_values(line, ivocab, {w: (bd if v is None else v) for w, v in per[p][0].items()}, bd)
            q, _ = word_values(line, ivocab, per[p][1], bs)
        except ValueError as e:
            raise ValueError('prosody (--prosody): prompt %d: %s' % (p, e)) from None
        out.append(np.array([d, q], dtype=np.int32).reshape(2, -1).T.copy())
    return out


def f0_range(f0):
    """`f0` of test(): None / False (off), True (60 .. 400 Hz) or (lo, hi) in Hz -> None or (lo, hi) after lib.f0_tables has accepted
    them at 16 kHz; ValueError"""
    if f0 is None or f0 is False:
        return None
    try:
        lo, hi = (60.0, 400.0) if f0 is True else (float(x) for x in f0)
        lib.f0_tables(SR, lo, hi)
    except (TypeError, ValueError) as e:
        raise ValueError('f0 (--f0 / --f0-range): %s' % e) from None
    return lo, hi


def f0_lines(who, f0row, asked_step=None, rate_step=None, prosody=False):
    """the line(s) --f0 prints for `who` ('prompt 3', or 'prompt 3 piece 1' with --long) from its row of the statistics: f0row =
    (model_stats, vocoder_stats, pitch_stats | None), and with --f0-smooth behind them the row's lib.f0_viterbi counts: the line
    gains `, smoothing moved M of N frames` (without --pitch and --rate that is the whole line).  prosody (--prosody): the drift line of
    --rate without a figure asked for -- the curves ask for something else in every word"""
    model, voc, paired = f0row[:3]
    out = []
    if len(f0row) > 3 and f0row[3] is not None:
        tail = 'smoothing moved %d of %d frames' % (int(f0row[3][2]), int(f0row[3][0]))
        lines = f0_lines(who, f0row[:3], asked_step, rate_step, prosody)
        return ['%s, %s' % (lines[0], tail)] + lines[1:] if lines else ['%s f0: %s' % (who, tail)]
    if prosody:
        out.append('%s prosody: mean log-F0 moved %+.1f cents (%d -> %d voiced frames)'
                   % (who, 1200.0 * (float(model[1]) - float(voc[1])), int(model[0]), int(voc[0])))
    elif asked_step is not None and paired is not None:
        out.append('%s pitch: asked %+.2f, measured %+.2f semitones over %d voiced frames'
                   % (who, 12.0 * np.log2(65536.0 / asked_step), 12.0 * float(paired[1]), int(paired[0])))
    elif rate_step is not None:
        out.append('%s rate %.3f: mean log-F0 moved %+.1f cents (%d -> %d voiced frames)'
                   % (who, rate_step / 65536.0, 1200.0 * (float(model[1]) - float(voc[1])), int(model[0]), int(voc[0])))
    return out


def loud_row(loud, blocks):
    """a row of lib.wave_loudness's loud (4) and blocks (4) -> the 8 float64 values of prompt_NNN_loud.npy"""
    return np.concatenate([np.asarray(loud, dtype=np.float64), np.asarray(blocks, dtype=np.float64)])


def loud_line(who, row, peak_db=PEAK_DB):
    """the line --loudness prints for `who` from its loud_row"""
    I, g, limited = float(row[0]), float(row[2]), int(row[7])
    if not np.isfinite(I):
        return '%s: no block above the gates, level unchanged' % who
    after = I + 20.0 * np.log10(g)
    if limited:
        return '%s: %.1f LUFS -> %.1f, limited by the %g dB ceiling' % (who, I, after, peak_db)
    return '%s: %.1f LUFS -> %.1f (gain %+.1f dB)' % (who, I, after, 20.0 * np.log10(g))


def limit_row(peaks, counts, I_reached, tp_out, I_in):
    """a row of lib.wave_limit's peaks (4) and counts (2), the loudness reached, the true peak of the output and the loudness of the
    input -> 9 float64 values: the 8 of prompt_NNN_limit.npy (tp_in, G, g_min, peak_out, n_b, n_limited, I_reached, tp_out), then I_in"""
    return np.concatenate([np.asarray(peaks, dtype=np.float64), np.asarray(counts, dtype=np.float64),
                           np.asarray([I_reached, tp_out, I_in], dtype=np.float64)])


def limit_line(who, row, target):
    """the line --loudness --limit prints for `who` from its limit_row"""
    g_min, n_b, n_lim, I_out, tp_out, I_in = (float(row[k]) for k in (2, 4, 5, 6, 7, 8))
    if not np.isfinite(I_in):
        return '%s: no block above the gates, level unchanged' % who
    db = lambda v: 20.0 * np.log10(v) if v > 0.0 else -np.inf
    return ('%s: %.1f LUFS -> %.1f (asked %.1f), true peak %.1f dBTP, %.1f %% of samples limited, deepest %.1f dB'
            % (who, I_in, I_out, target, db(tp_out), 100.0 * n_lim / max(n_b, 1.0), db(g_min)))


def level_line(who, row, level):
    """loud_line or limit_line, by what `level` asked for"""
    return limit_line(who, row, level['target']) if level.get('limit') else loud_line(who, row, level['ceiling_db'])


def level_finished(fin, level, **rows):
    """level_waveform(fin, **rows, **level) on finished device rows -> (pcm (B, L) int16 on the device, the rows' loud_rows; with
    level['limit'] their limit_rows).  With the limiter the input is measured once more for the line, and the TRUE peak of the
    output by one measure-only call of lib.wave_limit; everything is read back in one go at the end"""
    if not level.get('limit'):
        _, pcm, loud, blocks = level_waveform(fin, want_out=False, want_pcm=True, **rows, **level)
        return pcm, np.stack([loud_row(a, b) for a, b in zip(loud.cpu().numpy(), blocks.cpu().numpy())])
    out, pcm, loud, _, peaks, counts = level_waveform(fin, want_pcm=True, **rows, **level)
    n_b = counts[:, 0].contiguous()
    I_in = lib.wave_loudness(fin, n_b, sr=SR, target=None)[2][:, 0]
    P = level['oversample']
    taps = lib.true_peak_taps(P) if P > 1 else np.zeros((0, lib.LIMIT_T), np.float32)
    tp_out = lib.wave_limit(out, n_b, taps=taps)[2][:, 0]
    return pcm, np.stack([limit_row(*r) for r in zip(peaks.cpu().numpy(), counts.cpu().numpy(), loud[:, 0].cpu().numpy(),
                                                     tp_out.cpu().numpy(), I_in.cpu().numpy())])


def check_options(n_iter=50, stop=None, vocode_lengths=False, gl_momentum=None, deemphasis=None, trim_db=None, long=None, rate=None,
                  vocode=True, pitch=None, lifter=32, f0=None, f0_smooth=None, prosody=None, gl_init=None, loudness=None, peak_db=None,
                  limit=False, limit_ms=None, true_peak=None, limit_passes=None, path_jump=None):
    """The option ranges of test() and of the command line (`stop`: a rule, or True / None for given / not given; `path_jump`: None
    without --timings; `f0_smooth`: None / False, True or the number of candidates; `prosody`: None / False or anything else for
    given; `gl_init`: None, 'random' or 'estimate'; `peak_db`: None for not given; `limit`: True / False, `limit_ms`, `true_peak`,
    `limit_passes`: None for not given); ValueError."""
    if loudness is not None:
        if not vocode:
            raise ValueError('loudness (--loudness) levels the waveform: it needs vocode')
        if not -70.0 <= float(loudness) <= 0.0:   # (NaN fails)
            raise ValueError('loudness (--loudness) must be in [-70, 0] LUFS, got %r' % (loudness,))
    if peak_db is not None:
        if loudness is None:
            raise ValueError('peak_db (--peak-db) is the ceiling of loudness (--loudness): it needs loudness')
        if not float(peak_db) <= 0.0 or np.isinf(float(peak_db)):
            raise ValueError('peak_db (--peak-db) must be a finite number of decibels <= 0, got %r' % (peak_db,))
    if not isinstance(limit, bool):
        raise ValueError('limit (--limit) must be True or False, got %r' % (limit,))
    if limit and loudness is None:
        raise ValueError('limit (--limit) holds the true peak of loudness (--loudness) at its ceiling: it needs loudness')
    for name, v in (('limit_ms (--limit-ms)', limit_ms), ('true_peak (--true-peak)', true_peak), ('limit_passes (--limit-passes)', limit_passes)):
        if v is not None and not limit:
            raise ValueError('%s is a setting of limit (--limit): it needs limit' % name)
    if limit:
        limit_options(limit_ms, true_peak, limit_passes)
    if gl_init not in (None, 'random', 'estimate'):
        raise ValueError("gl_init (--gl-init) must be 'random' or 'estimate', got %r" % (gl_init,))
    if gl_init == 'estimate' and not vocode:
        raise ValueError('gl_init (--gl-init) estimates the phases Griffin-Lim starts from: it needs vocode')
    if prosody is not None and prosody is not False:
        if not vocode:
            raise ValueError('prosody (--prosody) shapes the magnitudes in front of Griffin-Lim: it needs vocode')
        if not stop:
            raise ValueError('prosody (--prosody) needs a stop rule (--stop): the curves follow the path over each prompt\'s own steps')
        if long_options(long) is not None:
            raise ValueError('prosody (--prosody) cannot be combined with long (--long): the pieces re-index the words of a prompt')
    if f0_smooth is not None and f0_smooth is not False:
        if f0 is None or f0 is False:
            raise ValueError('f0_smooth (--f0-smooth) smooths the track of f0 (--f0): it needs f0')
        if f0_smooth is not True:
            lib.int_arg('check_options', 'f0_smooth (--f0-candidates)', f0_smooth, 1, lib.F0_MAX_CAND)
    if path_jump is not None:
        lib.int_arg('check_options', 'path_jump (--path-jump)', path_jump, 1, lib.PATH_MAX_JUMP)
    if f0 is not None and f0 is not False:
        if not vocode:
            raise ValueError('f0 (--f0) measures the magnitudes in front of Griffin-Lim: it needs vocode')
        f0_range(f0)
    if pitch is not None:
        if not vocode:
            raise ValueError('pitch (--pitch) shifts the magnitudes in front of Griffin-Lim: it needs vocode')
        pitch_steps(pitch, None)
        lib.int_arg('check_options', 'lifter (--lifter)', lifter, 1, lib.PITCH_MAX_LIFTER)
    if rate is not None:
        if not vocode:
            raise ValueError('rate (--rate) stretches the magnitudes in front of Griffin-Lim: it needs vocode')
        rate_steps(rate, None)
    if long_options(long) is not None and not stop:
        raise ValueError('long (--long) needs a stop rule (--stop): without one every piece carries max_decode_iter steps')
    if vocode_lengths and not stop:
        raise ValueError('vocode_lengths (--vocode-lengths) needs a stop rule (--stop): the lengths come from taco_infer_stop')
    if gl_momentum is not None and not 0.0 <= float(gl_momentum) < 1.0:
        raise ValueError('gl_momentum (--gl-momentum) must be in [0, 1), got %r' % (gl_momentum,))
    if int(n_iter) < 0:
        raise ValueError('n_iter (--gl-iters) must be >= 0, got %r' % (n_iter,))
    if deemphasis is not None and not 0.0 <= float(deemphasis) < 1.0:
        raise ValueError('deemphasis (--deemphasis) must be in [0, 1), got %r' % (deemphasis,))
    if trim_db is not None and not float(trim_db) > 0.0:
        raise ValueError('trim_db (--trim-db) must be > 0, got %r' % (trim_db,))


def limit_options(limit_ms=None, true_peak=None, limit_passes=None):
    """the limiter's keywords of level_waveform from the options (None: the default), checked; ValueError"""
    opt = dict(lookahead_ms=LIMIT_MS if limit_ms is None else limit_ms, oversample=lib.LIMIT_P if true_peak is None else true_peak,
               passes=LIMIT_PASSES if limit_passes is None else limit_passes)
    limit_settings('limit (--limit-ms, --true-peak, --limit-passes)', sr=SR, **opt)
    return dict(limit=True, **opt)


def write_prompt(out_dir, n, r, spec, align, wav=None, len_b=None, pcm=None, trim=None, conv=None, piece=None, ascore=None, zoom=4,
                 rate=None, pitch=None, f0=None, dur=None, prosody=None, loud=None):
    """The files of prompt n from its rows of the batch's arrays.  len_b (with a stop rule): the prompt keeps frames = min(len_b r, F)
    spectrogram frames, len_b alignment rows and the 300 (frames - 1) samples Griffin-Lim gives for that many frames (hop 300).
    piece (--long): the arrays of piece `piece` of a prompt of several, as prompt_NNN_kMM_*.npy; its samples are in the prompt's wav.
    ascore (--align-scores): the prompt's 8 alignment scores, written as _ascore.npy (float64) next to _align.png, the attention picture
    over the kept alignment rows at `zoom` pixels per cell.
    rate (--rate): (step_q, Fo_b) of the prompt, written as _rate.npy; wav is then the stretched waveform and keeps 300 (Fo_b - 1)
    samples, whatever len_b says.
    pitch (--pitch): (step_q, lifter) of the prompt, written as _pitch.npy; nothing else depends on it.
    f0 (--f0): the prompt's (frames, 2) float32 rows of (period, strength) over the frames the vocoder was given, already cut to them;
    written as _f0.npy.
    dur (--timings): the steps of each of the prompt's characters, written as _dur.npy (int32).
    prosody (--prosody): (the prompt's (L, 2) per-character (dur_q, step_q), Fo_b): the table is written as _prosody.npy (int32); wav is
    then the waveform behind the stretch curve and keeps 300 (Fo_b - 1) samples, whatever len_b says.
    loud (--loudness): the prompt's loud_row, written as _loud.npy (float64); pcm then holds the levelled samples.  With --limit: the
    prompt's limit_row, whose first 8 values are written as _limit.npy instead."""
    path = os.path.join(out_dir, 'prompt_%03d' % n if piece is None else 'prompt_%03d_k%02d' % (n, piece))
    if len_b is not None:
        frames = min(len_b * r, spec.shape[0])
        spec, align = spec[:frames], align[:len_b]
        if wav is not None and rate is None and prosody is None:
            wav = wav[:300 * (frames - 1)]
        np.save(path + '_len.npy', np.int32(len_b))
    if rate is not None:
        if wav is not None:
            wav = wav[:300 * max(0, int(rate[1]) - 1)]
        np.save(path + '_rate.npy', np.asarray(rate, dtype=np.int32))
    if pitch is not None:
        np.save(path + '_pitch.npy', np.asarray(pitch, dtype=np.int32))
    if prosody is not None:
        if wav is not None:
            wav = wav[:300 * max(0, int(prosody[1]) - 1)]
        np.save(path + '_prosody.npy', np.asarray(prosody[0], dtype=np.int32).reshape(-1, 2))
    if f0 is not None:
        np.save(path + '_f0.npy', np.asarray(f0, dtype=np.float32))
    if dur is not None:
        np.save(path + '_dur.npy', np.asarray(dur, dtype=np.int32))
    np.save(path + '_spec.npy', spec)
    np.save(path + '_align.npy', align)
    if wav is not None:
        write_wav(path + '.wav', wav)
    if pcm is not None:   # (finished on the device: already cut to the row's own samples, then trimmed to [s, e))
        write_wav_pcm(path + '.wav', pcm[:int(trim[1]) - int(trim[0])])
    if trim is not None:
        np.save(path + '_trim.npy', trim)
    if conv is not None:
        np.save(path + '_conv.npy', conv)
    if loud is not None:
        save_level(path, loud)
    if ascore is not None:
        np.save(path + '_ascore.npy', np.asarray(ascore, dtype=np.float64))
        attention_png(path + '_align.png', align, zoom=zoom)


def save_level(path, row):
    """a loud_row -> path_loud.npy; a limit_row -> its 8 values of path_limit.npy"""
    row = np.asarray(row, dtype=np.float64)
    np.save(path + ('_limit.npy' if len(row) == 9 else '_loud.npy'), row[:8])


def test(config, prompts, out_dir='log/test', checkpoint=None, speaker=0, n_iter=50, vocode=True, stop=None, vocode_lengths=False,
         gl_momentum=None, deemphasis=None, trim_db=None, long=None, align_scores=False, rate=None, pitch=None, lifter=32, f0=None,
         timings=False, path_jump=lib.PATH_JUMP, f0_smooth=None, prosody=None, gl_init=None, loudness=None, peak_db=None, limit=False,
         limit_ms=None, true_peak=None, limit_passes=None):
    """test.py:13-70: restore the checkpoint (weights AND stft_mean / stft_std, test.py:27-28), run every prompt batch,
    de-normalise `out * stft_std + stft_mean` (test.py:64), undo the r-frame layout and invert with Griffin-Lim -- all on the
    GPU (lib.denorm_unframe, tacotron_amd.griffinlim).  ONE Tacotron (workspace + outputs) serves every batch of the same
    size; only a smaller final batch builds a second one.  `speaker`: id fed to a multi-speaker model for every prompt
    (data_input.py:101-106 feeds none: the reference's test.py cannot drive its own VCTK model).
    `stop`: a lib.TacoStopRule, or None for the reference's fixed max_decode_iter steps.  With a rule, prompt i keeps len_b decoder
    steps: len_b r spectrogram frames, len_b alignment rows and the 300 (len_b r - 1) samples Griffin-Lim gives for that many frames
    (the vocoder still runs over the full, zero-filled length); len_b goes to prompt_NNN_len.npy.
    `vocode_lengths` (needs `stop`): the vocoder gets model.lengths and runs over each prompt's own frames only; the files keep
    their sizes, the samples are the Griffin-Lim of that prompt alone, from phases drawn on the device (seed = index of the batch's
    first prompt).
    `gl_momentum`: None, or the momentum of the fast Griffin-Lim rounds; prompt_NNN_conv.npy then holds the n_iter + 1 convergence
    values of the prompt (over the frames the vocoder ran on: the prompt's own with `vocode_lengths`, else the full length).
    `deemphasis` (None, or a in [0, 1)) / `trim_db` (None, or decibels > 0): with either, the batch's waveform is finished on the
    device (finish_waveform; with `stop`, each row over the samples of its own len_b r frames) and prompt_NNN.wav is written from
    the device's int16 samples: e - s of them, [s, e] in prompt_NNN_trim.npy.  The other files are unchanged.
    `long` (needs `stop` and `vocode`): None, True, or a dict with 'pause_ms' (SENTENCE, CLAUSE, WORD; default 300, 150, 0) and / or
    'fade_ms' (default 5) -- choices, not tuned by ear.  Every prompt is cut into pieces of at most 140 characters (data.split_prompt),
    the pieces run in order as rows of batches of <= 32, every batch is finished on the device into its rows of one buffer (without
    `deemphasis` / `trim_db`: bounds [0, n_b)), and the pieces of each prompt are joined there (join_waveform), <= 256 pieces and the
    rest of the prompt they end in per call.  prompt_NNN.wav holds the prompt's total samples, prompt_NNN_pieces.npy (K, 4) int32
    offset, length, gap, kind per piece, prompt_NNN_kMM_*.npy the arrays of piece MM; a prompt of one piece writes the files and the
    contents it writes without `long`.
    `align_scores`: every batch is scored on the device (Tacotron.alignment_scores: over model.lengths with `stop`, else all steps) and
    each prompt -- with `long`, each piece -- additionally writes _ascore.npy and _align.png (write_prompt); a prompt whose scores
    alignment.flags marks is named in one WARNING line.  Nothing else changes.
    `rate` (needs `vocode`): None, a speaking rate in [0.25, 4] (1.0: the model's own) or a sequence with one rate per prompt; with
    `long`, a prompt's pieces inherit its rate.  The magnitudes of every row are stretched on the device in front of Griffin-Lim
    (invert_spectrogram(rate=...)): over the row's own len_b r frames with `stop` (whether or not `vocode_lengths` is set; the phases
    are then drawn on the device), else over all frames.  prompt_NNN.wav holds 300 (Fo_b - 1) samples, Fo_b = lib.stretch_frames of
    those frames -- cut on the host by that formula, or with finishing on the device from the stretch's own frames_out -- and
    prompt_NNN_rate.npy (step_q, Fo_b) as int32.  Every other file is the model's own output, unstretched; without `rate` every file
    is what it was.
    `pitch` (needs `vocode`) / `lifter`: None, a pitch shift in semitones in [-12, 12] (0: the model's own) or a sequence with one per
    prompt; with `long`, a prompt's pieces inherit its pitch.  The harmonics of every magnitude frame the vocoder is given are moved
    under the frame's own envelope of `lifter` quefrencies (invert_spectrogram(pitch=...), in front of the stretch of `rate`): over the
    row's own len_b r frames wherever the vocoder gets the lengths, else over all frames.  prompt_NNN_pitch.npy holds (step_q, lifter)
    as int32; no file changes its size, the model's own files stay what they are, and pitch 0 gives the audio of pitch None.
    `f0` (needs `vocode`): None, True (60 .. 400 Hz) or (lo, hi) in Hz: invert_spectrogram(f0=...) tracks the pitch of the frames on the
    device, over the row's own len_b r frames with `stop`; prompt_NNN_f0.npy holds (period, strength) of the frames the vocoder was
    given, and f0_lines() prints what `pitch` or `rate` did to it.  Untuned, and meaningless on an untrained model; nothing else
    changes.
    `f0_smooth` (needs `f0`): None, True (lib.F0_CANDIDATES candidates per frame) or their number in 1 .. 15: the tracks are smoothed
    across frames on the device (invert_spectrogram(f0={'smooth': ...}), lib.f0_viterbi with lib.f0_viterbi_tables' UNTUNED bias and
    costs for the range of `f0`); _f0.npy and f0_lines() use the smoothed track and the line names the frames the smoothing moved.
    `timings` / `path_jump`: every batch's best monotone attention paths are found on the device (Tacotron.alignment_path with
    max_jump = path_jump: over model.lengths with `stop`, else all steps); each prompt -- with `long`, each piece -- additionally
    writes _dur.npy, each prompt _words.tsv (alignment.word_times of the file it wrote) and one line, a WARNING when the path ends
    before the text does.  Nothing else changes.
    `prosody` (needs `stop` and `vocode`, excludes `long`): None, or the rows of parse_prosody -- (prompt, word, rate | None,
    semitones | None) -- rate and pitch per word; words not listed take `rate` / `pitch`, or stay neutral.  Per batch, all on the
    device: the path (Tacotron.alignment_path, max_jump = path_jump), two lib.path_curve gathers of the per-character dur_q / step_q
    into per-frame curves, then invert_spectrogram(rate_curve=..., pitch_curve=...) over each row's own len_b r frames (the pitch curve
    only when a pitch is asked for anywhere).  prompt_NNN.wav holds 300 (Fo_b - 1) samples, Fo_b the stretch's frames_out (with finishing
    the row ends there on the device); prompt_NNN_prosody.npy the per-character (dur_q, step_q); _rate.npy / _pitch.npy are not written.
    With `timings` the word rows go through the stretch's time map (alignment.word_times(src=...)); with `f0` the line is the drift
    line without a figure asked for.
    `gl_init` (needs `vocode` for 'estimate'): None or 'random' -- every file is what it was -- or 'estimate': Griffin-Lim starts from
    phases read off the magnitudes it is handed (invert_spectrogram(phase_init='estimate'), lib.phase_estimate), on whichever path the
    other options choose; with n_iter = 0 the waveform is the estimate's own synthesis pass.  No file changes its size.
    `loudness` (needs `vocode`) / `peak_db`: None, or the target in LUFS in [-70, 0] and the ceiling on the sample peak in decibels
    <= 0 (None: -1).  The waveform is finished on the device as with `long` (without `deemphasis` / `trim_db`: bounds [0, n_b)) and
    the finished rows are levelled there (level_waveform over each row's own e - s samples); with `long` the JOINED prompts are
    levelled, after join_waveform.  prompt_NNN.wav holds the levelled int16 samples, prompt_NNN_loud.npy the prompt's loud_row, and
    loud_line() is printed per prompt.  Without it lib.wave_loudness is never reached and every file is what it was.
    `limit` (needs `loudness`) / `limit_ms` / `true_peak` / `limit_passes`: the true-peak limiter (level_waveform(limit=True),
    taco_wave_limit): the prompt gets the gain its target asks for and only the neighbourhood of a peak is pulled down; `peak_db` then
    is the ceiling on the TRUE peak (dBTP).  None: LIMIT_MS of look-ahead, lib.LIMIT_P x oversampling, LIMIT_PASSES passes -- untuned,
    and nobody has listened to a limited file.  prompt_NNN.wav holds the limited int16 samples, prompt_NNN_limit.npy (tp_in, G, g_min, peak_out, n_b,
    n_limited, I_reached, tp_out) as float64 (no _loud.npy), and limit_line() is printed per prompt.  Without it lib.wave_limit is
    never reached."""
    check_options(n_iter, stop, vocode_lengths, gl_momentum, deemphasis, trim_db, long, rate, vocode, pitch, lifter, f0,
                  f0_smooth=f0_smooth, path_jump=path_jump if timings else None, prosody=prosody, gl_init=gl_init, loudness=loudness,
                  peak_db=peak_db, limit=limit, limit_ms=limit_ms, true_peak=true_peak, limit_passes=limit_passes)
    level = None if loudness is None else dict(target=float(loudness), ceiling_db=PEAK_DB if peak_db is None else float(peak_db))
    if limit:
        level.update(limit_options(limit_ms, true_peak, limit_passes))
    gl_init = None if gl_init == 'random' else gl_init
    if prosody is not None and prosody is not False:
        lib.int_arg('check_options', 'path_jump (--path-jump)', path_jump, 1, lib.PATH_MAX_JUMP)
    else:
        prosody = None
    f0_smooth = None if f0_smooth is None or f0_smooth is False else (lib.F0_CANDIDATES if f0_smooth is True else int(f0_smooth))
    f0 = f0_range(f0)
    f0_opt = None   # the tables on the device, made at the first batch
    steps = rate_steps(rate, len(prompts))
    row_pitch = pitch_steps(pitch, len(prompts))
    long = long_options(long)
    if long is not None and not vocode:
        raise ValueError('long (--long) joins waveforms: it needs vocode')
    finish = deemphasis is not None or trim_db is not None or long is not None or level is not None
    meta_path = os.path.join(config.data_path, 'meta.pkl')
    if os.path.exists(meta_path):
        with open(meta_path, 'rb') as f:
            ivocab = pkl.load(f)['vocab']
    else:
        ivocab = {i + 1: ch for i, ch in enumerate("abcdefghijklmnopqrstuvwxyz '.,?!-")}
        ivocab[0] = '<pad>'
    config.vocab_size = len(ivocab)
    ckpt = torch.load(checkpoint) if checkpoint else None
    if ckpt is not None:
        config.r, config.vocab_size = ckpt.get('shape', (config.r, config.vocab_size))
        config.num_speakers = int(ckpt.get('num_speakers', 1))
    pros = None   # per prompt: (L, 2) int32 (dur_q, step_q) per encoded character
    if prosody is not None:   # the curves carry --rate and --pitch as the value of every character no row of the table names
        pros = prosody_table(prosody, prompts, ivocab, _steps('rate', rate, lib.stretch_dur, len(prompts)), row_pitch)
        pros_pitch = row_pitch is not None or any(sem is not None for _, _, _, sem in prosody)
        pros_max = max([lib.STRETCH_ONE] + [int(t[:, 0].max()) for t in pros if len(t)])
        steps = row_pitch = None
    state = {'params': None}
    models = {}   # batch size -> Tacotron
    os.makedirs(out_dir, exist_ok=True)

    def synthesise(batch, n, out_rows=None, bounds_rows=None):
        """one batch whose first row has index n -> (spec, align, wav, conv, pcm, trim, lengths, scores, f0res, paths, curved, louds),
        host arrays or None.  louds (`loudness` without `long`): the batch's loud_rows (B, 8); pcm then is the levelled one.  curved (`prosody`): (frames_out (B), src (B, Fo)) of the stretch curve.  paths (`timings`): (dur (B, Tt), counts (B, 3), mass (B)) of the best monotone paths.
        out_rows / bounds_rows (`long`): the finished fp32 samples and their bounds go to these device rows and no PCM16 is made.
        f0res (`f0`): (track (B, Fv, 2), model_stats, vocoder_stats, pitch_stats | None, and with `f0_smooth` the vocoder track's
        lib.f0_viterbi counts (B, 4))"""
        nonlocal f0_opt
        Bn = batch['text'].shape[0]
        if config.num_speakers > 1:
            batch['speaker'] = torch.full((Bn,), int(speaker), dtype=torch.int32)
        if state['params'] is None:
            shape = lib.make_shape(Bn, batch['text'].shape[1], config.max_decode_iter, config.r, config.vocab_size,
                                   config.num_speakers)
            state['params'] = ParamBuffer(shape, 'cuda').init_(0)
        model = models.get(Bn)
        if model is None:
            model = models[Bn] = Tacotron(config, batch, train=False, params=state['params'])
            if ckpt is not None:
                model.load_state_dict(ckpt)
        else:
            model.set_inputs(batch)
        out, al = model.run(stop=stop)
        scores = model.alignment_scores() if align_scores else None   # (enqueued behind the decode; read with the other results below)
        found = model.alignment_path(path_jump) if timings or pros is not None else None   # (likewise; the path stays on the device)
        paths = found[1:] if timings else None
        model.check()
        mean = model.stft_mean if model.stft_mean is not None else torch.zeros(config.fft_size * config.r)
        std = model.stft_std if model.stft_std is not None else torch.ones(config.fft_size * config.r)
        mean = torch.as_tensor(mean, dtype=torch.float32).cuda()
        std = torch.as_tensor(std, dtype=torch.float32).cuda()
        spec = lib.denorm_unframe(out, mean, std, config.r)                       # (B, Td*r, 1025) chronological log-magnitudes
        wav = conv = pcm = trim = f0res = curved = louds = None
        level_rows = level is not None and out_rows is None   # (`long` levels the joined prompts instead)
        if vocode:
            fout = None
            shift = {}
            if row_pitch is not None:   # (step_q as the device takes it: no way back through semitones)
                shift = dict(pitch=torch.tensor(row_pitch[n:n + Bn], dtype=torch.int32).cuda(), lifter=lifter)
            if f0 is not None:
                if f0_opt is None:
                    w, g, lag_min, lag_max = lib.f0_tables(SR, f0[0], f0[1])
                    f0_opt = dict(weight=torch.from_numpy(w).cuda(), gain=torch.from_numpy(g).cuda(), lag_min=lag_min, lag_max=lag_max)
                    if f0_smooth is not None:
                        bias, lg, jump, switch = lib.f0_viterbi_tables(SR, f0[0], f0[1])
                        f0_opt['smooth'] = dict(bias=torch.from_numpy(bias).cuda(), lg=torch.from_numpy(lg).cuda(), candidates=f0_smooth,
                                                jump_cost=jump, switch_cost=switch)
                shift['f0'] = dict(f0_opt, lengths=model.lengths if stop is not None else None)
            if pros is not None:
                Tt, Fm = batch['text'].shape[1], (out.shape[1] // 4) * 4 * config.r
                values = np.empty((2, Bn, Tt), dtype=np.int32)
                values[0], values[1] = lib.STRETCH_ONE, lib.PITCH_ONE
                for i in range(Bn):
                    table = pros[n + i][:Tt]
                    values[:, i, :len(table)] = table.T
                values = torch.from_numpy(values).cuda()
                curves = [lib.path_curve(found[0], values[k], config.r, one)[:, :Fm].contiguous()
                          for k, one in ((0, lib.STRETCH_ONE), (1, lib.PITCH_ONE)) if k == 0 or pros_pitch]
                res = invert_spectrogram(out, mean, std, config.r, n_iter=n_iter, seed=n, momentum=gl_momentum,
                                         want_conv=gl_momentum is not None, phase_init=gl_init, lengths=model.lengths, rate_curve=curves[0],
                                         pitch_curve=curves[1] if pros_pitch else None, lifter=lifter, dur_q_max=pros_max, **shift)
            elif steps is None:
                res = invert_spectrogram(out, mean, std, config.r, n_iter=n_iter, seed=n, momentum=gl_momentum,
                                         want_conv=gl_momentum is not None, phase_init=gl_init, lengths=model.lengths if vocode_lengths else None, **shift)
            else:   # (the rows' own frames whenever there is a rule: the host's Fo_b and the device's frames_out are then one number)
                res = invert_spectrogram(out, mean, std, config.r, n_iter=n_iter, seed=n, momentum=gl_momentum,
                                         want_conv=gl_momentum is not None, phase_init=gl_init, lengths=model.lengths if stop is not None else None,
                                         rate=[q / 65536.0 for q in row_steps[n:n + Bn]], **shift)
            res = list(res) if isinstance(res, tuple) else [res]   # waveform [, conv] [, frames_out] [, tracks]
            if f0 is not None:
                tracks = res.pop()
                f0res = (torch.stack(tracks['vocoder'], dim=2).cpu().numpy(), tracks['model_stats'].cpu().numpy(),
                         tracks['vocoder_stats'].cpu().numpy(), tracks['pitch_stats'].cpu().numpy() if 'pitch_stats' in tracks else None)
                if f0_smooth is not None:
                    f0res += (tracks['vocoder_counts'].cpu().numpy(),)
            if pros is not None:
                src = res.pop()
            if steps is not None or pros is not None:
                fout = res.pop()
            if pros is not None:
                curved = (fout.cpu().numpy(), src.cpu().numpy())
            wav = res[0] if gl_momentum is None else res
            if gl_momentum is not None:
                wav, conv = wav[0], wav[1].cpu().numpy()
                print('Griffin-Lim momentum %g, %d rounds: worst final spectral convergence of the batch %.4f'
                      % (gl_momentum, n_iter, float(conv[:, -1].max())))
            if finish and fout is not None:   # (a rate: the row ends where the stretch says; `long`: the rows are wider than this batch's)
                fin, pcm, trim, _ = finish_waveform(wav, fout, 1, deemphasis=0.0 if deemphasis is None else deemphasis,
                                                    trim_top_db=0.0 if trim_db is None else trim_db,
                                                    want_out=out_rows is not None or level_rows,
                                                    want_pcm=out_rows is None and not level_rows, bounds=bounds_rows)
                if out_rows is not None:
                    out_rows[:, :fin.shape[1]].copy_(fin)
            elif finish:   # (the fp32 waveform stays on the device)
                fin, pcm, trim, _ = finish_waveform(wav, model.lengths if stop is not None else None, config.r,
                                                    deemphasis=0.0 if deemphasis is None else deemphasis,
                                                    trim_top_db=0.0 if trim_db is None else trim_db,
                                                    want_out=out_rows is not None or level_rows,
                                                    want_pcm=out_rows is None and not level_rows, out=out_rows, bounds=bounds_rows)
            else:
                wav = wav.cpu().numpy()
            if finish:
                if level_rows:   # (the finished fp32 rows stay on the device; their PCM16 is the levelled one)
                    pcm, louds = level_finished(fin, level, bounds=trim)
                pcm, trim, wav = None if pcm is None else pcm.cpu().numpy(), trim.cpu().numpy(), None
        lengths = model.lengths.cpu().numpy() if stop is not None else None
        if scores is not None:
            scores = np.stack([scores_row(c, m) for c, m in zip(scores[0].cpu().numpy(), scores[1].cpu().numpy())])
        if paths is not None:
            paths = tuple(x.cpu().numpy() for x in paths)
        return spec.cpu().numpy(), al.cpu().numpy(), wav, conv, pcm, trim, lengths, scores, f0res, paths, curved, louds

    def marks(score, L):
        """the flags of one row's 8 scores, against the stop rule's own target when there is a rule"""
        return flags(score[:6], score[6:], L, end_offset=stop.end_offset if stop is not None else 1)

    F = (config.max_decode_iter // 4) * 4 * config.r   # frames per row of the model's output

    def rate_of(row, len_b):
        """(step_q, Fo_b) of global row `row`, or None without a rate"""
        if steps is None:
            return None
        return row_steps[row], lib.stretch_frames(F if len_b is None else min(int(len_b) * config.r, F), row_steps[row])

    def pitch_of(row):
        """(step_q, lifter) of global row `row`, or None without a pitch"""
        return None if row_pitch is None else (row_pitch[row], int(lifter))

    def f0_of(row, i, len_b, f0res, who, curved=None):
        """the _f0.npy rows of row i of a batch (global row `row`), cut to the frames the vocoder was given; prints the row's line"""
        if f0res is None:
            return None
        stretched = rate_of(row, len_b)
        frames = stretched[1] if stretched is not None else (F if len_b is None else min(int(len_b) * config.r, F))
        if curved is not None:
            frames = int(curved[0][i])
        for line in f0_lines(who, [None if a is None else a[i] for a in f0res[1:]], None if row_pitch is None else row_pitch[row],
                             None if steps is None else row_steps[row], curved is not None):
            print(line)
        return f0res[0][i, :frames]

    def timing_of(row, i, len_b, trim, paths, text_len, line, who, offset=0, curved=None):
        """(_dur.npy of row i of a batch (global row `row`), its word rows in the file it goes to) with `timings`, else (None, None);
        prints the row's line.  trim: the row's [s, e] when the waveform was finished; offset: of the piece in a joined file; curved
        (`prosody`): the batch's (frames_out, src) -- the word boundaries then go through the row's time map"""
        if paths is None:
            return None, None
        dur, counts, mass = (a[i] for a in paths)
        print(path_line(who, counts, mass, text_len, stop.end_offset if stop is not None else 1)[0])
        stretched = rate_of(row, len_b)
        frames = stretched[1] if stretched is not None else (F if len_b is None else min(int(len_b) * config.r, F))
        if curved is not None:
            frames = int(curved[0][i])
            return dur[:text_len], word_times(line, ivocab, dur[:text_len], config.r, None, trim, offset, 300 * max(0, frames - 1), SR,
                                              src=curved[1][i, :frames])
        words = word_times(line, ivocab, dur[:text_len], config.r, None if steps is None else row_steps[row], trim, offset,
                           300 * max(0, frames - 1), SR)
        return dur[:text_len], words

    def write_words(n, words):
        with open(os.path.join(out_dir, 'prompt_%03d_words.tsv' % n), 'w') as f:
            f.write(words_tsv(words))

    n = 0
    row_steps = steps
    if long is not None:
        if row_pitch is not None:
            row_pitch = [row_pitch[p] for p, line in enumerate(prompts) for _ in split_prompt(line)]
        L = None
        if steps is not None:   # a piece has its prompt's rate; every row of the joined buffer holds the slowest one's samples
            row_steps = [steps[p] for p, line in enumerate(prompts) for _ in split_prompt(line)]
            L = 300 * (max(5, lib.stretch_capacity(F, min(row_steps, default=lib.STRETCH_ONE))) - 1)
        n = _test_long(config, prompts, ivocab, out_dir, synthesise, long, marks, L, rate_of, pitch_of, f0_of,
                       timing_of if timings else None, write_words, level)
        print('wrote %d samples to %s' % (n, out_dir))
        return n
    for batch in load_prompts(prompts, ivocab):
        Bn = batch['text'].shape[0]
        spec, al, wav, conv, pcm, trim, lengths, scores, f0res, paths, curved, louds = synthesise(batch, n)
        for i in range(Bn):
            wi, len_b, pi, ti, ci, si, li = (None if a is None else a[i] for a in (wav, lengths, pcm, trim, conv, scores, louds))
            dur, words = timing_of(n, i, len_b, ti, paths, int(batch['text_length'][i]), prompts[n], 'prompt %d' % n, curved=curved)
            write_prompt(out_dir, n, config.r, spec[i], al[i], wi, None if len_b is None else int(len_b), pi, ti, ci, ascore=si,
                         rate=rate_of(n, len_b), pitch=pitch_of(n), f0=f0_of(n, i, len_b, f0res, 'prompt %d' % n, curved), dur=dur,
                         prosody=None if curved is None else (pros[n], int(curved[0][i])), loud=li)
            if li is not None:
                print(level_line('prompt %d' % n, li, level))
            if words is not None:
                write_words(n, words)
            found = marks(si, int(batch['text_length'][i])) if si is not None else []
            if found:
                print('WARNING prompt %d: %s' % (n, ', '.join(found)))
            n += 1
    print('wrote %d samples to %s' % (n, out_dir))
    return n


def _test_long(config, prompts, ivocab, out_dir, synthesise, long, marks, L=None, rate_of=lambda row, len_b: None,
               pitch_of=lambda row: None, f0_of=lambda row, i, len_b, f0res, who: None, timing_of=None, write_words=None, level=None):
    """the `long` mode of test(): split, synthesise the pieces into the rows of one device buffer per group, join, write.  L: the samples
    per row when a rate makes them more or fewer than the model's own; rate_of(row, len_b) / pitch_of(row) / f0_of(row, i, len_b, f0res,
    who): what write_prompt gets as `rate` / `pitch` / `f0`; timing_of / write_words (`timings`): test()'s own, called once the joined
    offsets of a group are known; level (`loudness`): level_waveform's target and ceiling_db -- the joined prompts are levelled"""
    pause_ms, fade_ms = long
    split = [split_prompt(p) for p in prompts]
    groups, start = [], 0   # [prompt lo, prompt hi): a group ends at the first prompt boundary at which it holds >= JOIN_GROUP pieces
    held = 0
    for p, pieces in enumerate(split):
        held += len(pieces)
        if held >= JOIN_GROUP or p == len(split) - 1:
            groups.append((start, p + 1))
            start, held = p + 1, 0
    if L is None:
        L = 300 * ((config.max_decode_iter // 4) * 4 * config.r - 1)   # samples per row of invert_spectrogram
    who = ['prompt %d' % p if len(pieces) == 1 else 'prompt %d piece %d' % (p, k) for p, pieces in enumerate(split) for k in range(len(pieces))]
    row = 0   # index of the next piece over the whole run (the Griffin-Lim seed of its batch, as the prompt index is without `long`)
    for lo, hi in groups:
        lines = [line for pieces in split[lo:hi] for line, _ in pieces]
        kinds = [kind for pieces in split[lo:hi] for _, kind in pieces]
        first = np.concatenate([[0], np.cumsum([len(pieces) for pieces in split[lo:hi]])]).astype(np.int64).tolist()
        N = len(lines)
        rows = torch.empty(N, L, dtype=torch.float32, device='cuda')
        bounds = torch.empty(N, 2, dtype=torch.int32, device='cuda')
        arrays = []   # per piece: (spec, align, len_b, trim, conv, scores, text length, f0 rows)
        timed = []    # per piece with `timings`: (the batch's paths, row in the batch)
        at = 0
        for batch in load_prompts(lines, ivocab):
            Bn = batch['text'].shape[0]
            spec, al, _, conv, _, trim, lengths, scores, f0res, paths, _, _ = synthesise(batch, row + at, rows[at:at + Bn], bounds[at:at + Bn])
            timed += [(paths, i) for i in range(Bn)]
            arrays += [(spec[i], al[i], int(lengths[i]), trim[i], None if conv is None else conv[i],
                        None if scores is None else scores[i], int(batch['text_length'][i]),
                        f0_of(row + at + i, i, int(lengths[i]), f0res, who[row + at + i])) for i in range(Bn)]
            at += Bn
        gap = join_gaps(kinds, pause_ms)
        louds = None
        if level is None:
            _, pcm, offsets, total, _ = join_waveform(rows, bounds, first, kinds, pause_ms=pause_ms, fade_ms=fade_ms, want_out=False)
        else:   # (the joined fp32 prompts stay on the device; their PCM16 is the levelled one)
            joined, _, offsets, total, _ = join_waveform(rows, bounds, first, kinds, pause_ms=pause_ms, fade_ms=fade_ms, want_pcm=False)
            pcm, louds = level_finished(joined, level, total=total)
        pcm, total, offsets = pcm.cpu().numpy(), total.cpu().numpy(), offsets.cpu().numpy()   # (the one copy back of the group)
        for p in range(lo, hi):
            a, b = first[p - lo], first[p - lo + 1]
            path = os.path.join(out_dir, 'prompt_%03d' % p)
            found, words = [], []
            for k in range(a, b):
                spec, al, len_b, trim, conv, score, text_len, f0rows = arrays[k]
                dur = None
                if timing_of is not None:
                    dur, piece_words = timing_of(row + k, timed[k][1], len_b, trim, timed[k][0], text_len, lines[k], who[row + k],
                                                 int(offsets[k]))
                    words += piece_words
                write_prompt(out_dir, p, config.r, spec, al, None, len_b, None, trim, conv, piece=None if b - a == 1 else k - a, ascore=score,
                             rate=rate_of(row + k, len_b), pitch=pitch_of(row + k), f0=f0rows, dur=dur)
                names = marks(score, text_len) if score is not None else []
                if names:
                    found.append(', '.join(names) if b - a == 1 else 'piece %d %s' % (k - a, ', '.join(names)))
            if found:
                print('WARNING prompt %d: %s' % (p, '; '.join(found)))
            write_wav_pcm(path + '.wav', pcm[p - lo, :int(total[p - lo])])
            if louds is not None:
                save_level(path, louds[p - lo])
                print(level_line('prompt %d' % p, louds[p - lo], level))
            if timing_of is not None:
                write_words(p, words)
            if b - a > 1:
                table = [[int(offsets[k]), min(L, max(0, int(arrays[k][3][1]) - int(arrays[k][3][0]))), 0 if k == b - 1 else gap[k],
                          kinds[k]] for k in range(a, b)]
                np.save(path + '_pieces.npy', np.array(table, dtype=np.int32))
                print('prompt %d: %d pieces (%s), %d samples' % (p, b - a, ' '.join(KIND_NAMES[kinds[k]] for k in range(a, b)),
                                                                 int(total[p - lo])))
        row += N
    return len(split)


def _pause_ms(text):
    parts = text.split(',')
    if len(parts) != 3:
        raise argparse.ArgumentTypeError('expected SENTENCE,CLAUSE,WORD, got %r' % text)
    return tuple(float(x) for x in parts)


def _f0_range(text):
    parts = text.split(',')
    if len(parts) != 2:
        raise argparse.ArgumentTypeError('expected LO,HI in Hz, got %r' % text)
    return tuple(float(x) for x in parts)


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('-t', '--train-set', default='nancy')
    ap.add_argument('--checkpoint', default=None)
    ap.add_argument('--speaker', type=int, default=0, help='speaker id for a multi-speaker checkpoint')
    ap.add_argument('--out-dir', default='log/test')
    ap.add_argument('--stop', action='store_true', help='end each prompt where its attention ends (not in the reference)')
    ap.add_argument('--end-offset', type=int, default=1, help='--stop: argmax target is character L - 1 - end_offset')
    ap.add_argument('--hold', type=int, default=4, help='--stop: consecutive steps at or past the target')
    ap.add_argument('--min-steps', type=int, default=8, help='--stop: steps before the rule may fire')
    ap.add_argument('--vocode-lengths', action='store_true',
                    help='--stop: Griffin-Lim over the frames of each prompt alone, phases drawn on the device')
    ap.add_argument('--gl-momentum', type=float, default=None,
                    help='fast Griffin-Lim rounds with this momentum in [0, 1) (0.99: librosa\'s default); writes prompt_NNN_conv.npy')
    ap.add_argument('--gl-iters', type=int, default=50, help='Griffin-Lim rounds (the reference: 50)')
    ap.add_argument('--gl-init', choices=('random', 'estimate'), default='random',
                    help='where Griffin-Lim starts: random phases (the default; every file is what it was), or an estimate read off the '
                         'magnitudes on the device (single-pass spectrogram inversion); --gl-iters 0 --gl-init estimate is a draft voice '
                         'without any round (not in the reference; nobody has listened to it)')
    ap.add_argument('--deemphasis', type=float, nargs='?', const=0.97, default=None, metavar='A',
                    help='undo the training features\' pre-emphasis on the device: y[n] = x[n] + A y[n-1], A in [0, 1) (default 0.97)')
    ap.add_argument('--trim-db', type=float, default=None, metavar='DB',
                    help='cut leading / trailing silence more than DB > 0 decibels below the loudest frame; writes prompt_NNN_trim.npy')
    ap.add_argument('--long', action='store_true',
                    help='--stop: cut a line of more than 140 characters where a speaker would pause, synthesise the pieces and join '
                         'them on the device into one prompt_NNN.wav (not in the reference)')
    ap.add_argument('--pause-ms', type=_pause_ms, default=PAUSE_MS, metavar='SENTENCE,CLAUSE,WORD',
                    help='--long: milliseconds of silence behind a piece cut after .?! / after ,;: / at a word boundary (default '
                         '300,150,0: choices of the author, not tuned by ear; a cut inside a word gets none)')
    ap.add_argument('--fade-ms', type=float, default=FADE_MS,
                    help='--long: milliseconds of linear ramp at every interior edge of a piece (default 5: a choice, not tuned by ear)')
    ap.add_argument('--rate', type=float, default=None, metavar='R',
                    help='speaking rate, 0.25 <= R <= 4: 1.0 is the model\'s own, 0.8 slower, 1.25 faster; the magnitudes are stretched on '
                         'the device in front of Griffin-Lim, so the pitch stays; writes prompt_NNN_rate.npy (not in the reference)')
    ap.add_argument('--pitch', type=float, default=None, metavar='SEMITONES',
                    help='pitch shift, -12 <= SEMITONES <= 12: 0 is the model\'s own, 3 higher, -3 lower; the harmonics of every magnitude '
                         'frame are moved under its own spectral envelope on the device in front of Griffin-Lim, so the formants and the '
                         'duration stay; writes prompt_NNN_pitch.npy (not in the reference)')
    ap.add_argument('--lifter', type=int, default=32, metavar='Q',
                    help='--pitch: the quefrencies 0 .. Q of the cepstrum make the envelope, 1 <= Q <= 64 (default 32 = 2 ms at 16 kHz: '
                         'a choice, not tuned by ear)')
    ap.add_argument('--f0', action='store_true',
                    help='measure the pitch of every magnitude frame the vocoder is given on the device; writes prompt_NNN_f0.npy (period '
                         'in samples, strength) and, with --pitch or --rate, prints what was asked for and what is measured (untuned '
                         'ratio 0.9 / threshold 0.3; meaningless on an untrained model; not in the reference)')
    ap.add_argument('--f0-range', type=_f0_range, default=None, metavar='LO,HI', help='--f0: the pitch range searched in Hz (default 60,400)')
    ap.add_argument('--f0-smooth', action='store_true',
                    help='--f0, with the track smoothed across frames on the device (a Viterbi path over the candidates of every frame, '
                         'untuned costs); _f0.npy and the per-prompt line use the smoothed track')
    ap.add_argument('--f0-candidates', type=int, default=None, metavar='K',
                    help='--f0-smooth: candidates kept per frame, 1 <= K <= 15 (default %d, untuned)' % lib.F0_CANDIDATES)
    ap.add_argument('--align-scores', action='store_true',
                    help='score every prompt\'s attention on the device: prompt_NNN_ascore.npy (8 values: n, end, pad_steps, back, skip, '
                         'covered, focus, pad_mass), prompt_NNN_align.png, and a WARNING line for a prompt the (untuned) thresholds mark')
    ap.add_argument('--timings', action='store_true',
                    help='when each word is spoken: the best monotone path through every prompt\'s attention, found on the device; writes '
                         'prompt_NNN_dur.npy (steps per character) and prompt_NNN_words.tsv (start_s, end_s, word); exact at multiples of 4 '
                         'decoder steps, nominal inside a block (not in the reference)')
    ap.add_argument('--prosody', default=None, metavar='FILE',
                    help='--stop: rate and pitch per word.  FILE holds lines prompt<TAB>word<TAB>rate<TAB>semitones, both indices '
                         '0-based, - in the rate or semitones field for "leave"; words not listed take --rate / --pitch or stay neutral.  '
                         'The curves follow the attention path on the device; writes prompt_NNN_prosody.npy (dur_q, step_q per character).  '
                         'Refused with --long: the pieces re-index the words of a prompt, which is out of scope (not in the reference)')
    ap.add_argument('--loudness', type=float, default=None, metavar='LUFS',
                    help='write every prompt at this integrated loudness (ITU-R BS.1770, measured and applied on the device), '
                         '-70 <= LUFS <= 0: -23 is EBU R 128, -16 to -19 voice assistants and podcasts; implies finishing; writes '
                         'prompt_NNN_loud.npy; with --long the joined prompt is levelled (not in the reference)')
    ap.add_argument('--peak-db', type=float, default=None, metavar='DB',
                    help='--loudness: the ceiling on the sample peak in decibels re full scale, DB <= 0 (default %g); where it binds, '
                         'the gain is what it allows' % PEAK_DB)
    ap.add_argument('--limit', action='store_true',
                    help='--loudness: give every prompt the gain its target asks for and hold its TRUE peak (inter-sample peaks read '
                         'through a polyphase interpolator) at --peak-db by a look-ahead limiter on the device that pulls down only the '
                         'neighbourhood of a peak; writes prompt_NNN_limit.npy.  The defaults below are untuned and nobody has listened '
                         'to a limited file (not in the reference)')
    ap.add_argument('--limit-ms', type=float, default=None, metavar='MS', help='--limit: the look-ahead in milliseconds (default %g)' % LIMIT_MS)
    ap.add_argument('--true-peak', type=int, default=None, metavar='P',
                    help='--limit: the oversampling of the true-peak meter, 1 <= P <= 8; 1 limits the sample peak (default %d)' % lib.LIMIT_P)
    ap.add_argument('--limit-passes', type=int, default=None, metavar='N',
                    help='--limit: passes of the limiter, each after the first re-aimed at the target, 1 <= N <= 8 (default %d)' % LIMIT_PASSES)
    ap.add_argument('--path-jump', type=int, default=None, metavar='J',
                    help='--timings / --prosody: characters a decoder step may advance on the path, 1 <= J <= 15 (default %d, untuned)' % lib.PATH_JUMP)
    a = ap.parse_args(argv)
    a.long = dict(pause_ms=a.pause_ms, fade_ms=a.fade_ms) if a.long else None
    if a.f0_candidates is not None and not a.f0_smooth:
        ap.error('--f0-candidates needs --f0-smooth')
    a.f0 = a.f0 or a.f0_smooth
    a.f0_smooth = (a.f0_candidates if a.f0_candidates is not None else True) if a.f0_smooth else None
    if a.f0_range is not None and not a.f0:
        ap.error('--f0-range needs --f0')
    a.f0 = (a.f0_range if a.f0_range is not None else True) if a.f0 else None
    if a.path_jump is not None and not a.timings and a.prosody is None:
        ap.error('--path-jump needs --timings or --prosody')
    a.path_jump = lib.PATH_JUMP if a.path_jump is None else a.path_jump
    try:
        check_options(a.gl_iters, a.stop, a.vocode_lengths, a.gl_momentum, a.deemphasis, a.trim_db, a.long, a.rate, pitch=a.pitch,
                      lifter=a.lifter, f0=a.f0, f0_smooth=a.f0_smooth, path_jump=a.path_jump if a.timings or a.prosody is not None else None,
                      prosody=a.prosody, gl_init=a.gl_init, loudness=a.loudness, peak_db=a.peak_db, limit=a.limit, limit_ms=a.limit_ms,
                      true_peak=a.true_peak, limit_passes=a.limit_passes)
        if a.prosody is not None:   # (the indices are held against the prompts in test(), once they are read)
            with open(a.prosody) as f:
                a.prosody = parse_prosody(f.read())
    except (ValueError, OSError) as e:
        ap.error(str(e))
    return a


if __name__ == '__main__':
    a = parse_args()
    prompts = [p for p in sys.stdin.readlines() if len(p) > 0]
    c = Config()
    c.data_path = 'data/%s/' % a.train_set
    c.save_path = a.train_set + '/tacotron'
    print('Building Tacotron')
    rule = lib.TacoStopRule(a.end_offset, a.hold, a.min_steps) if a.stop else None
    test(c, prompts, out_dir=a.out_dir, checkpoint=a.checkpoint, speaker=a.speaker, n_iter=a.gl_iters, stop=rule,
         vocode_lengths=a.vocode_lengths, gl_momentum=a.gl_momentum, deemphasis=a.deemphasis, trim_db=a.trim_db, long=a.long,
         align_scores=a.align_scores, rate=a.rate, pitch=a.pitch, lifter=a.lifter, f0=a.f0, timings=a.timings, path_jump=a.path_jump,
         f0_smooth=a.f0_smooth, prosody=a.prosody, gl_init=a.gl_init, loudness=a.loudness, peak_db=a.peak_db, limit=a.limit,
         limit_ms=a.limit_ms, true_peak=a.true_peak, limit_passes=a.limit_passes)
