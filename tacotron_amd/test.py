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
and after, the true peak and how much was limited.  With --long the JOINED prompt is limited.  Without --limit no new code is reached.
--sharpen BETA [--sharpen-lifter Q] (opt-in, not in the reference): spectral sharpening, -1 <= BETA <= 1.  Magnitudes trained under an
L1 loss have over-smoothed envelopes; directly behind the de-normalisation -- in front of --pitch, --rate, --prosody and --f0 -- every
magnitude frame goes through a cepstral post-filter on the device (lib.frames_sharpen, taco_frames_sharpen): the quefrencies 2 .. Q of
its cepstrum (default 32) are scaled by 1 + BETA and the frame keeps its energy.  prompt_NNN_sharpen.npy holds (beta, lifter) as
float64; every other file keeps its size, and the spectrogram, alignment, length and score files stay the model's own.  --sharpen 0 is
a run without the flag: the same files, byte for byte.  BETA and Q are UNTUNED and nobody has listened to the result;
`python -m tacotron_amd.evaluate --gv --sharpen BETA` gives the global-variance ratio with and without it.  It combines with every option
above; with --long every piece is sharpened.  The two settings are not fields of the options record of test(): they travel as
Config.sharpen / Config.sharpen_lifter, next to the paths the command line also leaves there, and a run reads them from its resolved
options like every other.
--pitch-range K [--pitch-range-smooth W] [--pitch-range-limit OCT] (opt-in, not in the reference): the intonation range, 0 <= K <= 4.
Where --pitch sits, the pitch of the frames in front of it is tracked on the device (lib.frames_f0; with --f0 that track, range and
smoothing are reused), lib.f0_range_curve (taco_f0_range_curve) turns the track into a per-frame pitch curve that multiplies every
frame's distance from the utterance's own level, in octaves, by K -- 0 a flat contour, 0.5 half the range, 1.5 half as wide again, the
cure for the flattened intonation of an L1-trained model that --f0 measures -- composed with --pitch or --prosody's pitch curve, and
the magnitudes go through lib.frames_pitch_curve.  W (default 2 frames) smooths the contour, OCT (default 0.5 octaves) caps the change
of one frame.  prompt_NNN_range.npy holds (scale_q, W, OCT, voiced frames, their mean log2 period, its deviation in front) as float64.
--pitch-range 1 is a run without the flag: the same files, byte for byte.  With --f0 one line per prompt says "range asked x1.50,
measured x1.46 (2.1 -> 3.1 semitones) over 212 voiced frames".  It combines with every option above; with --long every piece gets its
own centre.  K, W and OCT are UNTUNED, nobody has listened to the result, and on an untrained model the frames have no pitch: the
numbers then mean nothing.  The three settings travel as Config.pitch_range / pitch_range_smooth / pitch_range_limit.
--formant SEMITONES [--formant-lifter Q] (opt-in, not in the reference): timbre, -12 <= SEMITONES <= 12, the dual of --pitch.  Behind
--sharpen and in front of --pitch, --prosody's curves and --rate every magnitude frame goes through lib.frames_formant
(taco_frames_formant): the frame's envelope of Q quefrencies (default 32) is read at k / ratio, ratio = 2^(SEMITONES / 12) -- + moves
the formants up, a shorter vocal tract -- under the unmoved harmonics, and the frame keeps its energy.  prompt_NNN_formant.npy holds
(step_q, lifter) as int32; every other file keeps its name and size, and the spectrogram, alignment, length and score files stay the
model's own.  --formant 0 is a run without the flag: the same files, byte for byte.  With --f0 one line per prompt says "formant asked
+2.00 semitones, F0 moved +N cents over M voiced frames": the drift of the pitch, which should be none.  It combines with every option
above; with --long every piece is shifted, and with --prosody it is a per-row constant in front of the curves.  Q is UNTUNED and nobody
has listened to the result.  Like the sharpening pair the two settings travel as Config.formant / Config.formant_lifter and a run
reads them from its resolved options.
--ema (opt-in, with --checkpoint; not in the reference): the weights are the checkpoint's exponential moving average of the parameters
(`train --ema DECAY`) instead of the ones the last minibatch left.  A checkpoint without an average -- written without `train --ema`,
or imported from TF -- is refused before anything is synthesised.  Everything downstream is unchanged, and it combines with every
option above.  Nobody has listened to the difference."""
from __future__ import annotations

import argparse
import collections
import dataclasses
import os
import pickle as pkl
import sys
import wave
from typing import Any

import numpy as np
import torch

from .config import Config
from .alignment import attention_png, encoded_chars, flags, path_line, scores_row, word_times, word_values, words_tsv
from .data import KIND_NAMES, load_prompts, split_prompt
from .griffinlim import finish_waveform, join_gaps, join_samples, join_waveform, level_waveform, limit_settings, vocode
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


def formant_line(who, step_q, paired):
    """the line --f0 prints for `who` behind --formant from the row of 'formant_stats' (the formant track against the model's over
    the frames voiced in both): what was asked of the envelope, and how far the pitch moved with it -- which should be nowhere"""
    return ('%s formant asked %+.2f semitones, F0 moved %+.0f cents over %d voiced frames'
            % (who, 12.0 * np.log2(65536.0 / step_q), 1200.0 * float(paired[1]), int(paired[0])))


def range_line(who, row):
    """the line --f0 prints for `who` behind --pitch-range from (scale_q, the row of 'range_stats': the voiced frames behind the stage,
    the deviation of log2(period) in front of it and behind it, their ratio)"""
    scale_q, (count, sd_in, sd_out, ratio) = row
    return ('%s range asked x%.2f, measured x%.2f (%.1f -> %.1f semitones) over %d voiced frames'
            % (who, scale_q / 65536.0, float(ratio), 12.0 * float(sd_in), 12.0 * float(sd_out), int(count)))


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


FORMANT_LIFTER = 32   # --formant-lifter's default, lib.frames_formant's: UNTUNED, nobody has listened


def given(option):
    """whether an option whose None / False mean "off" is set"""
    return option is not None and option is not False


_OptionFields = dataclasses.make_dataclass('_OptionFields', frozen=True, fields=[(name, Any, default) for name, default in dict(
    n_iter=50, vocode=True, stop=None, vocode_lengths=False, gl_momentum=None, deemphasis=None, trim_db=None, long=None, align_scores=False,
    rate=None, pitch=None, lifter=32, f0=None, timings=False, path_jump=lib.PATH_JUMP, f0_smooth=None, prosody=None, gl_init=None,
    loudness=None, peak_db=None, limit=False, limit_ms=None, true_peak=None, limit_passes=None).items()])


class Options(_OptionFields):
    """The synthesis options of test(), a frozen record with test()'s names and defaults (the fields above); test() documents them.
    check() holds their ranges, resolved() what a run reads.  As the command line and check_options() see them: `stop` a rule, or
    True / None for given / not given; `prosody` None / False or anything else for given."""

    def check(self):
        """The option ranges of test() and of the command line (`path_jump` is held to its range with `timings`; `f0_smooth`: None /
        False, True or the number of candidates; `gl_init`: None, 'random' or 'estimate'; `peak_db`, `limit_ms`, `true_peak`,
        `limit_passes`: None for not given); ValueError."""
        o = self
        if o.loudness is not None:
            if not o.vocode:
                raise ValueError('loudness (--loudness) levels the waveform: it needs vocode')
            if not -70.0 <= float(o.loudness) <= 0.0:   # (NaN fails)
                raise ValueError('loudness (--loudness) must be in [-70, 0] LUFS, got %r' % (o.loudness,))
        if o.peak_db is not None:
            if o.loudness is None:
                raise ValueError('peak_db (--peak-db) is the ceiling of loudness (--loudness): it needs loudness')
            if not float(o.peak_db) <= 0.0 or np.isinf(float(o.peak_db)):
                raise ValueError('peak_db (--peak-db) must be a finite number of decibels <= 0, got %r' % (o.peak_db,))
        if not isinstance(o.limit, bool):
            raise ValueError('limit (--limit) must be True or False, got %r' % (o.limit,))
        if o.limit and o.loudness is None:
            raise ValueError('limit (--limit) holds the true peak of loudness (--loudness) at its ceiling: it needs loudness')
        for name, v in (('limit_ms (--limit-ms)', o.limit_ms), ('true_peak (--true-peak)', o.true_peak),
                        ('limit_passes (--limit-passes)', o.limit_passes)):
            if v is not None and not o.limit:
                raise ValueError('%s is a setting of limit (--limit): it needs limit' % name)
        if o.limit:
            limit_options(o.limit_ms, o.true_peak, o.limit_passes)
        if o.gl_init not in (None, 'random', 'estimate'):
            raise ValueError("gl_init (--gl-init) must be 'random' or 'estimate', got %r" % (o.gl_init,))
        if o.gl_init == 'estimate' and not o.vocode:
            raise ValueError('gl_init (--gl-init) estimates the phases Griffin-Lim starts from: it needs vocode')
        if given(o.prosody):
            if not o.vocode:
                raise ValueError('prosody (--prosody) shapes the magnitudes in front of Griffin-Lim: it needs vocode')
            if not o.stop:
                raise ValueError('prosody (--prosody) needs a stop rule (--stop): the curves follow the path over each prompt\'s own steps')
            if long_options(o.long) is not None:
                raise ValueError('prosody (--prosody) cannot be combined with long (--long): the pieces re-index the words of a prompt')
        if given(o.f0_smooth):
            if not given(o.f0):
                raise ValueError('f0_smooth (--f0-smooth) smooths the track of f0 (--f0): it needs f0')
            if o.f0_smooth is not True:
                lib.int_arg('check_options', 'f0_smooth (--f0-candidates)', o.f0_smooth, 1, lib.F0_MAX_CAND)
        if o.timings:
            lib.int_arg('check_options', 'path_jump (--path-jump)', o.path_jump, 1, lib.PATH_MAX_JUMP)
        if given(o.f0):
            if not o.vocode:
                raise ValueError('f0 (--f0) measures the magnitudes in front of Griffin-Lim: it needs vocode')
            f0_range(o.f0)
        if o.pitch is not None:
            if not o.vocode:
                raise ValueError('pitch (--pitch) shifts the magnitudes in front of Griffin-Lim: it needs vocode')
            pitch_steps(o.pitch, None)
            lib.int_arg('check_options', 'lifter (--lifter)', o.lifter, 1, lib.PITCH_MAX_LIFTER)
        if o.rate is not None:
            if not o.vocode:
                raise ValueError('rate (--rate) stretches the magnitudes in front of Griffin-Lim: it needs vocode')
            rate_steps(o.rate, None)
        if long_options(o.long) is not None and not o.stop:
            raise ValueError('long (--long) needs a stop rule (--stop): without one every piece carries max_decode_iter steps')
        if o.vocode_lengths and not o.stop:
            raise ValueError('vocode_lengths (--vocode-lengths) needs a stop rule (--stop): the lengths come from taco_infer_stop')
        if o.gl_momentum is not None and not 0.0 <= float(o.gl_momentum) < 1.0:
            raise ValueError('gl_momentum (--gl-momentum) must be in [0, 1), got %r' % (o.gl_momentum,))
        if int(o.n_iter) < 0:
            raise ValueError('n_iter (--gl-iters) must be >= 0, got %r' % (o.n_iter,))
        if o.deemphasis is not None and not 0.0 <= float(o.deemphasis) < 1.0:
            raise ValueError('deemphasis (--deemphasis) must be in [0, 1), got %r' % (o.deemphasis,))
        if o.trim_db is not None and not float(o.trim_db) > 0.0:
            raise ValueError('trim_db (--trim-db) must be > 0, got %r' % (o.trim_db,))
        if long_options(o.long) is not None and not o.vocode:
            raise ValueError('long (--long) joins waveforms: it needs vocode')

    def resolved(self, sharpen=None, sharpen_lifter=lib.SHARPEN_LIFTER, formant=None, formant_lifter=FORMANT_LIFTER, pitch_range=None,
                 pitch_range_smooth=lib.F0_RANGE_SMOOTH, pitch_range_limit=lib.F0_RANGE_LIMIT):
        """check(), then the options as a run reads them, a Resolved: `gl_init` None for 'random', `f0` None or (lo, hi), `f0_smooth`
        None or the number of candidates, `long` None or (pause_ms, fade_ms), `prosody` None when not given -- given, it holds
        `path_jump` to its range as `timings` does.  sharpen / sharpen_lifter (--sharpen, --sharpen-lifter; Config.sharpen /
        Config.sharpen_lifter): checked by sharpen_options, the Resolved holds what it returns; formant / formant_lifter (--formant,
        --formant-lifter; Config.formant / Config.formant_lifter) likewise by formant_options; pitch_range / pitch_range_smooth / pitch_range_limit (--pitch-range and
        its two settings; Config's fields of those names) by pitch_range_options; ValueError"""
        self.check()
        sharpen = sharpen_options(sharpen, sharpen_lifter, self.vocode)
        formant = formant_options(formant, formant_lifter, self.vocode)
        pitch_range = pitch_range_options(pitch_range, pitch_range_smooth, pitch_range_limit, self.vocode)
        level = None if self.loudness is None else dict(target=float(self.loudness),
                                                        ceiling_db=PEAK_DB if self.peak_db is None else float(self.peak_db))
        if self.limit:
            level.update(limit_options(self.limit_ms, self.true_peak, self.limit_passes))
        if given(self.prosody):
            lib.int_arg('check_options', 'path_jump (--path-jump)', self.path_jump, 1, lib.PATH_MAX_JUMP)
        smooth = (lib.F0_CANDIDATES if self.f0_smooth is True else int(self.f0_smooth)) if given(self.f0_smooth) else None
        f0, long = f0_range(self.f0), long_options(self.long)
        return Resolved(**dict(vars(self), gl_init=None if self.gl_init == 'random' else self.gl_init, f0=f0, f0_smooth=smooth, long=long,
                               prosody=self.prosody if given(self.prosody) else None), level=level,
                        finish=self.deemphasis is not None or self.trim_db is not None or long is not None or level is not None,
                        sharpen=sharpen, formant=formant, pitch_range=pitch_range)


@dataclasses.dataclass(frozen=True)
class Resolved(Options):
    """Options.resolved(): the options in the form a run reads, and what follows from them.  level: None, or level_waveform's target,
    ceiling_db and, with `limit`, limiter keywords; finish: whether the waveform is finished on the device; sharpen: None, or
    (beta, lifter) of the post-filter in front of every other stage; formant: None, or (step_q, lifter) of the formant shift
    behind it; pitch_range: None, or (scale_q, smooth, limit) of the intonation range where the pitch stage sits"""
    level: Any = None
    finish: bool = False
    sharpen: Any = None
    formant: Any = None
    pitch_range: Any = None


def sharpen_options(sharpen=None, sharpen_lifter=lib.SHARPEN_LIFTER, vocode=True):
    """--sharpen BETA / --sharpen-lifter Q -> None for no post-filter (BETA None or 0: every file is what it was), else
    (beta, lifter), checked against lib.frames_sharpen's ranges at the 1025 bins of the model; ValueError"""
    if sharpen is None:
        return None
    try:
        beta = float(sharpen)
        ok = not isinstance(sharpen, bool) and lib.SHARPEN_MIN_BETA <= beta <= lib.SHARPEN_MAX_BETA   # (NaN fails)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError('sharpen (--sharpen) must be a number in [%g, %g], got %r' % (lib.SHARPEN_MIN_BETA, lib.SHARPEN_MAX_BETA, sharpen))
    lifter = lib.int_arg('check_options', 'sharpen_lifter (--sharpen-lifter)', sharpen_lifter, lib.SHARPEN_FIRST, lib.PITCH_MAX_LIFTER)
    if not vocode:
        raise ValueError('sharpen (--sharpen) filters the magnitudes in front of Griffin-Lim: it needs vocode')
    return None if beta == 0.0 else (beta, lifter)


def formant_options(formant=None, formant_lifter=FORMANT_LIFTER, vocode=True):
    """--formant SEMITONES / --formant-lifter Q -> None for no shift (SEMITONES None or 0: every file is what it was), else
    (step_q, lifter): lib.formant_step of the semitones, the lifter checked against lib.frames_formant's range at the 1025 bins of
    the model; ValueError"""
    if formant is None:
        return None
    if isinstance(formant, bool):
        raise ValueError('formant (--formant) must be a number of semitones in [-12, 12], got %r' % (formant,))
    step = lib.formant_step(formant)
    lifter = lib.int_arg('check_options', 'formant_lifter (--formant-lifter)', formant_lifter, 1, lib.PITCH_MAX_LIFTER)
    if not vocode:
        raise ValueError('formant (--formant) shifts the envelope of the magnitudes in front of Griffin-Lim: it needs vocode')
    return None if float(formant) == 0.0 else (step, lifter)


def pitch_range_options(pitch_range=None, smooth=lib.F0_RANGE_SMOOTH, limit=lib.F0_RANGE_LIMIT, vocode=True):
    """--pitch-range K / --pitch-range-smooth W / --pitch-range-limit OCT -> None for the model's own intonation (K None or 1: every
    file is what it was), else (scale_q, W, OCT): lib.range_scale of the factor, the two UNTUNED settings checked against
    lib.f0_range_curve's ranges; ValueError"""
    if pitch_range is None:
        return None
    try:
        scale_q = lib.range_scale(pitch_range)
    except ValueError:
        raise ValueError('pitch_range (--pitch-range) must be a factor in [0, 4], got %r' % (pitch_range,)) from None
    smooth = lib.int_arg('check_options', 'pitch_range_smooth (--pitch-range-smooth)', smooth, 0, lib.F0_RANGE_MAX_SMOOTH)
    limit = lib.float_arg('check_options', 'pitch_range_limit (--pitch-range-limit)', limit, 0.0, 1.0)
    if limit == 0.0:
        raise ValueError('check_options: pitch_range_limit (--pitch-range-limit) must be a number of octaves in (0, 1], got %r' % (limit,))
    if not vocode:
        raise ValueError('pitch_range (--pitch-range) scales the pitch contour of the magnitudes in front of Griffin-Lim: it needs vocode')
    return None if float(pitch_range) == 1.0 else (scale_q, smooth, limit)


def check_options(*, n_iter=50, vocode=True, stop=None, vocode_lengths=False, gl_momentum=None, deemphasis=None, trim_db=None, long=None,
                  align_scores=False, rate=None, pitch=None, lifter=32, f0=None, timings=False, f0_smooth=None, prosody=None, gl_init=None,
                  loudness=None, peak_db=None, limit=False, limit_ms=None, true_peak=None, limit_passes=None, path_jump=None):
    """Options.check() for keywords (`path_jump`: None without --timings; given, it is held to its range); ValueError."""
    Options(**dict(locals(), timings=timings or path_jump is not None)).check()


def limit_options(limit_ms=None, true_peak=None, limit_passes=None):
    """the limiter's keywords of level_waveform from the options (None: the default), checked; ValueError"""
    opt = dict(lookahead_ms=LIMIT_MS if limit_ms is None else limit_ms, oversample=lib.LIMIT_P if true_peak is None else true_peak,
               passes=LIMIT_PASSES if limit_passes is None else limit_passes)
    limit_settings('limit (--limit-ms, --true-peak, --limit-passes)', sr=SR, **opt)
    return dict(limit=True, **opt)


def write_prompt(out_dir, n, r, spec, align, wav=None, len_b=None, pcm=None, trim=None, conv=None, piece=None, ascore=None, zoom=4,
                 rate=None, pitch=None, f0=None, dur=None, prosody=None, loud=None, sharpen=None, formant=None, pitch_range=None):
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
    prompt's limit_row, whose first 8 values are written as _limit.npy instead.
    sharpen (--sharpen): (beta, lifter) of the post-filter, written as _sharpen.npy (float64); nothing else depends on it.
    formant (--formant): (step_q, lifter) of the formant shift, written as _formant.npy (int32); nothing else depends on it.
    pitch_range (--pitch-range): (scale_q, smooth, limit, voiced frames, centre, deviation in front), written as _range.npy (float64);
    nothing else depends on it."""
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
    if sharpen is not None:
        np.save(path + '_sharpen.npy', np.asarray(sharpen, dtype=np.float64))
    if formant is not None:
        np.save(path + '_formant.npy', np.asarray(formant, dtype=np.int32))
    if pitch_range is not None:
        np.save(path + '_range.npy', np.asarray(pitch_range, dtype=np.float64))
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
    (vocode(rate=...)): over the row's own len_b r frames with `stop` (whether or not `vocode_lengths` is set; the phases
    are then drawn on the device), else over all frames.  prompt_NNN.wav holds 300 (Fo_b - 1) samples, Fo_b = lib.stretch_frames of
    those frames -- cut on the host by that formula, or with finishing on the device from the stretch's own frames_out -- and
    prompt_NNN_rate.npy (step_q, Fo_b) as int32.  Every other file is the model's own output, unstretched; without `rate` every file
    is what it was.
    `pitch` (needs `vocode`) / `lifter`: None, a pitch shift in semitones in [-12, 12] (0: the model's own) or a sequence with one per
    prompt; with `long`, a prompt's pieces inherit its pitch.  The harmonics of every magnitude frame the vocoder is given are moved
    under the frame's own envelope of `lifter` quefrencies (vocode(pitch=...), in front of the stretch of `rate`): over the
    row's own len_b r frames wherever the vocoder gets the lengths, else over all frames.  prompt_NNN_pitch.npy holds (step_q, lifter)
    as int32; no file changes its size, the model's own files stay what they are, and pitch 0 gives the audio of pitch None.
    `f0` (needs `vocode`): None, True (60 .. 400 Hz) or (lo, hi) in Hz: vocode(f0=...) tracks the pitch of the frames on the
    device, over the row's own len_b r frames with `stop`; prompt_NNN_f0.npy holds (period, strength) of the frames the vocoder was
    given, and f0_lines() prints what `pitch` or `rate` did to it.  Untuned, and meaningless on an untrained model; nothing else
    changes.
    `f0_smooth` (needs `f0`): None, True (lib.F0_CANDIDATES candidates per frame) or their number in 1 .. 15: the tracks are smoothed
    across frames on the device (vocode(f0={'smooth': ...}), lib.f0_viterbi with lib.f0_viterbi_tables' UNTUNED bias and
    costs for the range of `f0`); _f0.npy and f0_lines() use the smoothed track and the line names the frames the smoothing moved.
    `timings` / `path_jump`: every batch's best monotone attention paths are found on the device (Tacotron.alignment_path with
    max_jump = path_jump: over model.lengths with `stop`, else all steps); each prompt -- with `long`, each piece -- additionally
    writes _dur.npy, each prompt _words.tsv (alignment.word_times of the file it wrote) and one line, a WARNING when the path ends
    before the text does.  Nothing else changes.
    `prosody` (needs `stop` and `vocode`, excludes `long`): None, or the rows of parse_prosody -- (prompt, word, rate | None,
    semitones | None) -- rate and pitch per word; words not listed take `rate` / `pitch`, or stay neutral.  Per batch, all on the
    device: the path (Tacotron.alignment_path, max_jump = path_jump), two lib.path_curve gathers of the per-character dur_q / step_q
    into per-frame curves, then vocode(rate_curve=..., pitch_curve=...) over each row's own len_b r frames (the pitch curve
    only when a pitch is asked for anywhere).  prompt_NNN.wav holds 300 (Fo_b - 1) samples, Fo_b the stretch's frames_out (with finishing
    the row ends there on the device); prompt_NNN_prosody.npy the per-character (dur_q, step_q); _rate.npy / _pitch.npy are not written.
    With `timings` the word rows go through the stretch's time map (alignment.word_times(src=...)); with `f0` the line is the drift
    line without a figure asked for.
    `gl_init` (needs `vocode` for 'estimate'): None or 'random' -- every file is what it was -- or 'estimate': Griffin-Lim starts from
    phases read off the magnitudes it is handed (vocode(phase_init='estimate'), lib.phase_estimate), on whichever path the
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
    never reached.
    `config.sharpen` / `config.sharpen_lifter` (need `vocode`; Config's defaults: None, 32): None or 0 -- every file is what it was -- or
    a beta in [-1, 1]: the magnitudes of every row go through the cepstral post-filter first (vocode(sharpen=...), lib.frames_sharpen),
    in front of `pitch`, `rate`, `prosody` and `f0`, over the row's own len_b r frames wherever the vocoder gets the lengths, else over
    all frames; with `long`, every piece.  prompt_NNN_sharpen.npy holds (beta, lifter) as float64.  Untuned; nobody has listened.
    `config.formant` / `config.formant_lifter` (need `vocode`; Config's defaults: None, 32): None or 0 -- every file is what it was --
    or semitones in [-12, 12]: behind the post-filter and in front of `pitch`, `prosody`'s curves and `rate`, the envelope of every
    frame is moved under its harmonics (vocode(formant=...), lib.frames_formant), over the frames `sharpen` runs over; with `long`,
    every piece.  prompt_NNN_formant.npy holds (step_q, lifter) as int32, and with `f0` formant_line() is printed per prompt.
    Untuned; nobody has listened.
    `config.use_ema` (--ema; needs `checkpoint`; Config's default: False): decode from the checkpoint's AVERAGED weights (train --ema,
    Tacotron.load_state_dict(use_ema=True)) instead of the live ones; lib.TacoError before the first batch when the checkpoint holds
    none.  Like the sharpening pair it travels on the Config, not in the options record: it chooses the weights, and everything
    downstream is unchanged."""
    opt = Options(**{k: v for k, v in locals().items() if k in Options.__dataclass_fields__}).resolved(   # (locals(): the parameters)
        getattr(config, 'sharpen', None), getattr(config, 'sharpen_lifter', lib.SHARPEN_LIFTER), getattr(config, 'formant', None),
        getattr(config, 'formant_lifter', FORMANT_LIFTER), getattr(config, 'pitch_range', None),
        getattr(config, 'pitch_range_smooth', lib.F0_RANGE_SMOOTH), getattr(config, 'pitch_range_limit', lib.F0_RANGE_LIMIT))
    run = Run(config, opt, prompts, out_dir, checkpoint, speaker, bool(getattr(config, 'use_ema', False)))
    n = _test_long(run) if opt.long is not None else _test_rows(run, prompts)
    print('wrote %d samples to %s' % (n, out_dir))
    return n


class Batch(collections.namedtuple('Batch', 'spec al wav conv pcm trim lengths scores f0res paths curved louds ranged')):
    """What Run.synthesise returns for one batch: host arrays with one row per prompt, or None.  wav: the float waveform when it was
    not finished on the device, else pcm and trim: the device's int16 samples and [s, e].  lengths (`stop`): len_b.  louds (`loudness`
    without `long`): the loud_rows (B, 8), with `limit` the limit_rows; pcm then is the levelled one.  scores (`align_scores`): (B, 8).
    f0res (`f0`): (track (B, Fv, 2), model_stats, vocoder_stats, pitch_stats | None, and with `f0_smooth` the vocoder track's
    lib.f0_viterbi counts (B, 4); with a formant shift a sixth place behind them -- the fifth None without `f0_smooth` -- holds
    'formant_stats' (B, 3)).  paths (`timings`): (dur (B, Tt), counts (B, 3), mass (B)) of the best monotone paths.  curved
    (`prosody`): (frames_out (B), src (B, Fo)) of the stretch curve.  ranged (a pitch range): (the lib.f0_range_curve stats (B, 3) of the
    track in front of the stage, and with `f0` vocode's 'range_stats' (B, 4), else None)."""

    def row(self, i):
        """the same fields for row i of the batch alone: row i of every array, inside the tuples too"""
        def at(a):
            if a is None:
                return None
            return tuple(at(x) for x in a) if isinstance(a, tuple) else a[i]
        return Batch(*(at(a) for a in self))


class Run:
    """What one call of test() holds across its batches: the configuration, the resolved options and the vocabulary, the checkpoint,
    the parameter buffer and ONE Tacotron per batch size, the F0 tables on the device, the `prosody` table, and per ROW -- a prompt,
    with `long` a piece of one, which inherits its prompt's rate and pitch -- the line, its name in printed lines and its step_q
    values, all resolved before the first batch."""

    def __init__(self, config, opt, prompts, out_dir, checkpoint=None, speaker=0, use_ema=False):
        steps, pitch = rate_steps(opt.rate, len(prompts)), pitch_steps(opt.pitch, len(prompts))
        self.config, self.opt, self.out_dir, self.speaker = config, opt, out_dir, speaker
        meta_path = os.path.join(config.data_path, 'meta.pkl')
        if os.path.exists(meta_path):
            with open(meta_path, 'rb') as f:
                self.ivocab = pkl.load(f)['vocab']
        else:
            self.ivocab = {i + 1: ch for i, ch in enumerate("abcdefghijklmnopqrstuvwxyz '.,?!-")}
            self.ivocab[0] = '<pad>'
        config.vocab_size = len(self.ivocab)
        self.ckpt = torch.load(checkpoint) if checkpoint else None
        self.use_ema = bool(use_ema)
        if self.use_ema and (self.ckpt is None or 'ema' not in self.ckpt):   # (before anything is built or written)
            raise lib.TacoError('use_ema (--ema): %s' % ('there is no checkpoint to take averaged weights from' if self.ckpt is None else
                                                         'the checkpoint %s holds no averaged weights (written without `train --ema`, or '
                                                         'imported): its keys are %s' % (checkpoint, ', '.join(sorted(map(str, self.ckpt))))))
        if self.ckpt is not None:
            config.r, config.vocab_size = self.ckpt.get('shape', (config.r, config.vocab_size))
            config.num_speakers = int(self.ckpt.get('num_speakers', 1))
        self.F = (config.max_decode_iter // 4) * 4 * config.r   # frames per row of the model's output
        self.pros = None   # per prompt: (L, 2) int32 (dur_q, step_q) per encoded character
        if opt.prosody is not None:   # the curves carry --rate and --pitch as the value of every character no row of the table names
            self.pros = prosody_table(opt.prosody, prompts, self.ivocab, _steps('rate', opt.rate, lib.stretch_dur, len(prompts)), pitch)
            self.pros_pitch = pitch is not None or any(sem is not None for _, _, _, sem in opt.prosody)
            self.pros_max = max([lib.STRETCH_ONE] + [int(t[:, 0].max()) for t in self.pros if len(t)])
            steps = pitch = None
        self.params = None
        self.models = {}     # batch size -> Tacotron
        self.f0_opt = None   # the tables on the device, made at the first batch
        os.makedirs(out_dir, exist_ok=True)
        self.pieces = [split_prompt(p) if opt.long is not None else [(p, None)] for p in prompts]   # per prompt: its (line, kind of cut)
        owner = [p for p, pieces in enumerate(self.pieces) for _ in pieces]
        self.lines = [line for pieces in self.pieces for line, _ in pieces]
        self.who = ['prompt %d' % p if len(pieces) == 1 else 'prompt %d piece %d' % (p, k)
                    for p, pieces in enumerate(self.pieces) for k in range(len(pieces))]
        self.row_steps = None if steps is None else [steps[p] for p in owner]
        self.row_pitch = None if pitch is None else [pitch[p] for p in owner]
        self.L = 300 * (self.F - 1)   # `long`: samples per row of the joined buffer; with a rate, every row holds the slowest one's
        if opt.long is not None and steps is not None:
            self.L = 300 * (max(5, lib.stretch_capacity(self.F, min(self.row_steps, default=lib.STRETCH_ONE))) - 1)

    def model_for(self, batch):
        """the Tacotron for this batch's size with the batch as its inputs; only a smaller final batch builds a second one"""
        c, Bn = self.config, batch['text'].shape[0]
        if c.num_speakers > 1:
            batch['speaker'] = torch.full((Bn,), int(self.speaker), dtype=torch.int32)
        if self.params is None:
            shape = lib.make_shape(Bn, batch['text'].shape[1], c.max_decode_iter, c.r, c.vocab_size, c.num_speakers)
            self.params = ParamBuffer(shape, 'cuda').init_(0)
        model = self.models.get(Bn)
        if model is None:
            model = self.models[Bn] = Tacotron(c, batch, train=False, params=self.params)
            if self.ckpt is not None:
                model.load_state_dict(self.ckpt, use_ema=True) if self.use_ema else model.load_state_dict(self.ckpt)
        else:
            model.set_inputs(batch)
        return model

    def f0_tables(self):
        """vocode's `f0` keywords for the range of `f0`, and with `f0_smooth` its 'smooth' ones; the tables go up once"""
        o = self.opt
        if self.f0_opt is None:
            w, g, lag_min, lag_max = lib.f0_tables(SR, o.f0[0], o.f0[1])
            self.f0_opt = dict(weight=torch.from_numpy(w).cuda(), gain=torch.from_numpy(g).cuda(), lag_min=lag_min, lag_max=lag_max)
            if o.f0_smooth is not None:
                bias, lg, jump, switch = lib.f0_viterbi_tables(SR, o.f0[0], o.f0[1])
                self.f0_opt['smooth'] = dict(bias=torch.from_numpy(bias).cuda(), lg=torch.from_numpy(lg).cuda(), candidates=o.f0_smooth,
                                             jump_cost=jump, switch_cost=switch)
        return self.f0_opt

    def curves(self, path, batch, n):
        """vocode's rate_curve / pitch_curve for a batch whose first row is prompt n (`prosody`): two gathers of the per-character
        values along the device's path (the pitch curve only when a pitch is asked for anywhere)"""
        Bn, Tt = batch['text'].shape
        Fm = (path.shape[1] // 4) * 4 * self.config.r
        values = np.empty((2, Bn, Tt), dtype=np.int32)
        values[0], values[1] = lib.STRETCH_ONE, lib.PITCH_ONE
        for i in range(Bn):
            table = self.pros[n + i][:Tt]
            values[:, i, :len(table)] = table.T
        values = torch.from_numpy(values).cuda()
        curves = [lib.path_curve(path, values[k], self.config.r, one)[:, :Fm].contiguous()
                  for k, one in ((0, lib.STRETCH_ONE), (1, lib.PITCH_ONE)) if k == 0 or self.pros_pitch]
        return dict(rate_curve=curves[0], pitch_curve=curves[1] if self.pros_pitch else None)

    def synthesise(self, batch, n, out_rows=None, bounds_rows=None):
        """one batch whose first row has index n -> its Batch.  out_rows / bounds_rows (`long`): the finished fp32 samples and their
        bounds go to these device rows, no PCM16 is made and nothing is levelled (`long` levels the joined prompts instead)"""
        o, c = self.opt, self.config
        rows = slice(n, n + batch['text'].shape[0])
        model = self.model_for(batch)
        out, al = model.run(stop=o.stop)
        lengths = model.lengths if o.stop is not None else None
        scores = model.alignment_scores() if o.align_scores else None   # (enqueued behind the decode; read with the other results below)
        found = model.alignment_path(o.path_jump) if o.timings or self.pros is not None else None   # (likewise; the path stays on the device)
        paths = found[1:] if o.timings else None
        model.check()
        mean, std = (torch.as_tensor(s if s is not None else neutral(c.fft_size * c.r), dtype=torch.float32).cuda()
                     for s, neutral in ((model.stft_mean, torch.zeros), (model.stft_std, torch.ones)))
        spec = lib.denorm_unframe(out, mean, std, c.r)                       # (B, Td*r, 1025) chronological log-magnitudes
        wav = conv = pcm = trim = f0res = curved = louds = ranged = None
        if o.vocode:
            # the vocoder runs over the rows' own frames with `vocode_lengths`, and with a rate or curves whenever there is a rule: the
            # host's Fo_b and the device's frames_out are then one number
            kw = dict(lengths=lengths if o.vocode_lengths or self.row_steps is not None or self.pros is not None else None)
            if self.row_steps is not None:
                kw['rate'] = [q / 65536.0 for q in self.row_steps[rows]]
            if self.row_pitch is not None:   # (step_q as the device takes it: no way back through semitones)
                kw['pitch'] = torch.tensor(self.row_pitch[rows], dtype=torch.int32).cuda()
            if o.f0 is not None:
                kw['f0'] = dict(self.f0_tables(), lengths=lengths)
            if self.pros is not None:
                kw.update(self.curves(found[0], batch, n), dur_q_max=self.pros_max)
            if o.sharpen is not None:
                kw.update(sharpen=o.sharpen[0], sharpen_lifter=o.sharpen[1])
            if o.formant is not None:   # (step_q as the device takes it, one value for every row)
                kw.update(formant=torch.full((batch['text'].shape[0],), o.formant[0], dtype=torch.int32).cuda(), formant_lifter=o.formant[1])
            if o.pitch_range is not None:   # (scale_q as the device takes it, one value for every row; every row, piece or prompt, its own centre)
                Bn = batch['text'].shape[0]
                kw.update(intonation=torch.full((Bn,), o.pitch_range[0], dtype=torch.int32).cuda(), intonation_smooth=o.pitch_range[1],
                          intonation_limit=o.pitch_range[2], intonation_stats=torch.empty(Bn, 3, dtype=torch.float32, device='cuda'))
            v = vocode(out, mean, std, c.r, n_iter=o.n_iter, seed=n, momentum=o.gl_momentum, want_conv=o.gl_momentum is not None,
                       phase_init=o.gl_init, lifter=o.lifter, **kw)
            if v.tracks is not None:
                f0res = (torch.stack(v.tracks['vocoder'], dim=2).cpu().numpy(), v.tracks['model_stats'].cpu().numpy(),
                         v.tracks['vocoder_stats'].cpu().numpy(), v.tracks['pitch_stats'].cpu().numpy() if 'pitch_stats' in v.tracks else None)
                if o.f0_smooth is not None:
                    f0res += (v.tracks['vocoder_counts'].cpu().numpy(),)
                if 'formant_stats' in v.tracks:   # (the sixth place, whether or not the fifth is taken)
                    f0res = f0res[:5] + (None,) * (5 - len(f0res)) + (v.tracks['formant_stats'].cpu().numpy(),)
            if o.pitch_range is not None:
                ranged = (kw['intonation_stats'].cpu().numpy(), v.tracks['range_stats'].cpu().numpy() if v.tracks is not None else None)
            if v.src is not None:
                curved = (v.frames_out.cpu().numpy(), v.src.cpu().numpy())
            wav = v.waveform
            if v.conv is not None:
                conv = v.conv.cpu().numpy()
                print('Griffin-Lim momentum %g, %d rounds: worst final spectral convergence of the batch %.4f'
                      % (o.gl_momentum, o.n_iter, float(conv[:, -1].max())))
            if o.finish:   # (the fp32 waveform stays on the device)
                level_rows = o.level is not None and out_rows is None
                # a rate or curves: the row ends where the stretch says, and the rows of `long` are wider than this batch's
                counts, unit, into = (lengths, c.r, out_rows) if v.frames_out is None else (v.frames_out, 1, None)
                fin, pcm, trim, _ = finish_waveform(wav, counts, unit, deemphasis=0.0 if o.deemphasis is None else o.deemphasis,
                                                    trim_top_db=0.0 if o.trim_db is None else o.trim_db,
                                                    want_out=out_rows is not None or level_rows,
                                                    want_pcm=out_rows is None and not level_rows, out=into, bounds=bounds_rows)
                if out_rows is not None and into is None:
                    out_rows[:, :fin.shape[1]].copy_(fin)
                if level_rows:   # (the finished fp32 rows stay on the device; their PCM16 is the levelled one)
                    pcm, louds = level_finished(fin, o.level, bounds=trim)
                pcm, trim, wav = None if pcm is None else pcm.cpu().numpy(), trim.cpu().numpy(), None
            else:
                wav = wav.cpu().numpy()
        if scores is not None:
            scores = np.stack([scores_row(k, m) for k, m in zip(scores[0].cpu().numpy(), scores[1].cpu().numpy())])
        if paths is not None:
            paths = tuple(x.cpu().numpy() for x in paths)
        return Batch(spec.cpu().numpy(), al.cpu().numpy(), wav, conv, pcm, trim, None if lengths is None else lengths.cpu().numpy(), scores,
                     f0res, paths, curved, louds, ranged)

    def marks(self, score, L):
        """the flags of one row's 8 scores, against the stop rule's own target when there is a rule"""
        return flags(score[:6], score[6:], L, end_offset=self.opt.stop.end_offset if self.opt.stop is not None else 1)

    def frames_of(self, row, rec):
        """the frames the vocoder was given for global row `row`, rec its Batch.row: the stretch's own frames_out behind curves, Fo_b
        behind a rate, else the row's own len_b r or all F"""
        if rec.curved is not None:
            return int(rec.curved[0])
        own = self.F if rec.lengths is None else min(int(rec.lengths) * self.config.r, self.F)
        return own if self.row_steps is None else lib.stretch_frames(own, self.row_steps[row])

    def rate_of(self, row, rec):
        """(step_q, Fo_b) of global row `row`, or None without a rate"""
        return None if self.row_steps is None else (self.row_steps[row], self.frames_of(row, rec))

    def pitch_of(self, row):
        """(step_q, lifter) of global row `row`, or None without a pitch"""
        return None if self.row_pitch is None else (self.row_pitch[row], int(self.opt.lifter))

    def range_of(self, row, rec):
        """the _range.npy values of global row `row`, or None without a pitch range; with `f0` prints the row's line"""
        if rec.ranged is None:
            return None
        if rec.ranged[1] is not None:
            print(range_line(self.who[row], (self.opt.pitch_range[0], rec.ranged[1])))
        return tuple(self.opt.pitch_range) + tuple(float(x) for x in rec.ranged[0])

    def f0_of(self, row, rec):
        """the _f0.npy rows of global row `row`, cut to the frames the vocoder was given; prints the row's line"""
        if rec.f0res is None:
            return None
        frames = self.frames_of(row, rec)
        for line in f0_lines(self.who[row], list(rec.f0res[1:5]), None if self.row_pitch is None else self.row_pitch[row],
                             None if self.row_steps is None else self.row_steps[row], rec.curved is not None):
            print(line)
        if len(rec.f0res) > 5:
            print(formant_line(self.who[row], self.opt.formant[0], rec.f0res[5]))
        return rec.f0res[0][:frames]

    def timing_of(self, row, rec, text_len, offset=0):
        """(_dur.npy of global row `row`, its word rows in the file it goes to) with `timings`, else (None, None); prints the row's
        line.  offset: of the piece in a joined file; the row's trim [s, e] is applied when the waveform was finished, and behind
        curves (`prosody`) the word boundaries go through the row's time map"""
        if rec.paths is None:
            return None, None
        dur, counts, mass = rec.paths
        print(path_line(self.who[row], counts, mass, text_len, self.opt.stop.end_offset if self.opt.stop is not None else 1)[0])
        frames = self.frames_of(row, rec)
        words = word_times(self.lines[row], self.ivocab, dur[:text_len], self.config.r, None if self.row_steps is None else self.row_steps[row],
                           rec.trim, offset, 300 * max(0, frames - 1), SR, src=None if rec.curved is None else rec.curved[1][:frames])
        return dur[:text_len], words

    def write_words(self, n, words):
        with open(os.path.join(self.out_dir, 'prompt_%03d_words.tsv' % n), 'w') as f:
            f.write(words_tsv(words))


def _test_rows(run, prompts):
    """test() without `long`: every prompt is a row of a batch and writes its own files"""
    n = 0
    for batch in load_prompts(prompts, run.ivocab):
        res = run.synthesise(batch, n)
        for i in range(batch['text'].shape[0]):
            rec, text_len = res.row(i), int(batch['text_length'][i])
            dur, words = run.timing_of(n, rec, text_len)
            write_prompt(run.out_dir, n, run.config.r, rec.spec, rec.al, rec.wav, None if rec.lengths is None else int(rec.lengths), rec.pcm,
                         rec.trim, rec.conv, ascore=rec.scores, rate=run.rate_of(n, rec), pitch=run.pitch_of(n), f0=run.f0_of(n, rec),
                         dur=dur, prosody=None if rec.curved is None else (run.pros[n], int(rec.curved[0])), loud=rec.louds,
                         sharpen=run.opt.sharpen, formant=run.opt.formant, pitch_range=run.range_of(n, rec))
            if rec.louds is not None:
                print(level_line('prompt %d' % n, rec.louds, run.opt.level))
            if words is not None:
                run.write_words(n, words)
            found = run.marks(rec.scores, text_len) if rec.scores is not None else []
            if found:
                print('WARNING prompt %d: %s' % (n, ', '.join(found)))
            n += 1
    return n


def _test_long(run):
    """the `long` mode of test(): the pieces of the prompts (run.pieces) are the rows; they are synthesised into the rows of one device
    buffer per group, joined, and written.  With `loudness` the joined prompts are levelled."""
    o, split, L = run.opt, run.pieces, run.L
    pause_ms, fade_ms = o.long
    groups, start = [], 0   # [prompt lo, prompt hi): a group ends at the first prompt boundary at which it holds >= JOIN_GROUP pieces
    held = 0
    for p, pieces in enumerate(split):
        held += len(pieces)
        if held >= JOIN_GROUP or p == len(split) - 1:
            groups.append((start, p + 1))
            start, held = p + 1, 0
    row = 0   # index of the next piece over the whole run (the Griffin-Lim seed of its batch, as the prompt index is without `long`)
    for lo, hi in groups:
        kinds = [kind for pieces in split[lo:hi] for _, kind in pieces]
        first = np.concatenate([[0], np.cumsum([len(pieces) for pieces in split[lo:hi]])]).astype(np.int64).tolist()
        N = len(kinds)
        rows = torch.empty(N, L, dtype=torch.float32, device='cuda')
        bounds = torch.empty(N, 2, dtype=torch.int32, device='cuda')
        done = []   # per piece: (its Batch.row, its text length, its f0 rows)
        for batch in load_prompts(run.lines[row:row + N], run.ivocab):
            at, Bn = len(done), batch['text'].shape[0]
            res = run.synthesise(batch, row + at, rows[at:at + Bn], bounds[at:at + Bn])
            for i in range(Bn):
                rec = res.row(i)
                done.append((rec, int(batch['text_length'][i]), run.f0_of(row + at + i, rec)))
        gap = join_gaps(kinds, pause_ms)
        louds = None
        if o.level is None:
            _, pcm, offsets, total, _ = join_waveform(rows, bounds, first, kinds, pause_ms=pause_ms, fade_ms=fade_ms, want_out=False)
        else:   # (the joined fp32 prompts stay on the device; their PCM16 is the levelled one)
            joined, _, offsets, total, _ = join_waveform(rows, bounds, first, kinds, pause_ms=pause_ms, fade_ms=fade_ms, want_pcm=False)
            pcm, louds = level_finished(joined, o.level, total=total)
        pcm, total, offsets = pcm.cpu().numpy(), total.cpu().numpy(), offsets.cpu().numpy()   # (the one copy back of the group)
        for p in range(lo, hi):
            a, b = first[p - lo], first[p - lo + 1]
            path = os.path.join(run.out_dir, 'prompt_%03d' % p)
            found, words = [], []
            for k in range(a, b):
                rec, text_len, f0rows = done[k]
                dur, piece_words = run.timing_of(row + k, rec, text_len, int(offsets[k]))
                if o.timings:
                    words += piece_words
                write_prompt(run.out_dir, p, run.config.r, rec.spec, rec.al, None, int(rec.lengths), None, rec.trim, rec.conv,
                             piece=None if b - a == 1 else k - a, ascore=rec.scores, rate=run.rate_of(row + k, rec), pitch=run.pitch_of(row + k),
                             f0=f0rows, dur=dur, sharpen=o.sharpen, formant=o.formant, pitch_range=run.range_of(row + k, rec))
                names = run.marks(rec.scores, text_len) if rec.scores is not None else []
                if names:
                    found.append(', '.join(names) if b - a == 1 else 'piece %d %s' % (k - a, ', '.join(names)))
            if found:
                print('WARNING prompt %d: %s' % (p, '; '.join(found)))
            write_wav_pcm(path + '.wav', pcm[p - lo, :int(total[p - lo])])
            if louds is not None:
                save_level(path, louds[p - lo])
                print(level_line('prompt %d' % p, louds[p - lo], o.level))
            if o.timings:
                run.write_words(p, words)
            if b - a > 1:
                table = [[int(offsets[k]), min(L, max(0, int(done[k][0].trim[1]) - int(done[k][0].trim[0]))), 0 if k == b - 1 else gap[k],
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


def option_keywords(a):
    """The namespace of parse_args -> test()'s option keywords: every field of Options under its own name, but `n_iter` (--gl-iters),
    `stop` (the rule of --stop, --end-offset, --hold and --min-steps, or None) and `vocode`, which has no flag"""
    kw = {k: getattr(a, k) for k in Options.__dataclass_fields__ if k not in ('n_iter', 'stop', 'vocode')}
    return dict(kw, n_iter=a.gl_iters, stop=lib.TacoStopRule(a.end_offset, a.hold, a.min_steps) if a.stop else None)


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
    ap.add_argument('--sharpen', type=float, default=None, metavar='BETA',
                    help='spectral sharpening, -1 <= BETA <= 1: a cepstral post-filter on the device in front of every other stage scales '
                         'the quefrencies 2 .. Q of every magnitude frame by 1 + BETA at unchanged frame energy, against the over-smoothed '
                         'envelopes of an L1-trained model; 0 is a run without the flag; writes prompt_NNN_sharpen.npy (untuned; nobody has '
                         'listened; not in the reference)')
    ap.add_argument('--sharpen-lifter', type=int, default=None, metavar='Q',
                    help='--sharpen: the highest quefrency scaled, 2 <= Q <= 64 (default %d, untuned)' % lib.SHARPEN_LIFTER)
    ap.add_argument('--formant', type=float, default=None, metavar='SEMITONES',
                    help='timbre, -12 <= SEMITONES <= 12: behind --sharpen and in front of --pitch and --rate the envelope of every magnitude '
                         'frame is moved along the bin axis on the device (+: formants up) under the unmoved harmonics at unchanged frame '
                         'energy; 0 is a run without the flag; writes prompt_NNN_formant.npy, and with --f0 prints how far the pitch moved '
                         '(untuned; nobody has listened; not in the reference)')
    ap.add_argument('--formant-lifter', type=int, default=None, metavar='Q',
                    help='--formant: the quefrencies 0 .. Q make the envelope, 1 <= Q <= 64 (default %d, untuned)' % FORMANT_LIFTER)
    ap.add_argument('--pitch-range', type=float, default=None, metavar='K',
                    help='intonation range, 0 <= K <= 4: where --pitch sits the pitch contour of the frames is tracked on the device and '
                         'every frame\'s distance from the utterance\'s own level is multiplied by K (0 flat, 1.5 half as wide again), composed '
                         'with --pitch / --prosody; 1 is a run without the flag; writes prompt_NNN_range.npy, and with --f0 prints the range '
                         'asked for and the range measured (K and its two settings are untuned; nobody has listened; on an untrained model '
                         'the frames have no pitch and the numbers mean nothing; not in the reference)')
    ap.add_argument('--pitch-range-smooth', type=int, default=None, metavar='W',
                    help='--pitch-range: the contour is smoothed by a triangle of half-width W frames, 0 <= W <= 8 (default %d, untuned)'
                         % lib.F0_RANGE_SMOOTH)
    ap.add_argument('--pitch-range-limit', type=float, default=None, metavar='OCT',
                    help='--pitch-range: the most one frame\'s excursion may change, 0 < OCT <= 1 octaves (default %g, untuned)'
                         % lib.F0_RANGE_LIMIT)
    ap.add_argument('--ema', action='store_true',
                    help='decode from the averaged weights of a checkpoint written by `train --ema DECAY` instead of the live ones; an '
                         'error when the checkpoint holds none (not in the reference; nobody has listened to the difference)')
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
    if a.sharpen_lifter is not None and a.sharpen is None:
        ap.error('--sharpen-lifter needs --sharpen')
    if a.ema and a.checkpoint is None:
        ap.error('--ema needs --checkpoint: the averaged weights come from a checkpoint of `train --ema`')
    a.sharpen_lifter = lib.SHARPEN_LIFTER if a.sharpen_lifter is None else a.sharpen_lifter
    if a.formant_lifter is not None and a.formant is None:
        ap.error('--formant-lifter needs --formant')
    a.formant_lifter = FORMANT_LIFTER if a.formant_lifter is None else a.formant_lifter
    if (a.pitch_range_smooth is not None or a.pitch_range_limit is not None) and a.pitch_range is None:
        ap.error('--pitch-range-smooth and --pitch-range-limit need --pitch-range')
    a.pitch_range_smooth = lib.F0_RANGE_SMOOTH if a.pitch_range_smooth is None else a.pitch_range_smooth
    a.pitch_range_limit = lib.F0_RANGE_LIMIT if a.pitch_range_limit is None else a.pitch_range_limit
    try:
        Options(**option_keywords(a)).resolved(a.sharpen, a.sharpen_lifter, a.formant, a.formant_lifter, a.pitch_range,
                                               a.pitch_range_smooth, a.pitch_range_limit)
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
    c.sharpen, c.sharpen_lifter = a.sharpen, a.sharpen_lifter
    c.formant, c.formant_lifter = a.formant, a.formant_lifter
    c.pitch_range, c.pitch_range_smooth, c.pitch_range_limit = a.pitch_range, a.pitch_range_smooth, a.pitch_range_limit
    c.use_ema = a.ema
    print('Building Tacotron')
    test(c, prompts, out_dir=a.out_dir, checkpoint=a.checkpoint, speaker=a.speaker, **option_keywords(a))
