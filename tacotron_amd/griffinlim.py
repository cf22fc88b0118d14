"""Vocoder boundary of the reference (audio.invert_spectrogram / audio.griffinlim, audio.py:69-97; test.py:64) on the GPU.

`invert_spectrogram(out, stft_mean, stft_std, r)` takes what `Tacotron.run()` returns -- (B, Td, 1025 r) normalised
log-magnitude frames in the r-frame layout -- and returns waveforms (B, 300 (F - 1)), F = (Td // 4) * 4 * r:
de-normalise + inverse r-frame layout + exp + transpose in ONE HIP gather (taco_denorm_unframe), then Griffin-Lim
(taco_griffinlim: hand-written 2048-point FFT, 50 rounds like the reference).  The reference draws the initial phase with
np.random.rand; here it comes from a seeded torch generator so that a run can be reproduced.  `vocode(...)` is the same call with
its results by name (a `Vocoded`); `invert_spectrogram` flattens it into the reference-shaped return.

With `lengths` (the per-row decoder steps `Tacotron.run(stop=rule)` leaves on the device) every row is vocoded over its own
len_b r frames (taco_griffinlim_rows): the Griffin-Lim of that prompt alone, zeros behind it, and -- unless the caller gives
phase0 -- initial phases from the library's counter-hash generator: no host random numbers, no upload, nothing read back.

With `momentum` (opt-in) the rounds are those of the fast Griffin-Lim algorithm (taco_griffinlim_fast), and `want_conv` returns the
per-round spectral convergence next to the waveform.

With `rate` (opt-in) the magnitude matrix is resampled along its frame axis before Griffin-Lim (taco_frames_stretch): the utterance gets
slower or faster and Griffin-Lim finds phases for the new length, so the pitch stays where it was.

With `pitch` (opt-in) the harmonics of every magnitude frame are moved along the bin axis under the frame's own spectral envelope before
Griffin-Lim (taco_frames_pitch): the voice gets higher or lower, the formants and the duration stay.

With `rate_curve` / `pitch_curve` (opt-in) the two controls take one value per frame instead of one per row (taco_frames_stretch_curve,
taco_frames_pitch_curve): a word slower, a question raised at its end.  The stretch then also returns its time map `src`.

With `f0` (opt-in) the pitch of the magnitude frames is measured on the device (taco_frames_f0, taco_f0_stats): the frames as de-normalised
and, behind `pitch` / `rate`, the frames the vocoder is handed -- the objective stand-in for listening to those two controls.  With
'smooth' in it every track is smoothed across frames (taco_f0_viterbi) before it is summarised.

With `sharpen` (opt-in) every magnitude frame goes through a cepstral post-filter first (taco_frames_sharpen): the low quefrencies of
its envelope are scaled up at unchanged energy, against the over-smoothed envelopes an L1 loss leaves.

With `formant` (opt-in) the envelope of every magnitude frame is moved along the bin axis under the frame's own unmoved harmonics
(taco_frames_formant), the dual of `pitch`: the voice gets smaller or larger, the pitch and the duration stay.

With `intonation` (opt-in) the pitch contour of the frames in front of the pitch stage is tracked and every frame's distance from the
utterance's own level is scaled (taco_f0_range_curve, then taco_frames_pitch_curve): a wider, narrower or flat intonation around the
same level, against the regression to the mean an L1 loss leaves in the F0 contour.

With `phase_init='estimate'` (opt-in) Griffin-Lim starts from phases read off the magnitudes (taco_phase_estimate: single-pass
spectrogram inversion) instead of random ones; with n_iter = 0 that estimate alone is the waveform -- a draft voice at one synthesis pass.

`finish_waveform(wave, lengths, r)` (opt-in) turns that waveform into finished audio on the device (taco_wave_finish): it undoes the
front end's pre-emphasis, optionally trims silence by the front end's energy rule and emits fp32 samples and PCM16.

`join_waveform(pieces, bounds, first, kinds)` (opt-in) puts the finished pieces of long prompts together on the device (taco_wave_join):
a pause after each piece by the kind of cut that ended it (data.split_prompt), a short linear ramp at every interior edge, one fp32 /
PCM16 row per prompt."""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import lib
from .data import CLAUSE, SENTENCE, WORD

SR = 16000   # test.py:11


def invert_spectrogram(out, stft_mean, stft_std, r, n_iter=50, seed=0, phase0=None, mag_t=None, wave=None, work=None,
                       lengths=None, momentum=None, want_conv=False, rate=None, frames_out=None, pitch=None, lifter=32, f0=None,
                       rate_curve=None, pitch_curve=None, dur_q_max=lib.STRETCH_MAX_STEP, src=None, phase_init=None, sharpen=None,
                       sharpen_lifter=lib.SHARPEN_LIFTER, formant=None, formant_lifter=32, intonation=None,
                       intonation_smooth=lib.F0_RANGE_SMOOTH, intonation_limit=lib.F0_RANGE_LIMIT, intonation_stats=None):
    """mag_t / wave / work: the caller's own buffers for the magnitudes, the waveform and Griffin-Lim's workspace (default: fresh).
    lengths: (B) int32 decoder steps on the device (e.g. model.lengths); work then holds lib.griffinlim_rows_workspace_floats.
    momentum: None for the plain algorithm on the two paths above, or a number in [0, 1) for the fast Griffin-Lim of Perraudin,
    Balazs and Sondergaard (lib.griffinlim_fast; 0.99 is librosa's default), with `lengths` or without; work then holds
    lib.griffinlim_fast_workspace_floats.  Without phase0 the phases of that path ALWAYS come from the device's counter-hash
    generator (seeded by `seed`; no host draw, no upload) -- not the torch-generator phases of the momentum=None path without
    lengths, so the same seed gives another waveform there.
    want_conv (needs momentum): returns (waveform, conv (B, n_iter + 1)), the spectral convergence in front of every round and of
    the waveform returned (include/taco_hip.h).
    rate: None for the model's own speaking rate on the paths above, untouched.  Otherwise a number in [0.25, 4] (1.0: the model's rate,
    0.8 slower, 1.25 faster), a host sequence of B such numbers, or a (B) int32 device tensor of step_q values (lib.stretch_step): the
    first len_b r frames of every row (all F frames without `lengths`) are resampled by lib.frames_stretch into (B, 1025, Fo), Fo the
    capacity at the slowest rate of the batch (a device tensor: at rate 0.25) and at least the 5 frames Griffin-Lim needs, and the
    stretched matrix is vocoded over the device's frames_out with frames_per_unit = 1.  With a rate the vocoder ALWAYS takes the
    per-row entry points (lib.griffinlim_rows, or lib.griffinlim_fast with `momentum`), so without phase0 the phases come from the
    device's counter-hash generator over (B, 1025, Fo) -- not the torch-generator phases of the rate=None path without lengths.
    Returns what the call returns without a rate, over Fo frames -- the waveform (B, 300 (Fo - 1)), or (waveform, conv) -- followed
    by frames_out (B) int32 on the device: (waveform, frames_out) or (waveform, conv, frames_out).  wave / work / phase0 are then
    sized for Fo frames; frames_out: the caller's own buffer for the stretched frame counts (needs rate).
    pitch: None for the model's own pitch, untouched.  Otherwise a number of semitones in [-12, 12] (0: the model's pitch, which gives
    the bits of None), a host sequence of B such numbers, or a (B) int32 device tensor of step_q values (lib.pitch_step): right after
    the de-normalisation the first len_b r frames of every row (all F frames without `lengths`) go through lib.frames_pitch with
    `lifter` quefrencies of envelope (32: untuned), and the result takes the place of the magnitudes on every path above -- in
    front of the stretch when `rate` is given too.  It changes no phase source and no return shape.
    f0: None: nothing is measured and the path and the return are what they were.  True, or a dict of lib.frames_f0's keywords
    (weight, gain, lag_min, lag_max, ratio, threshold; True: lib.f0_tables() and the UNTUNED ratio 0.9 / threshold 0.3) and optionally
    'lengths', the (B) int32 decoder steps to measure over when the vocoder itself is not given them: the frames are tracked as
    de-normalised, behind `pitch`, and behind `rate`, each over the row's own frames, and the return gains one last element (a bare
    waveform becomes (waveform, tracks)), the dict
      'model' / 'vocoder': (period, strength) (B, F) of the de-normalised frames / of the frames Griffin-Lim was handed (the same
                 tensors without pitch and rate; over Fo frames with a rate), 'pitched': behind `pitch`, in front of the stretch
      'model_stats' / 'vocoder_stats': lib.f0_stats of those periods (B, 3): count, mean and deviation of log2(period)
      'pitch_stats': with `pitch`, the paired lib.f0_stats (B, 3) of 'pitched' against 'model': 12 x its mean is the shift measured
                 in semitones over the frames voiced in both.
      'smooth' in the dict (opt-in): True, or a dict of lib.f0_viterbi's keywords (bias, lg, candidates, threshold, jump_cost,
                 switch_cost; True and whatever is missing: lib.f0_viterbi_lag_tables for the lags tracked, Praat's costs of
                 lib.f0_viterbi_tables() and the pick's threshold -- all UNTUNED).  Every track is then taken with want_acf=True and
                 passed through lib.f0_viterbi: tracks[name] holds the SMOOTHED (period, strength) and every *_stats is taken over
                 those; tracks[name + '_raw'] holds the per-frame pair (the bits of a run without 'smooth') and
                 tracks[name + '_counts'] the (B, 4) int32 counts in the order lib.F0_VITERBI_COUNTS.  The waveform does not change.
    pitch_curve / rate_curve (opt-in): prosody inside an utterance, one value per FRAME -- (B, F) int32 device tensors, F = the frames
    of mag_t, e.g. lib.path_curve of per-character values along lib.alignment_path.  pitch_curve holds step_q values
    (lib.pitch_step) and takes the place of `pitch` (lib.frames_pitch_curve); rate_curve holds dur_q values (lib.stretch_dur: the
    output frames a source frame lasts) and takes the place of `rate` (lib.frames_stretch_curve).  Giving both of a pair is a
    ValueError.  The order is the same: pitch on the unstretched frames, then the stretch.  Fo is
    lib.stretch_curve_capacity(F, dur_q_max), dur_q_max the caller's statement of the slowest duration in rate_curve (default
    262144: rate 0.25), and at least 5; the vocoder takes the per-row entry points over frames_out as with `rate`, and the return
    gains frames_out (B) and src (B, Fo) int32 -- the time map, (i << 16) | wq per output frame, -1 behind Fo_b -- behind the
    waveform: (waveform, frames_out, src) or (waveform, conv, frames_out, src).  frames_out / src: the caller's own buffers.  The
    f0 tracks behave as behind `pitch` / `rate`.  Neutral curves (65536 everywhere) give the bits of pitch=0 / rate=1.0.
    phase_init (opt-in): None or 'random' -- the phase sources described above, bit for bit -- or 'estimate': the initial phases are
    read off the magnitudes the vocoder is handed (lib.phase_estimate, taco_phase_estimate: single-pass spectrogram inversion), behind
    pitch and behind the stretch, over each row's own frames (frames_out with per-unit 1 where there is a rate, like the 'vocoder' F0
    track), and go in as phase0 to the entry point the path takes anyway; `seed` then has no influence.  With n_iter = 0 the
    waveform is the estimate's own: one synthesis pass, a draft voice.  'estimate' together with phase0 is a ValueError.  Return
    shapes do not change.
    sharpen (opt-in): None or 0 -- nothing is touched, bit for bit -- or a beta in [-1, 1]: directly behind the de-normalisation, in
    front of the 'model' F0 track, `pitch` and `rate`, the first len_b r frames of every row (all F frames without `lengths`) go
    through lib.frames_sharpen (taco_frames_sharpen): the quefrencies 2 .. sharpen_lifter of every frame's cepstrum scaled by
    1 + beta at unchanged frame energy, against the over-smoothed envelopes of an L1-trained post-net.  beta and the lifter (32)
    are UNTUNED: nobody has listened.  Return shapes do not change.
    formant (opt-in): None or 0 -- nothing is touched, bit for bit -- or a number of semitones in [-12, 12] (+ moves the formants up:
    a shorter vocal tract), a host sequence of B such numbers, or a (B) int32 device tensor of step_q values (lib.formant_step):
    behind `sharpen` and the 'model' F0 track and in front of `pitch` / `pitch_curve` and the stretch, the first len_b r frames of
    every row (all F frames without `lengths`) go through lib.frames_formant (taco_frames_formant) with formant_lifter quefrencies
    of envelope (32: UNTUNED): the envelope is read at k / ratio under the unmoved harmonics, at unchanged frame energy.  With `f0`
    the frames behind the stage are tracked as 'formant' (with 'formant_raw' / 'formant_counts' under 'smooth'), and
    'formant_stats' is the paired lib.f0_stats (B, 3) of 'formant' against 'model': 1200 x its mean is the drift of the pitch in
    cents, which should be none.  'pitch_stats' then compares 'pitched' with 'formant', the track directly in front of the pitch
    stage.  Nobody has listened.  Return shapes do not change.
    intonation (opt-in): None or a plain 1.0 -- nothing is touched, bit for bit -- or the factor k in [0, 4] by which every frame's
    distance from the row's own pitch level is multiplied (0 flat, 0.5 half the range, 1.5 half as wide again), a host sequence of B
    such numbers, or a (B) int32 device tensor of scale_q values (lib.range_scale; clamped on the device, never read here), against
    the flattened intonation of an L1-trained model that 'model_stats' measures.  The stage sits where the pitch stage sits: the
    frames directly in front of it ('formant' if that stage ran, else 'model') are tracked -- with `f0` that track and its settings
    are reused, the Viterbi-smoothed one under 'smooth'; without `f0` they are tracked once with lib.f0_tables() defaults, and the
    return shape does not change -- lib.f0_range_curve (taco_f0_range_curve) turns the track into a per-frame step curve, composed
    with `pitch_curve`, or with `pitch` broadcast to (B, F) on the device, and the curve goes through lib.frames_pitch_curve in place
    of the pitch stage.  intonation_smooth (frames, 0 .. 8) and intonation_limit (octaves, (0, 1]) default to 2 and 0.5: UNTUNED,
    nobody has listened.  With `f0` the frames behind the stage are tracked as 'pitched', as behind `pitch`, and
    tracks['range_stats'] is (B, 4) fp32: the count of 'pitched', the deviation of log2(period) of the track in front, that of
    'pitched', and their ratio (0 where the former is 0) -- the closed-loop reading "asked x1.5, measured x1.47".
    intonation_stats (needs the stage to run): the caller's own (B, 3) fp32 buffer for what lib.f0_range_curve says of the track in
    front -- lib.f0_stats' count, centre and deviation over the frames the stage ran on -- also without `f0`.
    Everything stays on the device.  F0 in Hz is SR / period."""
    res = tuple(x for x in vocode(**locals()) if x is not None)   # (the first statement: locals() are the parameters)
    return res[0] if len(res) == 1 else res


class Vocoded(NamedTuple):
    """what vocode() returns: invert_spectrogram's "waveform [, conv] [, frames_out] [, src] [, tracks]" by name; a field is None when
    it was not asked for"""
    waveform: torch.Tensor
    conv: Optional[torch.Tensor] = None
    frames_out: Optional[torch.Tensor] = None
    src: Optional[torch.Tensor] = None
    tracks: Optional[dict] = None


def _f0_tracker(f0, out, r, lengths):
    """`f0` of vocode() -> None, or (track, tracks): track(name, frames_t) measures the frames of one stage into the dict tracks --
    tracks[name], tracks[name + '_stats'], with 'smooth' also name + '_raw' / '_counts', behind 'pitched' the paired 'pitch_stats' --
    over the decoder steps `f0` names, or track('vocoder', stretched, frames_out) over the frames a stretch left.  The stage measured
    last is the vocoder's: its entries are tracks['vocoder' ...] too.  Host tables go up once here, not once per track; ValueError"""
    if f0 is None or f0 is False:
        return None
    opt = {} if f0 is True else dict(f0)
    unknown = set(opt) - {'weight', 'gain', 'lag_min', 'lag_max', 'ratio', 'threshold', 'lengths', 'smooth'}
    if unknown:
        raise ValueError('invert_spectrogram: f0: unknown settings %s' % sorted(unknown))
    smooth = opt.pop('smooth', None)
    smooth = None if smooth is None or smooth is False else {} if smooth is True else dict(smooth)
    unknown = set(smooth or ()) - {'bias', 'lg', 'candidates', 'threshold', 'jump_cost', 'switch_cost'}
    if unknown:
        raise ValueError('invert_spectrogram: f0: smooth: unknown settings %s' % sorted(unknown))
    f0_lengths = opt.pop('lengths', lengths)
    if not {'weight', 'gain', 'lag_min', 'lag_max'} & set(opt):   # (none given: the production tables at this bin count)
        opt['weight'], opt['gain'], opt['lag_min'], opt['lag_max'] = lib.f0_tables(C=out.shape[2] // r)
    if smooth is not None:   # (after the lags are known)
        lags = {k: opt[k] for k in ('lag_min', 'lag_max') if k in opt}
        if 'lg' not in smooth or 'bias' not in smooth:
            bias, lg = lib.f0_viterbi_lag_tables(lags.get('lag_min', 40), lags.get('lag_max', 266))
            smooth.setdefault('bias', bias)
            smooth.setdefault('lg', lg)
        smooth.setdefault('threshold', opt.get('threshold', lib.F0_THRESHOLD))
        smooth.update(lags)
    for d, k in ((opt, 'weight'), (opt, 'gain'), (smooth, 'bias'), (smooth, 'lg')):
        if d and d.get(k) is not None and not (torch.is_tensor(d[k]) and d[k].device == out.device):
            d[k] = torch.as_tensor(np.asarray(d[k], dtype=np.float32)).to(out.device)
    tracks = {}

    def track(name, frames_t, frames_out=None):
        counts, per_unit = (f0_lengths, r if f0_lengths is not None else 1) if frames_out is None else (frames_out, 1)
        if smooth is None:
            tracks[name] = lib.frames_f0(frames_t, counts, per_unit, **opt)
        else:
            period, strength, acf = lib.frames_f0(frames_t, counts, per_unit, want_acf=True, **opt)
            smoothed = lib.f0_viterbi(acf, counts, per_unit, **smooth)
            tracks[name], tracks[name + '_raw'], tracks[name + '_counts'] = smoothed[:2], (period, strength), smoothed[2]
        tracks[name + '_stats'] = lib.f0_stats(tracks[name][0], None, counts, per_unit)
        if name == 'pitched':   # against the track directly in front of the pitch stage
            tracks['pitch_stats'] = lib.f0_stats(tracks['pitched'][0], tracks['formant' if 'formant' in tracks else 'model'][0], counts,
                                                 per_unit)
        for k in ('', '_stats', '_raw', '_counts'):
            if name + k in tracks:
                tracks['vocoder' + k] = tracks[name + k]
        if name == 'formant':   # (behind the loop: 'vocoder_stats' keeps the track's own summary) the paired one takes the name
            tracks['formant_stats'] = lib.f0_stats(tracks['formant'][0], tracks['model'][0], counts, per_unit)

    return track, tracks


def _intonation_scale(intonation, B, dev):
    """`intonation` of vocode() -> None for a run without the stage (None, a plain 1.0), else the scale_q lib.f0_range_curve takes:
    a (B) int32 device tensor passed through, never read, or the lib.range_scale of a number or of B host numbers; ValueError"""
    if intonation is None:
        return None
    if torch.is_tensor(intonation) and intonation.device.type != 'cpu':
        return intonation
    if isinstance(intonation, bool):
        raise ValueError('invert_spectrogram: intonation must be a factor in [0, 4], got %r' % (intonation,))
    if isinstance(intonation, (int, float)) and float(intonation) == 1.0:
        return None
    scale = lib.steps_of(intonation, lib.range_scale, B)
    return torch.tensor(scale if isinstance(scale, list) else [scale] * B, dtype=torch.int32).to(dev)


def vocode(out, stft_mean, stft_std, r, n_iter=50, seed=0, phase0=None, mag_t=None, wave=None, work=None,
           lengths=None, momentum=None, want_conv=False, rate=None, frames_out=None, pitch=None, lifter=32, f0=None,
           rate_curve=None, pitch_curve=None, dur_q_max=lib.STRETCH_MAX_STEP, src=None, phase_init=None, sharpen=None,
           sharpen_lifter=lib.SHARPEN_LIFTER, formant=None, formant_lifter=32, intonation=None,
           intonation_smooth=lib.F0_RANGE_SMOOTH, intonation_limit=lib.F0_RANGE_LIMIT, intonation_stats=None):
    """invert_spectrogram with its result by name: the same parameters, documented there -> Vocoded"""
    if phase_init not in (None, 'random', 'estimate'):
        raise ValueError("invert_spectrogram: phase_init must be None, 'random' or 'estimate', got %r" % (phase_init,))
    if phase_init == 'estimate' and phase0 is not None:
        raise ValueError("invert_spectrogram: phase_init='estimate' excludes phase0: give one of them")
    track, tracks = _f0_tracker(f0, out, r, lengths) or (None, None)
    if pitch is not None and pitch_curve is not None:
        raise ValueError('invert_spectrogram: pitch_curve excludes pitch: give one of them')
    if rate is not None and rate_curve is not None:
        raise ValueError('invert_spectrogram: rate_curve excludes rate: give one of them')
    if frames_out is not None and rate is None and rate_curve is None:
        raise ValueError('invert_spectrogram: frames_out needs rate')
    if src is not None and rate_curve is None:
        raise ValueError('invert_spectrogram: src needs rate_curve')
    if want_conv and momentum is None:
        raise ValueError('invert_spectrogram: want_conv needs momentum (0 for the plain rounds)')
    mean, std = (torch.as_tensor(x, dtype=torch.float32, device=out.device) for x in (stft_mean, stft_std))
    mag_t = lib.denorm_unframe(out.contiguous(), mean, std, r, want_spec=False, want_mag_t=True, mag_t=mag_t)   # (B, 1025, F)
    # (mag_t, counts, per_unit): the frames the next stage is handed -- row b holds counts[b] * per_unit of them, all without counts.
    # taco_griffinlim_fast / _rows are given r as the frames per unit of an unstretched matrix also without counts: gl_unit
    counts, per_unit, gl_unit = lengths, r if lengths is not None else 1, r
    if sharpen is not None and float(sharpen) != 0.0:   # (first: every later stage, the F0 tracks included, sees the sharpened frames)
        mag_t = lib.frames_sharpen(mag_t, sharpen, sharpen_lifter, counts, per_unit)
    if track:
        track('model', mag_t)
    if formant is not None and not (isinstance(formant, (int, float)) and not isinstance(formant, bool) and float(formant) == 0.0):
        mag_t = lib.frames_formant(mag_t, counts, lib.steps_of(formant, lib.formant_step), frames_per_unit=per_unit, lifter=formant_lifter)
        if track:
            track('formant', mag_t)
    ranged = _intonation_scale(intonation, mag_t.shape[0], out.device)
    if intonation_stats is not None and ranged is None:
        raise ValueError('invert_spectrogram: intonation_stats needs intonation')
    if ranged is not None:   # in place of the pitch stage: the contour in front of it, scaled, composed with pitch / pitch_curve
        front = 'formant' if track and 'formant' in tracks else 'model'
        if track:
            period = tracks[front][0]
        else:
            w, g, lag_min, lag_max = lib.f0_tables(C=mag_t.shape[1])
            period = lib.frames_f0(mag_t, counts, per_unit, w, g, lag_min, lag_max)[0]
        base_q = pitch_curve
        if base_q is None and pitch is not None:
            step_q = lib.steps_of(pitch, lib.pitch_step, mag_t.shape[0])
            if not torch.is_tensor(step_q):
                step_q = torch.tensor(step_q if isinstance(step_q, list) else [step_q] * mag_t.shape[0], dtype=torch.int32).to(out.device)
            base_q = step_q.view(-1, 1).expand(-1, mag_t.shape[2]).contiguous()
        curve = lib.f0_range_curve(period, counts, per_unit, ranged, base_q, intonation_smooth, intonation_limit,
                                   out=None if intonation_stats is None else (None, intonation_stats), want_stats=intonation_stats is not None)
        curve = curve[0] if intonation_stats is not None else curve
        mag_t = lib.frames_pitch_curve(mag_t, counts, curve, frames_per_unit=per_unit, lifter=lifter)
    elif pitch_curve is not None:
        mag_t = lib.frames_pitch_curve(mag_t, counts, pitch_curve, frames_per_unit=per_unit, lifter=lifter)
    elif pitch is not None:
        mag_t = lib.frames_pitch(mag_t, counts, lib.steps_of(pitch, lib.pitch_step), frames_per_unit=per_unit, lifter=lifter)
    if track and (pitch is not None or pitch_curve is not None or ranged is not None):
        track('pitched', mag_t)
        if ranged is not None:   # (count of 'pitched', sd in front, sd behind, their ratio) from the two *_stats, on the device
            sd_in, behind = tracks[front + '_stats'][:, 2], tracks['pitched_stats']
            ratio = torch.where(sd_in > 0, behind[:, 2] / sd_in, torch.zeros_like(sd_in))
            tracks['range_stats'] = torch.stack([behind[:, 0], sd_in, behind[:, 2], ratio], dim=1)
    if rate is not None or rate_curve is not None:
        F = mag_t.shape[2]
        if rate_curve is not None:
            Fo = max(5, lib.stretch_curve_capacity(F, lib.int_arg('invert_spectrogram', 'dur_q_max', dur_q_max, lib.STRETCH_MIN_STEP,
                                                                  lib.STRETCH_MAX_STEP)))
            mag_t, frames_out, src = lib.frames_stretch_curve(mag_t, counts, rate_curve, frames_per_unit=per_unit, Fo=Fo,
                                                              frames_out=frames_out, src=src)
        else:
            step_q = lib.steps_of(rate, lib.stretch_step)
            if torch.is_tensor(step_q):   # (on a device, never read: any rate down to the slowest)
                slowest = lib.STRETCH_MIN_STEP
            else:
                slowest = min(step_q, default=lib.STRETCH_ONE) if isinstance(step_q, list) else step_q
            Fo = max(5, lib.stretch_capacity(F, slowest))
            mag_t, frames_out = lib.frames_stretch(mag_t, counts, step_q, frames_per_unit=per_unit, Fo=Fo, frames_out=frames_out)
        counts, per_unit, gl_unit = frames_out, 1, 1   # (the stretched rows hold frames_out frames each, whatever `lengths` was)
        if track:
            track('vocoder', mag_t, frames_out)
    if phase0 is not None:
        phase0 = phase0.contiguous()
    if phase_init == 'estimate':   # (over the frames the vocoder runs on: every row's own with counts, else all of them)
        phase0 = lib.phase_estimate(mag_t, counts, per_unit)
    conv = None
    if momentum is not None:
        waveform = lib.griffinlim_fast(mag_t, counts, phase0=phase0, seed=seed, n_iter=n_iter, momentum=momentum, frames_per_unit=gl_unit,
                                       want_conv=want_conv, out=wave, work=work)
        if want_conv:
            waveform, conv = waveform
    elif counts is not None:
        waveform = lib.griffinlim_rows(mag_t, counts, phase0=phase0, seed=seed, n_iter=n_iter, frames_per_unit=gl_unit, out=wave, work=work)
    else:
        if phase0 is None:
            g = torch.Generator(device='cpu').manual_seed(seed)
            phase0 = (2.0 * math.pi * torch.rand(mag_t.shape, generator=g)).to(out.device)
        waveform = lib.griffinlim(mag_t, phase0, n_iter, out=wave, work=work)
    return Vocoded(waveform, conv, frames_out, src, tracks)


def finish_samples(lengths, r, L):
    """(B) int32 decoder steps -> (B) int32 samples n_b of the rows of a (B, L) waveform, L = 300 (F - 1), by the rule of
    taco_griffinlim_rows: F_b = min(F, lengths * r) frames, n_b = 300 (F_b - 1), and 0 below 5 frames.  Torch ops on the tensor's own
    device; nothing is read back."""
    F = int(L) // 300 + 1
    Fb = torch.clamp(lengths.to(torch.int64) * int(r), max=F)
    return torch.where(Fb < 5, torch.zeros_like(Fb), 300 * (Fb - 1)).to(torch.int32)


def finish_waveform(wave, lengths=None, r=1, deemphasis=0.97, trim_top_db=0.0, want_out=True, want_pcm=True, out=None, pcm=None,
                    bounds=None, peak=None, work=None):
    """wave (B, L) as invert_spectrogram returns it -> (out, pcm, bounds, peak) of lib.wave_finish: de-emphasised (the inverse of the
    front end's pre-emphasis 0.97), trimmed at trim_top_db (0: not trimmed), as fp32 and as PCM16.  lengths: (B) int32 decoder steps
    on the device (model.lengths, with r the reduction factor): row b then ends where its Griffin-Lim ended."""
    if lengths is not None:
        if int(r) < 1:
            raise ValueError('finish_waveform: r must be >= 1, got %r' % (r,))
        if wave.dim() != 2 or tuple(lengths.shape) != (wave.shape[0],) or lengths.dtype != torch.int32:
            raise ValueError('finish_waveform: lengths must be an int32 tensor of shape (B,) for a (B, L) waveform')
    samples = None if lengths is None else finish_samples(lengths, r, wave.shape[1])
    return lib.wave_finish(wave, samples, deemphasis=deemphasis, trim_top_db=trim_top_db, want_out=want_out, want_pcm=want_pcm, out=out,
                           pcm=pcm, bounds=bounds, peak=peak, work=work)


def join_samples(ms, sr=SR):
    """milliseconds -> samples at `sr`, rounded to the nearest sample; ValueError below 0 or NaN"""
    ms = float(ms)
    if not ms >= 0.0 or math.isinf(ms):
        raise ValueError('join_waveform: a duration must be a finite number of milliseconds >= 0, got %r' % (ms,))
    return int(round(ms * sr / 1000.0))


def join_gaps(kinds, pause_ms=(300.0, 150.0, 0.0), sr=SR):
    """the samples of silence behind each piece from the kind of cut that ended it: pause_ms = (SENTENCE, CLAUSE, WORD) milliseconds;
    a HARD cut (inside a word) and the END of a prompt get none"""
    if len(pause_ms) != 3:
        raise ValueError('join_waveform: pause_ms must be (SENTENCE, CLAUSE, WORD) milliseconds, got %r' % (pause_ms,))
    table = {SENTENCE: join_samples(pause_ms[0], sr), CLAUSE: join_samples(pause_ms[1], sr), WORD: join_samples(pause_ms[2], sr)}
    return [table.get(int(k), 0) for k in kinds]


def join_waveform(pieces, bounds, first, kinds, pause_ms=(300.0, 150.0, 0.0), fade_ms=5.0, **kw):
    """pieces (N, L) and bounds (N, 2) as finish_waveform returns them (out, bounds), first (P + 1) host integers, kinds (N) the
    kinds of data.split_prompt -> (out, pcm, offsets, total, peak) of lib.wave_join, with gap = join_gaps(kinds, pause_ms) and a ramp of
    fade_ms milliseconds at every interior edge.  The defaults (300 / 150 / 0 ms pauses, 5 ms ramps) are choices, not tuned by ear.
    Keywords go to lib.wave_join (Lj, want_out, want_pcm and the caller's own buffers)."""
    return lib.wave_join(pieces, bounds, first, join_gaps(kinds, pause_ms), fade=join_samples(fade_ms), **kw)


def limit_settings(who, lookahead_ms=1.5, oversample=4, passes=2, sr=SR):
    """The checked settings of the true-peak limiter -> (W, P, passes): W = round(lookahead_ms sr / 1000) samples of look-ahead,
    clamped into 0 .. lib.LIMIT_MAX_W; P = oversample in 1..8 (1: a sample-peak limiter); passes in 1..8.  ValueError otherwise.
    The defaults (1.5 ms, 4 x, and lib.LIMIT_T = 12 taps at beta 6) are untuned: nobody has listened to a limited file."""
    try:
        lookahead_ms = float(lookahead_ms)
    except (TypeError, ValueError):
        raise ValueError('%s: lookahead_ms must be a number of milliseconds, got %r' % (who, lookahead_ms)) from None
    if not lookahead_ms >= 0.0 or math.isinf(lookahead_ms):
        raise ValueError('%s: lookahead_ms must be a finite number of milliseconds >= 0, got %r' % (who, lookahead_ms))
    P = lib.int_arg(who, 'oversample', oversample, 1, 8)
    passes = lib.int_arg(who, 'passes', passes, 1, 8)
    return min(lib.LIMIT_MAX_W, int(round(lookahead_ms * sr / 1000.0))), P, passes


def level_waveform(fin, bounds=None, total=None, target=-23.0, ceiling_db=-1.0, sr=SR, limit=False, lookahead_ms=1.5, oversample=4,
                   passes=2, **kw):
    """fin (B, L) finished fp32 rows -> (out, pcm, loud, blocks) of lib.wave_loudness: every row measured by ITU-R BS.1770 over its own
    samples and emitted at `target` LUFS (-23: EBU R 128) with its sample peak at or below ceiling_db decibels re full scale (<= 0).
    bounds: (B, 2) int32 on the device as finish_waveform returns them -- row b holds bounds[b, 1] - bounds[b, 0] samples; total: (B)
    int32 on the device as join_waveform returns it -- row b holds total[b]; neither: every row holds L samples.  The counts are
    formed by torch ops on the device; nothing is read back.  target None measures only.  Keywords go to lib.wave_loudness (want_out,
    want_pcm and the caller's own buffers).
    limit=True: the row gets the gain its target asks for and lib.wave_limit holds its TRUE peak at ceiling_db (dBTP) by pulling down
    only the neighbourhood of a peak -> (out, pcm, loud, blocks, peaks, counts): the measured gain G = 10^((target - I) / 20) (1
    where I is not finite) is formed on the device; the rows are limited with it; for each further pass the output is measured, G
    is multiplied by 10^((target - I_out) / 20) and the ORIGINAL rows are limited again; loud and blocks are a last measurement of
    the final out, peaks and counts those of lib.wave_limit.  lookahead_ms, oversample, passes: limit_settings.  Keywords then go to
    lib.wave_limit (want_pcm and the caller's own out, pcm, peaks, counts, work); out is always formed.  Nothing is read back."""
    if not isinstance(limit, bool):
        raise ValueError('level_waveform: limit must be True or False, got %r' % (limit,))
    if limit:
        W, P, passes = limit_settings('level_waveform', lookahead_ms, oversample, passes, sr)
        if target is None:
            raise ValueError('level_waveform: limit=True needs a target')
    if bounds is not None and total is not None:
        raise ValueError('level_waveform: give bounds (of finish_waveform) or total (of join_waveform), not both')
    B = fin.shape[0] if torch.is_tensor(fin) and fin.dim() == 2 else None
    samples = None
    if bounds is not None:
        lib.tensor_arg('level_waveform', 'bounds', bounds, torch.int32, (B, 2), fin.device)
        samples = (bounds[:, 1] - bounds[:, 0]).contiguous()
    elif total is not None:
        lib.tensor_arg('level_waveform', 'total', total, torch.int32, (B,), fin.device)
        samples = total
    ceiling_db = float(ceiling_db)
    if not ceiling_db <= 0.0 or math.isinf(ceiling_db):
        raise ValueError('level_waveform: ceiling_db must be a finite number of decibels <= 0, got %r' % (ceiling_db,))
    if not limit:
        return lib.wave_loudness(fin, samples, sr=sr, target=target, ceiling=10.0 ** (ceiling_db / 20.0), **kw)
    target = float(target)
    if not -70.0 <= target <= 0.0:   # (NaN fails)
        raise ValueError('level_waveform: target must be in [-70, 0] LUFS, got %r' % (target,))
    if kw.get('want_out', True) is False:
        raise ValueError('level_waveform: limit=True always forms out (the passes measure it)')
    kw = dict(kw, want_out=True)
    kw.setdefault('want_pcm', True)
    taps = lib.true_peak_taps(P, lib.LIMIT_T, lib.LIMIT_BETA) if P > 1 else np.zeros((0, lib.LIMIT_T), np.float32)
    loud = lib.wave_loudness(fin, samples, sr=sr, target=None)[2]   # (refuses what is no (B, L) fp32 tensor on the GPU)
    taps, window = torch.from_numpy(taps).to(fin.device), torch.from_numpy(lib.limit_window(W)).to(fin.device)

    def towards(I):   # the factor that carries a row read at I LUFS to the target; 1 where there is no reading
        return torch.where(torch.isfinite(I), torch.pow(10.0, (target - I) / 20.0), torch.ones_like(I))

    G = towards(loud[:, 0]).contiguous()
    for k in range(passes):
        out, pcm, peaks, counts = lib.wave_limit(fin, samples, gain=G, ceiling=10.0 ** (ceiling_db / 20.0), taps=taps, window=window, **kw)
        kw.update(out=out, pcm=pcm, peaks=peaks, counts=counts)   # (the next pass writes the same buffers)
        _, _, loud, blocks = lib.wave_loudness(out, samples, sr=sr, target=None)
        if k + 1 < passes:
            G = (G * towards(loud[:, 0])).contiguous()
    return out, pcm, loud, blocks, peaks, counts
