"""Config -- the reference's hyper-parameter object (models/tacotron.py:12-33) with the same field names and
defaults, plus the audio constants it derives `max_decode_iter` from (audio.py:10-17)."""
from __future__ import annotations

# audio.py:10-17
n_fft = 2048
win_length = 1200
hop_length = int(win_length / 4)
maximum_audio_length = 108000
r = 2

# data_input.py:15-18
BATCH_SIZE = 32
SHUFFLE_BUFFER_SIZE = 10000
MAX_TEXT_LEN = 140

# train.py:13-14
SAVE_EVERY = 5000
RESTORE_FROM = None


class Config(object):
    """Same attribute names as the reference; mutated at runtime by train()/test() exactly as the reference
    drivers do (`config.r`, `config.vocab_size`, `config.data_path`, `config.save_path`, `config.restore`)."""
    attention_units = 256
    decoder_units = 256
    mel_features = 80
    embed_dim = 256
    fft_size = 1025

    char_dropout_prob = 0.5
    audio_dropout_prob = 0.5

    num_speakers = 1
    speaker_embed_dim = 16

    scheduled_sample = 0.5

    cap_grads = 5

    init_lr = 0.0005
    annealing_rate = 1

    batch_size = 32

    # runtime-added in the reference (train.py:20-22,118-123); given defaults here so a bare Config() is usable
    r = r
    vocab_size = 60
    data_path = 'data/nancy/'
    save_path = 'nancy/tacotron'
    restore = False

    # synthesis only (test.py --sharpen BETA / --sharpen-lifter Q): the cepstral post-filter in front of the vocoder; None: off
    sharpen = None
    sharpen_lifter = 32

    # synthesis only (test.py --formant SEMITONES / --formant-lifter Q): the formant shift behind the post-filter; None: off
    formant = None
    formant_lifter = 32
    # synthesis only (test.py --pitch-range K / --pitch-range-smooth W / --pitch-range-limit OCT): the intonation range where the pitch
    # stage sits; None: off.  The two settings are UNTUNED (lib.F0_RANGE_SMOOTH, lib.F0_RANGE_LIMIT)
    pitch_range = None
    pitch_range_smooth = 2
    pitch_range_limit = 0.5

    # training only (train.py --ema DECAY; not in the reference): an exponential moving average of the parameters, kept on the device
    # beside the Adam slots and saved with them; 0: off -- no buffer, no launch, no checkpoint key.  No tuned default
    ema_decay = 0.0
    # synthesis only (test.py --ema): decode from the checkpoint's averaged weights instead of the live ones
    use_ema = False

    # models/tacotron.py:13 evaluates maximum_audio_length // (r hop_length) once, with audio.r; here `r` is changed at run time
    # (test.py from the checkpoint, train.py from meta.pkl), so the decode length follows the r in use unless a caller sets it
    _max_decode_iter = None

    @property
    def max_decode_iter(self):
        if self._max_decode_iter is not None:
            return self._max_decode_iter
        return maximum_audio_length // (self.r * hop_length)

    @max_decode_iter.setter
    def max_decode_iter(self, value):
        self._max_decode_iter = value

    def validate(self):
        """The HIP kernels compile the reference's layer widths in (include/taco_hip.h); refuse anything else loudly."""
        fixed = dict(attention_units=256, decoder_units=256, mel_features=80, embed_dim=256, fft_size=1025)
        for k, v in fixed.items():
            if getattr(self, k) != v:
                raise ValueError('Config.%s=%r is not supported by libtaco_hip (compiled for %r)' % (k, getattr(self, k), v))
        if self.num_speakers < 1:
            raise ValueError('Config.num_speakers must be >= 1')
        if self.num_speakers > 1 and self.speaker_embed_dim != 16:
            raise ValueError('Config.speaker_embed_dim=%r is not supported by libtaco_hip (compiled for 16)' % self.speaker_embed_dim)
        if not 0.0 <= float(self.ema_decay) < 1.0:   # (NaN fails)
            raise ValueError('Config.ema_decay must be in [0, 1) (0: no weight averaging), got %r' % (self.ema_decay,))
        if not (1 <= self.r <= 5):
            raise ValueError('Config.r must be in 1..5')
        for k in ('char_dropout_prob', 'audio_dropout_prob'):
            if getattr(self, k) not in (0, 0.0, 0.5):
                raise ValueError('Config.%s must be 0 or 0.5 (dropout scale 2 is compiled in)' % k)
