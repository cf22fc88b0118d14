"""Tacotron -- host-side mirror of the reference's model object (models/tacotron.py:187-195).

Same constructor contract `Tacotron(config, inputs, train)` and the same public attributes
(`.seq2seq_output .output .alignments .loss .global_step .lr .config`); TF's `sess.run(train_op)` becomes
`.step(lr)` and `sess.run([output, alignments])` becomes `.run()`.  All arithmetic is in libtaco_hip.so.
"""
from __future__ import annotations

import torch

from . import lib
from .params import ParamBuffer


# the training monitor (Tacotron.monitor_sites): the buffers read after the forward pass and after the update, and the workspace row
# (under the enc. / post. prefix) of each histogram site of the reference's CBHG (models/ops.py:73-130)
MONITOR_FORWARD = ('workspace', 'seq2seq_output', 'output')
MONITOR_UPDATE = ('params', 'grads', 'adam_m', 'adam_v')
MONITOR_ROWS = (('conv_bank', 'pool'), ('conv_proj_pre_bn', 'pj2pre'), ('conv_res', 'res'), ('highway_out', 'h4'), ('encoded', 'out'))


def monitor_sites(shape):
    """Tacotron.monitor_sites for a training model of `shape` (a lib.TacoShape); needs no device."""
    table = lib.param_table(shape)
    rows = {name: (off, size) for name, off, size, _ in lib.workspace_table(shape, True)}
    sites = {'workspace': [('pre_net_out',) + rows['enc.p2']]}
    for scope, pre in (('encoder', 'enc.'), ('post', 'post.')):
        sites['workspace'] += [('%s/%s' % (scope, name),) + rows[pre + row] for name, row in MONITOR_ROWS]
    sites['seq2seq_output'] = [('seq2seq_output', 0, shape.B * shape.Td * 80 * shape.r)]
    sites['output'] = [('output', 0, shape.B * shape.Td * 1025 * shape.r)]
    for buf, group in (('params', 'param'), ('grads', 'grad'), ('adam_m', 'adam_m'), ('adam_v', 'adam_v')):
        sites[buf] = [('%s/%s' % (group, name), off, size) for name, off, size, _ in table]
    return sites


class Tacotron(object):
    ESCALATE_WINDOW = 2000   # steps: two exchange time-outs closer than this escalate the decoder mode (check())

    def __init__(self, config, inputs, train=True, device='cuda', params=None, seed=0, reducer=None):
        config.validate()
        self._last_timeout_step = None
        self.config = config
        self.train = train
        self.device = torch.device(device)
        self.reducer = reducer            # tacotron_amd.dist.GradReducer or None
        self.lr = config.init_lr
        self.global_step = 0
        self.merged = None                # tf.summary plumbing is out of scope
        B, Tt = inputs['text'].shape
        if train:
            Td = inputs['mel'].shape[1]
        else:
            Td = config.max_decode_iter
        self.shape = lib.make_shape(B, Tt, Td, config.r, config.vocab_size, config.num_speakers)
        if params is None:
            params = ParamBuffer(self.shape, self.device).init_(seed)
        self.params = params
        R80, F2 = config.mel_features * config.r, config.fft_size * config.r
        dev = self.device
        self.seq2seq_output = torch.empty(B, Td, R80, device=dev)
        self.output = torch.empty(B, Td, F2, device=dev)
        self.alignments = torch.empty(B, Td, Tt, device=dev)
        self.lengths = None               # (B) int32 decoder steps kept per row after run(stop=...); None after run()
        self._lengths = None
        self._align_scores = None         # (counts, means) of alignment_scores(), allocated at its first call
        self._align_path = None           # (path, dur, counts, mass, workspace) of alignment_path(), allocated at its first call
        self._mel_eval = None             # the tensors of predicted_mel() / mel_distortion(), allocated at their first call
        self._monitor = None              # plans, row ranges and workspace of monitor_stats(), built at its first call
        self.monitor_result = None        # lib.TensorStats over monitor_names, on the device (step(monitor=True), monitor_stats())
        self.monitor_names = None
        self.mel_mean = self.mel_std = None   # (80 r) statistics the corpus's mel targets were standardised with; None: identity
        self._loss = torch.zeros(3, device=dev)
        self.workspace = torch.empty(lib.workspace_bytes(self.shape, train) // 4, dtype=torch.float32, device=dev)
        self.masks = None
        # the decoder kernels' two error words (sticky: cleared here and by check(), never by the library)
        eoff = [o for name, o, s, d in lib.workspace_table(self.shape, train) if name == 'dec.err'][0]
        self._err = self.workspace[eoff:eoff + 2].view(torch.int32)
        self._census = self.workspace[eoff + 4:eoff + 12].view(torch.int32)
        lib.clear_error(self.shape, train, self.workspace)
        self.stft_mean = self.stft_std = None   # train.py:31-33: normalisation statistics travel with the checkpoint
        if train:
            n = params.numel
            self.grads = torch.zeros(n, device=dev)
            self.adam_m = torch.zeros(n, device=dev)
            self.adam_v = torch.zeros(n, device=dev)
            self._scratch = torch.zeros(256, device=dev)
            self._gnorm = torch.zeros(1, device=dev)
            # weight averaging (Config.ema_decay in (0, 1); lib.param_ema): the average starts as a COPY of the weights -- an update
            # with w = 1 would not give one, e + (p - e) is not p in fp32.  With averaging off none of these attributes exists
            decay = float(getattr(config, 'ema_decay', 0.0) or 0.0)
            if decay > 0.0:
                self.ema_decay = decay
                self.ema = params.flat.detach().clone()
                self.ema_updates = 0              # ATTEMPTED updates, like global_step (apply_gradients)
                self.ema_stats = torch.zeros(3, dtype=torch.float64, device=dev)   # what the last step(ema_stats=True) left
                self._ema_work = torch.empty(lib.param_ema_workspace_bytes(n), dtype=torch.uint8, device=dev)
                self._ema_said = False
            # the five mask tensors are views of ONE byte buffer (16-byte aligned pieces), so that neighbours with the same
            # Bernoulli parameter are filled by a single launch (all five, with the reference's default rates)
            shapes = (('enc_keep1', (B, Tt, 256)), ('enc_keep2', (B, Tt, 128)), ('dec_keep1', (B, Td, 256)),
                      ('dec_keep2', (B, Td, 128)), ('sample', (Td, B)))
            sizes = [((s[0] * s[1] * (s[2] if len(s) > 2 else 1)) + 15) // 16 * 16 for _, s in shapes]
            self._mask_flat = torch.empty(sum(sizes), dtype=torch.uint8, device=dev)
            self._mask_buf, self._mask_span, off = {}, {}, 0
            for (k, s), sz in zip(shapes, sizes):
                n = s[0] * s[1] * (s[2] if len(s) > 2 else 1)
                self._mask_buf[k] = self._mask_flat[off:off + n].view(*s)
                self._mask_span[k] = (off, sz)
                off += sz
            # per-rank dropout / scheduled-sampling streams: replicas share the parameters, not the masks
            rank = reducer.rank if reducer is not None else 0
            self._seed = seed * 1000003 + 17 + rank * 7919
        self.set_inputs(inputs)

    # -- inputs -----------------------------------------------------------------------------------------
    def set_inputs(self, inputs):
        dev = self.device
        sh = self.shape
        want = {'text': (sh.B, sh.Tt), 'text_length': (sh.B,)}
        if self.train:
            want.update(mel=(sh.B, sh.Td, 80 * sh.r), stft=(sh.B, sh.Td, 1025 * sh.r))
        if self.config.num_speakers > 1:
            want['speaker'] = (sh.B,)
        for k, shp in want.items():
            if k not in inputs:
                raise lib.TacoError('inputs[%r] is missing' % k)
            if tuple(inputs[k].shape) != shp:   # the kernels index with self.shape: a differently shaped batch would read past the tensors
                raise lib.TacoError('inputs[%r] has shape %s, this model was built for %s' % (k, tuple(inputs[k].shape), shp))
        self.inputs = {
            'text': inputs['text'].to(dev, torch.int32).contiguous(),
            'text_length': inputs['text_length'].to(dev, torch.int32).contiguous(),
        }
        self.speaker = None
        if self.config.num_speakers > 1:   # tacotron.py:117-124
            self.speaker = inputs['speaker'].to(dev, torch.int32).contiguous()
        if self.train:
            self.inputs['mel'] = inputs['mel'].to(dev, torch.float32).contiguous()
            self.inputs['stft'] = inputs['stft'].to(dev, torch.float32).contiguous()

    def draw_masks(self):
        """Dropout keep masks (keep prob 1-rate) and the scheduled-sampling Bernoulli mask (tacotron.py:41-43,84-85)."""
        c = self.config
        m = {}
        self._seed += 5
        want = [('enc_keep1', 1.0 - c.char_dropout_prob if c.char_dropout_prob else None),
                ('enc_keep2', 1.0 - c.char_dropout_prob if c.char_dropout_prob else None),
                ('dec_keep1', 1.0 - c.audio_dropout_prob if c.audio_dropout_prob else None),
                ('dec_keep2', 1.0 - c.audio_dropout_prob if c.audio_dropout_prob else None),
                ('sample', c.scheduled_sample if c.scheduled_sample else None)]
        i = 0
        while i < len(want):
            k, p = want[i]
            if p is None:
                i += 1
                continue
            j = i
            while j + 1 < len(want) and want[j + 1][1] == p:   # run of neighbours with the same parameter: one launch
                j += 1
            off = self._mask_span[k][0]
            end = self._mask_span[want[j][0]][0] + self._mask_span[want[j][0]][1]
            lib.fill_bernoulli(self._mask_flat[off:end], p, self._seed + i)
            for q in range(i, j + 1):
                m[want[q][0]] = self._mask_buf[want[q][0]]
            i = j + 1
        return m

    # -- train ------------------------------------------------------------------------------------------
    def forward(self, masks=None):
        i = self.inputs
        self.masks = masks
        lib.forward(self.shape, self.params.flat, i['text'], i['text_length'], i['mel'], i['stft'], masks,
                    self.seq2seq_output, self.output, self.alignments, self._loss, self.workspace, self.speaker)

    def backward(self):
        i = self.inputs
        lib.backward(self.shape, self.params.flat, i['text'], i['text_length'], self.seq2seq_output, self.alignments,
                     self.masks, self.grads, self.workspace, self.speaker)

    def apply_gradients(self, lr, ema_stats=False):
        """Guarded: if a decoder kernel flagged a timed-out exchange (on ANY rank -- the error words are MAX-reduced with
        the gradients) the update is skipped on the device and `global_gradient_norm` reads -1; check() raises.
        `global_step` counts ATTEMPTED updates (it is advanced on the host before the device decides): after a skipped update
        the Adam bias-correction step, the annealing cadence and the checkpoint numbering run ahead of the updates actually
        applied by the number of skipped steps -- which check() reports at the next synchronisation point, where the drivers
        stop.
        With weight averaging on (Config.ema_decay), lib.param_ema follows on the same stream under the same error words, so the
        average skips what Adam skips; `ema_updates` counts attempted updates like `global_step`, with the same caveat, and sets the
        warm-up (lib.ema_decay).  ema_stats: the call also leaves its three statistics in `self.ema_stats` (device, fp64)."""
        self.global_step += 1
        lib.clip_adam_step(self.params.flat, self.grads, self.adam_m, self.adam_v, lr, self.config.cap_grads,
                           self.global_step, self._scratch, self._gnorm, self._err)
        if hasattr(self, 'ema'):
            lib.param_ema(self.ema, self.params.flat, lib.ema_weight(self.ema_decay, self.ema_updates), self._err,
                          self.ema_stats if ema_stats else None, self._ema_work if ema_stats else None)
            self.ema_updates += 1

    def step(self, lr=None, masks='draw', monitor=False, ema_stats=False):
        """One `sess.run(train_op)`: forward + backward (+ gradient all-reduce, overlapped with the backward pass) +
        clip + Adam.  Everything is enqueued on the current stream; nothing is copied to the host.
        monitor: the training monitor (monitor_sites, lib.tensor_stats).  The activation sites are read between the forward and the
        backward pass, which may reuse workspace rows; the parameters, the gradients and both Adam slots AFTER the update: the update
        reads the gradient buffer and never writes it, so what is seen there is the (reduced) gradient the step used, next to the
        parameters and slots it left.  Seven calls, into `monitor_result`, which stays on the device.  False: not one launch, copy
        or synchronisation more than before.
        ema_stats (weight averaging on only): this step's lib.param_ema also writes `self.ema_stats` = (squared distance of the new
        weights from the average before the update, sum of the weights' squares, 1; or -1, -1, 0 for a skipped update), which stays
        on the device.  False: the averaging pass is one launch and reduces nothing."""
        if masks == 'draw':
            masks = self.draw_masks()
        self.forward(masks)
        if monitor:
            self.monitor_stats(MONITOR_FORWARD)
        self.backward()
        if self.reducer is not None:
            self.reducer.reduce_after_backward(self)
        if ema_stats and hasattr(self, 'ema'):
            self.apply_gradients(self.lr if lr is None else lr, ema_stats=True)
        else:
            self.apply_gradients(self.lr if lr is None else lr)
        if monitor:
            self.monitor_stats(MONITOR_UPDATE)

    # -- training monitor -----------------------------------------------------------------------------------
    def monitor_sites(self):
        """The named segments the monitor reads, per buffer: {buffer: [(name, offset, size)]} in floats of that buffer, the buffers
        in the order MONITOR_FORWARD + MONITOR_UPDATE.  `params`, `grads`, `adam_m` and `adam_v` hold every tensor of
        lib.param_table as param/<name>, grad/<name>, adam_m/<name> and adam_v/<name>; `workspace` holds the reference's
        tf.summary.histogram sites (models/tacotron.py:129, models/ops.py:73-130) under its names, as rows of lib.workspace_table
        (MONITOR_ROWS); `seq2seq_output` and `output` (tacotron.py:139,152) are the model's own tensors.  The reference's conv_proj
        has no buffer here: pj2pre is the projection in front of its batch-norm affine and `res` already holds the residual sum,
        so the former is reported, as conv_proj_pre_bn."""
        assert self.train, 'monitor_sites: a training model'
        return monitor_sites(self.shape)

    def _monitor_state(self, e_lo, e_hi, sub_bits):
        """Plans (once per model), the three result tensors over all sites and one workspace (once per bucket choice)"""
        m = self._monitor
        if m is None:
            sites = self.monitor_sites()
            bufs = {'params': self.params.flat, 'grads': self.grads, 'adam_m': self.adam_m, 'adam_v': self.adam_v,
                    'workspace': self.workspace, 'seq2seq_output': self.seq2seq_output.view(-1), 'output': self.output.view(-1)}
            m = self._monitor = {'plans': {}, 'rows': {}, 'bufs': bufs, 'buckets': None}
            at = 0
            for buf in MONITOR_FORWARD + MONITOR_UPDATE:
                m['plans'][buf] = lib.tensor_stats_plan([(o, s) for _, o, s in sites[buf]], bufs[buf].numel(), self.device)
                m['rows'][buf] = (at, at + len(sites[buf]))
                at += len(sites[buf])
            self.monitor_names = [name for buf in MONITOR_FORWARD + MONITOR_UPDATE for name, _, _ in sites[buf]]
        if m['buckets'] != (e_lo, e_hi, sub_bits):
            N, dev = len(self.monitor_names), self.device
            NB = len(lib.tensor_stats_edges(e_lo, e_hi, sub_bits)) - 1
            self.monitor_result = lib.TensorStats(torch.zeros(N, len(lib.STATS_COUNTS), dtype=torch.int64, device=dev),
                                                  torch.zeros(N, len(lib.STATS_MOMENTS), dtype=torch.float64, device=dev),
                                                  torch.zeros(N, NB, dtype=torch.int64, device=dev))
            need = max(lib.tensor_stats_workspace_bytes(p.n, p.n_items, NB) for p in m['plans'].values())
            m['work'] = torch.empty(need, dtype=torch.uint8, device=dev)   # (one for all: the calls follow each other on the stream)
            m['buckets'] = (e_lo, e_hi, sub_bits)
        return m

    def monitor_stats(self, buffers=None, e_lo=lib.STATS_E_LO, e_hi=lib.STATS_E_HI, sub_bits=lib.STATS_SUB_BITS):
        """lib.tensor_stats of the sites of `buffers` (names of monitor_sites; None: all seven) as the buffers are NOW, one call per
        buffer on the current stream, into the rows of `monitor_result` = lib.TensorStats(counts (N, 6), moments (N, 5), hist (N, NB))
        that belong to them; row i is `monitor_names[i]`.  The tensors are allocated once and returned every time; rows of buffers
        not asked for keep what an earlier call left (zeros at first).  No copy and no synchronisation."""
        m = self._monitor_state(e_lo, e_hi, sub_bits)
        res = self.monitor_result
        for buf in (MONITOR_FORWARD + MONITOR_UPDATE if buffers is None else buffers):
            lo, hi = m['rows'][buf]
            lib.tensor_stats(m['bufs'][buf], m['plans'][buf], e_lo, e_hi, sub_bits, res.counts[lo:hi], res.moments[lo:hi], res.hist[lo:hi],
                             m['work'])
        return res

    def check(self):
        """Raises TacoError if a decoder kernel reported a timed-out cluster exchange (the kernels never hang: every spin is
        bounded and a time-out sets a STICKY error word in the workspace, which also makes the Adam update skip itself).
        This is a host synchronisation -- the drivers call it where they already synchronise (loss logging, after
        inference).  The words are cleared here, after the error has been turned into an exception."""
        flags = self._err.tolist()
        if flags[0] or flags[1]:
            lib.clear_error(self.shape, self.train, self.workspace)
            # self-heal: a SECOND time-out within ESCALATE_WINDOW steps of the previous one moves this PROCESS to the next more
            # conservative decoder mode (include/taco_hip.h taco_decoder_mode: XCD-local exchange -> agent-scope exchange ->
            # decoder.hip, ~2 x slower per decoder step).  A single time-out -- e.g. another tenant briefly holding CUs -- only
            # costs the updates skipped while the flag was set: it must not degrade the rest of a multi-day run.
            mode = lib.decoder_mode()
            prev = self._last_timeout_step
            self._last_timeout_step = self.global_step
            repeat = prev is not None and self.global_step - prev <= self.ESCALATE_WINDOW
            # error word 2 = the placement rendezvous of a decoder3 launch found a cluster NOT CO-RESIDENT (a peer workgroup was not
            # dispatched within 50 ms: something else holds CUs the persistent kernel needs).  That is a diagnosis, not a transient:
            # both decoder3 modes need all 256 workgroups resident and every such launch costs 50 ms, so the process goes straight
            # to decoder.hip (mode 2), whose launch geometry is sized from the occupancy query.
            not_resident = 2 in (flags[0], flags[1]) and mode < 2
            escalate = (repeat or not_resident) and mode < 2
            new_mode = 2 if not_resident else mode + 1
            what = ('decoder cluster NOT CO-RESIDENT (error word 2: a peer workgroup was not dispatched within 50 ms -- another kernel '
                    'holds CUs the persistent decoder needs)' if not_resident else 'decoder cluster exchange timed out')
            e = lib.TacoError('%s (forward=%d, backward=%d) in decoder mode %d at step %d; parameter '
                              'updates were skipped while the flag was set%s' %
                              (what, flags[0], flags[1], mode, self.global_step,
                               ('; switched to decoder mode %d' % new_mode if not_resident else
                                '; second time-out within %d steps: switched to decoder mode %d' % (self.ESCALATE_WINDOW, new_mode))
                               if escalate else ('' if mode >= 2 else '; mode kept (first time-out in this window)')))
            e.recoverable = mode < 2
            e.not_resident = not_resident
            if escalate:
                lib.decoder_mode(new_mode)
            raise e

    def placement_census(self):
        """Diagnostic, accumulated over the decoder-forward launches since the last clear_error(); host synchronisation.
        decoder3.hip (cluster width 32): [workgroups whose cluster exchanges through its XCD's L2, workgroups of clusters that
        straddle XCDs (or TACO_DEC_V3_AGENT=1) and exchange at agent scope, 0, ...] -- the second number should be 0.
        decoder.hip (cluster width <= 16): histogram of (blockIdx - XCD id) mod 8; one non-zero bin = the fast placement."""
        return self._census.tolist()

    @property
    def loss(self):
        return self._loss[0]

    @property
    def loss_terms(self):
        """(seq2seq_loss, output_loss) -- the two sums of add_loss_op (tacotron.py:158-160) behind `loss`; device tensors."""
        return self._loss[1], self._loss[2]

    @property
    def decoder_mode(self):
        """The process-wide decoder mode in use (0 XCD-local exchange, 1 agent-scope exchange, 2 decoder.hip); see check()."""
        return lib.decoder_mode()

    @property
    def global_gradient_norm(self):
        return self._gnorm[0]

    # -- inference --------------------------------------------------------------------------------------
    def run(self, stop=None):
        """`sess.run([model.output, model.alignments])` for train=False (test.py:52-56).
        stop: a lib.TacoStopRule -- end detection (taco_infer_stop): `lengths` (B, int32, device) receives each row's decoder steps
        len_b, and rows t >= len_b of the outputs and alignments are 0.  None: the reference's fixed Td steps."""
        i = self.inputs
        if stop is None:
            self.lengths = None
            lib.infer(self.shape, self.params.flat, i['text'], i['text_length'], self.seq2seq_output, self.output,
                      self.alignments, self.workspace, self.speaker)
        else:
            if self._lengths is None:
                self._lengths = torch.empty(self.shape.B, dtype=torch.int32, device=self.device)
            self.lengths = self._lengths
            lib.infer_stop(self.shape, self.params.flat, i['text'], i['text_length'], stop, self.seq2seq_output, self.output,
                           self.alignments, self.lengths, self.workspace, self.speaker)
        return self.output, self.alignments

    # -- alignment monitor --------------------------------------------------------------------------------
    def alignment_scores(self, max_jump=lib.MAX_JUMP):
        """Per-utterance attention scores of `alignments` (lib.alignment_scores): (counts (B, 6) int32, means (B, 2) fp32) in the
        order lib.ALIGN_COUNTS / lib.ALIGN_MEANS.  After run(stop=...) each row is scored over its own `lengths` steps, otherwise
        (run(), a training step) over all Td.  One launch on the current stream into two tensors the model allocates once and
        returns every time; no copy and no synchronisation -- read them where the host synchronises anyway."""
        if self._align_scores is None:
            B = self.shape.B
            self._align_scores = (torch.empty(B, len(lib.ALIGN_COUNTS), dtype=torch.int32, device=self.device),
                                  torch.empty(B, len(lib.ALIGN_MEANS), dtype=torch.float32, device=self.device))
        counts, means = self._align_scores
        return lib.alignment_scores(self.alignments, self.inputs['text_length'], self.lengths, max_jump, counts, means)

    def alignment_path(self, max_jump=lib.PATH_JUMP, steps=None):
        """The best monotone path through each row of `alignments` (lib.alignment_path): (path (B, Td) int32, dur (B, Tt) int32,
        counts (B, 3) int32 in the order lib.PATH_COUNTS, mass (B) fp32).  After run(stop=...) each row's path runs over its own
        `lengths` steps, otherwise over all Td; `steps` (B) int32 on the device overrides both.  One launch on the current stream into
        tensors (and a workspace) the model allocates once and returns every time; no copy and no synchronisation."""
        if self._align_path is None:
            B, Td, Tt, dev = self.shape.B, self.shape.Td, self.shape.Tt, self.device
            self._align_path = (torch.empty(B, Td, dtype=torch.int32, device=dev), torch.empty(B, Tt, dtype=torch.int32, device=dev),
                                torch.empty(B, len(lib.PATH_COUNTS), dtype=torch.int32, device=dev),
                                torch.empty(B, dtype=torch.float32, device=dev),
                                torch.empty(lib.alignment_path_workspace_bytes(B, Td, Tt), dtype=torch.uint8, device=dev))
        path, dur, counts, mass, work = self._align_path
        return lib.alignment_path(self.alignments, self.inputs['text_length'], self.lengths if steps is None else steps, max_jump, path,
                                  dur, counts, mass, work)

    # -- held-out evaluation ------------------------------------------------------------------------------
    def _mel_eval_tensors(self, cepstra):
        B, Td, r, dev = self.shape.B, self.shape.Td, self.shape.r, self.device
        e = self._mel_eval
        if e is None:
            F = (Td // 4) * 4 * r
            e = self._mel_eval = {'frames': torch.empty(B, F, 80, device=dev), 'na': torch.empty(B, dtype=torch.int32, device=dev),
                                  'cost': torch.empty(B, device=dev), 'steps': torch.empty(B, dtype=torch.int32, device=dev),
                                  'zeros': torch.zeros(80 * r, device=dev), 'ones': torch.ones(80 * r, device=dev), 'stats': None,
                                  'basis': {}, 'work': {}}
        if cepstra is not None and cepstra not in e['basis']:
            e['basis'][cepstra] = torch.from_numpy(lib.dct_basis(80, 1, cepstra)).to(dev)
        return e

    def predicted_mel(self):
        """`seq2seq_output` as chronological de-normalised mel frames (B, F, 80), F = (Td / 4) 4 r (lib.denorm_unframe with
        `mel_mean` / `mel_std`; identity when they are None), and na (B) int32, the frames each row holds: lengths * r after
        run(stop=...), else F.  Enqueued on the current stream into tensors the model allocates once and returns every time."""
        e = self._mel_eval_tensors(None)
        if self.mel_mean is None:
            mean, std = e['zeros'], e['ones']
        else:
            if e['stats'] is None or e['stats'][0] is not self.mel_mean or e['stats'][1] is not self.mel_std:
                e['stats'] = (self.mel_mean, self.mel_std, torch.as_tensor(self.mel_mean, dtype=torch.float32).to(self.device).contiguous(),
                              torch.as_tensor(self.mel_std, dtype=torch.float32).to(self.device).contiguous())
            mean, std = e['stats'][2:]
        lib.denorm_unframe(self.seq2seq_output, mean, std, self.shape.r, spec=e['frames'])
        if self.lengths is None:
            e['na'].fill_(e['frames'].shape[1])
        else:
            torch.mul(self.lengths, self.shape.r, out=e['na'])
        return e['frames'], e['na']

    def mel_distortion(self, recorded, nb=None, cepstra=13, want_path=False):
        """Distance of the model's mel frames from `recorded` over a dynamic-time-warping path (lib.frame_dtw): recorded (B, Fb, 80)
        fp32 chronological de-normalised log-mel frames on the device, nb (B) int32 their frame counts or None (all Fb), cepstra the
        DCT coefficients 1 .. cepstra the distance is taken over (lib.dct_basis) -> (cost (B) fp32, steps (B) int32, na (B) int32),
        device tensors; lib.MCD_DB * cost / steps is the row's mel-cepstral distortion in dB, taken over this model's own 80-band
        natural-log mel frames.  The prediction is predicted_mel().  Everything is enqueued on the current stream into tensors the
        model allocates once (per cepstra / Fb) and returns every time; no copy and no synchronisation.
        want_path: the warp with its path (lib.frame_dtw_path; the same cost and steps) -> (cost, steps, na, path_a, path_b), the
        last two (B, F + Fb - 1) int32: the predicted and the recorded frame of every cell of the path, -1 behind steps."""
        cepstra = int(cepstra)
        lib._frames_arg('mel_distortion', 'recorded', recorded)
        e = self._mel_eval_tensors(cepstra)
        frames, na = self.predicted_mel()
        key = (recorded.shape[1], cepstra)
        if want_path:
            if key not in e.setdefault('path', {}):
                P = frames.shape[1] + recorded.shape[1] - 1
                e['path'][key] = (torch.empty(self.shape.B, P, dtype=torch.int32, device=self.device),
                                  torch.empty(self.shape.B, P, dtype=torch.int32, device=self.device),
                                  torch.empty(lib.frame_dtw_path_workspace_bytes(self.shape.B, frames.shape[1], *key), dtype=torch.uint8,
                                              device=self.device))
            path_a, path_b, work = e['path'][key]
            cost, steps, path_a, path_b = lib.frame_dtw_path(frames, recorded, na, nb, e['basis'][cepstra], e['cost'], e['steps'], path_a,
                                                             path_b, work)
            return cost, steps, na, path_a, path_b
        if key not in e['work']:   # (empty unless the coefficients of both sequences do not fit LDS: include/taco_hip.h)
            e['work'][key] = torch.empty(lib.frame_dtw_workspace_bytes(self.shape.B, frames.shape[1], *key), dtype=torch.uint8,
                                         device=self.device)
        cost, steps = lib.frame_dtw(frames, recorded, na, nb, e['basis'][cepstra], e['cost'], e['steps'], e['work'][key])
        return cost, steps, na

    # -- checkpoint (train.py:47,85-90: weights + Adam slots + global_step) --------------------------------
    def state_dict(self):
        """Weights + Adam slots + global_step + the spectrogram normalisation statistics (the reference keeps stft_mean /
        stft_std as checkpointed variables, train.py:31-33, and test.py:27-28,64 de-normalises with them)."""
        d = {'params': self.params.flat.detach().cpu(), 'global_step': self.global_step,
             'shape': (self.shape.r, self.shape.V), 'num_speakers': max(1, self.shape.S), 'taco_version': lib.version(),
             'decoder_mode': lib.decoder_mode()}
        if self.stft_mean is not None:
            d['stft_mean'] = torch.as_tensor(self.stft_mean, dtype=torch.float32).cpu()
            d['stft_std'] = torch.as_tensor(self.stft_std, dtype=torch.float32).cpu()
        if self.train:
            d['adam_m'] = self.adam_m.cpu()
            d['adam_v'] = self.adam_v.cpu()
            if hasattr(self, 'ema'):   # weight averaging on: the average travels with the Adam slots; off: no key
                d['ema'] = self.ema.cpu()
                d['ema_updates'] = self.ema_updates
                d['ema_decay'] = self.ema_decay
        return d

    def load_state_dict(self, d, use_ema=False):
        """use_ema (test.py --ema, evaluate.py --ema): the weights are the checkpoint's AVERAGED weights d['ema'] instead of the live
        ones; lib.TacoError when the checkpoint holds none (written without --ema, or imported from TF).
        A training model with weight averaging on continues the checkpoint's average and its update count when it has them; else
        the average starts again from the restored weights with ema_updates = 0, said once."""
        if use_ema and 'ema' not in d:
            raise lib.TacoError('the checkpoint holds no averaged weights (written without --ema, or imported): its keys are %s'
                                % ', '.join(sorted(str(k) for k in d)))
        if tuple(d.get('shape', (self.shape.r, self.shape.V))) != (self.shape.r, self.shape.V) or \
                int(d.get('num_speakers', max(1, self.shape.S))) != max(1, self.shape.S) or \
                d['params'].numel() != self.params.numel:
            raise lib.TacoError('checkpoint was written for (r, V)=%s, %s speaker(s), %d parameters; this model has (r, V)=%s, '
                                '%d speaker(s), %d parameters' % (d.get('shape'), d.get('num_speakers', '?'), d['params'].numel(),
                                                                  (self.shape.r, self.shape.V), max(1, self.shape.S), self.params.numel))
        if use_ema and d['ema'].numel() != self.params.numel:
            raise lib.TacoError('the checkpoint\'s averaged weights hold %d floats, this model has %d parameters'
                                % (d['ema'].numel(), self.params.numel))
        self.params.flat.copy_(d['ema'] if use_ema else d['params'])
        self.global_step = int(d.get('global_step', 0))
        if 'stft_mean' in d:
            self.stft_mean, self.stft_std = d['stft_mean'], d['stft_std']
        if self.train and 'adam_m' in d:
            self.adam_m.copy_(d['adam_m'])
            self.adam_v.copy_(d['adam_v'])
        if self.train and hasattr(self, 'ema'):
            if 'ema' in d and d['ema'].numel() == self.params.numel:
                self.ema.copy_(d['ema'])
                self.ema_updates = int(d.get('ema_updates', 0))
            else:
                self.ema.copy_(self.params.flat)
                self.ema_updates = 0
                if not self._ema_said:
                    self._ema_said = True
                    print('the checkpoint holds no averaged weights: the average starts from the restored weights (ema_updates = 0)')
