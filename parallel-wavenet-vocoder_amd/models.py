"""IAFVocoder: the 4-flow IAF-WaveNet student, the generation (forward) path.

Counterpart of /root/reference/models.py:16-141 with the same constructor / call signature
(`IAFVocoder(batch_size, length)`, `model(wav, melspec, is_training, name='iaf_vocoder')`,
`_upsample_cond(melspec, is_training, strides)`), reading the same global `hparam`.
The training side of models.py:80-103 (the L1 loss, its gradients, Adam and the EMA) is pwv_amd/train.py; tensorpack's ModelDesc is
not mirrored.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import engine
from .engine import RepeatedCondition
from .hparam import hparam as hp
from .modules import LinearIAFLayer, SharedIAFLayer, WaveNet, normalize
from .variables import VariableStore, get_default_store, get_variable, variable_scope


def torch_cat(parts):
    return parts[0] if len(parts) == 1 else torch.cat(parts)


class VarlenOutput(list):
    """What IAFVocoder.generate_varlen returns: the [len_i, 1] results of the utterances (views), with the packed [R, 1] result as
    `.packed` and the batch's layout (engine.VarlenGeometry: lengths, cu_rows, cu_frames) as `.geometry`."""

    def __init__(self, packed, geometry):
        r = geometry.cu_rows_host
        super().__init__(packed[a:b] for a, b in zip(r, r[1:]))
        self.packed = packed
        self.geometry = geometry


def noise_streams(seeds, offsets, n, z=None):
    """[(seed_i, offset_i)] of a packed batch of n utterances with one noise stream each (IAFVocoder.generate_varlen), or None when
    `seeds` is None (then `offsets` must be too).  Every value is an integer in [0, 2**64): the sampler's uint64."""
    if seeds is None:
        if offsets is not None:
            raise ValueError('offsets need seeds')
        return None
    if z is not None:
        raise ValueError('seeds and z exclude each other: seeds draw the noise, z is the noise')

    def ints(vals, what):
        vals = list(vals.tolist() if hasattr(vals, 'tolist') else vals)
        if len(vals) != n:
            raise ValueError('%s holds %d values for %d utterances' % (what, len(vals), n))
        return [engine.check_u64(v, '%s[%d]' % (what, i)) for i, v in enumerate(vals)]
    return list(zip(ints(seeds, 'seeds'), ints([0] * n if offsets is None else offsets, 'offsets')))


def check_packed_mels(melspecs) -> None:
    """The mel list of a packed call (IAFVocoder.generate_varlen, graph.GraphedPackedVocoder): [t_mel_i >= 2, n_mels] each."""
    if not isinstance(melspecs, (list, tuple)) or not melspecs:
        raise ValueError('melspecs must be a non-empty list of [t_mel, n_mels] tensors')
    for i, m in enumerate(melspecs):
        if not hasattr(m, 'dim') or m.dim() != 2 or m.shape[1] != hp.signal.n_mels or m.shape[0] < 2:
            raise ValueError('melspecs[%d] must be [t_mel >= 2, %d], got %s' % (i, hp.signal.n_mels, tuple(getattr(m, 'shape', ()))))


class IAFVocoder(object):

    def __init__(self, batch_size, length, store: Optional[VariableStore] = None, precision: Optional[str] = None):
        self.batch_size = batch_size
        self.t_mel = 1 + length // hp.signal.hop_length          # models.py:20
        self.length = length
        self.store = store
        self.precision = precision
        self.ema = None
        # Logistic noise (models.py:32-33 draws a fresh sample per sess.run): counter-based sampler, one seed per model
        # object and a running offset so that every call -- eager or graph replay -- continues the same stream.  The
        # default seed is drawn from the OS (PWV_NOISE_SEED pins it); ranks of a sharded job get different seeds that way.
        self.noise_seed = None
        self.noise_offset = 0            # counters drawn so far (a running total: calls may differ in batch size)

    def _seed(self, seed=None):
        import os
        if seed is not None:
            return int(seed)
        if self.noise_seed is None:
            env = os.environ.get('PWV_NOISE_SEED')
            self.noise_seed = int(env) if env else engine.os_seed()
        return self.noise_seed

    def sample_noise(self, n, device, out=None, seed=None):
        """[n, length, 1] Logistic(0,1) noise (models.py:32-33); consecutive calls draw consecutive counter ranges."""
        numel = n * self.length
        z = engine.logistic_noise_op((n, self.length, 1), device, seed=self._seed(seed), offset=self.noise_offset, out=out)
        self.noise_offset += numel
        return z

    # -- network (models.py:23-78) -------------------------------------------------------------------
    def __call__(self, wav, melspec, is_training=False, name='iaf_vocoder', z=None, verify=None):
        """wav is unused by the forward (as in the reference); melspec [N, t_mel, n_mels] on the
        GPU.  ``z`` (optional, [N, length, 1]) replaces the logistic noise sampled at
        models.py:32-33 so results are reproducible against the oracle.

        By default the call returns a VERIFIED result (engine.verified_call): it waits for its launches, and a forward whose
        persistent launch gave up or whose operands left the range of the split-fp16 arithmetic is rerun (per-layer launches /
        exact fp32) on the same noise before anything is handed back.  ``verify=False`` (or PWV_ASYNC=1) only enqueues, like
        the C ABI; the caller then calls ``verify()`` before it reads the result."""
        store = self.store or get_default_store()
        engine.raise_if_range_flag('an earlier call')       # sticky words of un-verified forwards that have completed since
        engine.raise_if_persist_failed()
        melspec = engine._require_cuda_f32(melspec, 'melspec')
        if melspec.dim() != 3 or melspec.shape[1] != self.t_mel or melspec.shape[2] != hp.signal.n_mels:
            raise ValueError('melspec must be [N, %d, %d], got %s' % (self.t_mel, hp.signal.n_mels, tuple(melspec.shape)))
        n = melspec.shape[0]
        if z is None:   # Logistic(0,1) noise, models.py:32-33 (drawn once: a rerun sees the same noise)
            noise = self.sample_noise(n, melspec.device)
        else:
            noise = engine._require_cuda_f32(z, 'z')
            if tuple(noise.shape) != (n, self.length, 1):
                raise ValueError('z must be [%d, %d, 1], got %s' % (n, self.length, tuple(noise.shape)))
        return engine.verified_call(lambda prec: self._forward(store, melspec, noise, is_training, name, prec or self.precision), verify)

    def _flows(self, store, is_training, precision):
        """The IAF flows of the model (models.py:36-67), set up inside the caller's variable scope (that opens no scope of theirs)."""
        shared = bool(hp.model.get('shared_nets', False))
        flows = []
        for i in range(hp.model.n_iaf):
            with variable_scope('iaf{}'.format(i)):
                kwargs = dict(
                    batch_size=self.batch_size,
                    dilations=hp.model.dilations[i],
                    filter_width=hp.model.filter_width,
                    residual_channels=hp.model.residual_channels,
                    dilation_channels=hp.model.dilation_channels,
                    skip_channels=hp.model.skip_channels,
                    use_biases=hp.model.use_biases,
                    condition_channels=hp.model.condition_channels,
                    use_skip_connection=hp.model.use_skip_connection,
                    is_training=is_training,
                    normalize=hp.model.normalize_wavenet,
                    store=store, precision=precision)
                if shared:   # build extension: BASELINE.json configs[1]
                    net = WaveNet(quantization_channels=2, input_channels=1, name='shared', **kwargs)
                    iaf = SharedIAFLayer(batch_size=hp.train.batch_size, net=net)
                else:
                    # quantization_channels=1: the output is a real value, models.py:42,57
                    scaler = WaveNet(quantization_channels=1, name='scalar', **kwargs)
                    shifter = WaveNet(quantization_channels=1, name='shifter', **kwargs)
                    iaf = LinearIAFLayer(batch_size=hp.train.batch_size, scaler=scaler, shifter=shifter)
                flows.append(iaf)
        return flows

    def _forward(self, store, melspec, input, is_training, name, precision, length=None, geom=None):
        """models.py:23-78: condition, then the flows; only enqueues.  `length` overrides the constructor's (the padded form of a
        packed batch); with `geom` (an engine.VarlenGeometry) `melspec` is the packed [1, F, n_mels] and `input` the packed [R, 1]."""
        with variable_scope(name):
            flows = self._flows(store, is_training, precision)
            all_nets = [net for iaf in flows for net in iaf.nets()]
            with variable_scope('cond'):
                # (the flows are set up first -- that opens no variable scope of theirs, models.py:26-29 stays ahead of :36-67 in the
                # variable order -- so that the one-launch prologue can project for all of them)
                condition = self._condition(melspec, is_training, strides=[4, 4, 5], store=store, precision=precision, nets=all_nets,
                                            length=length)   # (n, t, h)
                if hp.model.normalize_cond and condition is not None:
                    if isinstance(condition, RepeatedCondition):
                        condition = condition.materialize()
                    with variable_scope('normalize'):
                        condition = normalize(condition, is_training, hp.model.normalize_cond, store=store)
            # the frame-rate projections of every net depend on the mel only: one GEMM for all flows, ahead of the first
            engine.project_all(all_nets, condition, precision=precision)
            for i, iaf in enumerate(flows):
                if geom is not None:
                    input = engine.run_flow_varlen(iaf, input, condition, geom, precision)      # (R, 1)
                else:
                    input = iaf(input, condition)  # (n, t, h)
                # normalization (identity at the default hparams), models.py:70
                input = normalize(input, is_training, hp.model.normalize, name='normalize{}'.format(i), store=store)
        return input

    # -- mixed-length batches ("Packed batches") -----------------------------------------------------
    def generate_varlen(self, melspecs, z=None, verify=None, seeds=None, offsets=None):
        """One forward over utterances of DIFFERENT lengths, without padding them to the longest.  `melspecs`: a list of
        [t_mel_i, n_mels] float32 tensors on the GPU (t_mel_i >= 2); utterance i yields len_i = (t_mel_i - 1) * hop samples.
        Returns a list (VarlenOutput) of [len_i, 1] tensors, views of ONE packed [R, 1] result (R = sum of len_i), which is
        `.packed` of the list.  ``z`` (optional): the noise, packed [R, 1] or a list of [len_i, 1]; by default one draw of R
        counters that continues this model's stream (row r of the packed batch is counter noise_offset + r).  The constructor's
        `batch_size` and `length` are not used here.  ``verify`` as for __call__.
        ``seeds`` (optional, one integer in [0, 2**64) per utterance) gives every utterance a noise stream of its own, starting at
        counter ``offsets[i]`` (default 0): piece i is then exactly what IAFVocoder(1, len_i) with noise_seed = seeds[i] and
        noise_offset = offsets[i] returns for mel i alone, whatever its companions and its position; this model's noise_offset does
        not move.  Not together with ``z``."""
        check_packed_mels(melspecs)
        noise_streams(seeds, offsets, len(melspecs), z)      # (checked before anything touches the device)
        if isinstance(z, (list, tuple)):      # (each piece against its own utterance: a split that only adds up to R would misassign)
            if len(z) != len(melspecs):
                raise ValueError('z holds %d utterances, melspecs %d' % (len(z), len(melspecs)))
            for i, (v, m) in enumerate(zip(z, melspecs)):
                want = ((m.shape[0] - 1) * hp.signal.hop_length, 1)
                if tuple(getattr(v, 'shape', ())) != want:
                    raise ValueError('z[%d] must be %s (utterance %d), got %s' % (i, want, i, tuple(getattr(v, 'shape', ()))))
            z = torch_cat([engine._require_cuda_f32(v, 'z[%d]' % i) for i, v in enumerate(z)])
        mels = [engine._require_cuda_f32(m, 'melspecs[%d]' % i) for i, m in enumerate(melspecs)]
        hop = hp.signal.hop_length
        layout = engine.PackedLayout([(m.shape[0] - 1) * hop for m in mels], hop)
        return self.forward_packed(torch_cat(mels), layout.cu_frames_host, z=z, verify=verify, seeds=seeds, offsets=offsets)

    def forward_packed(self, mel_packed, cu_frames, z=None, verify=None, seeds=None, offsets=None):
        """generate_varlen on the packed form: `mel_packed` [F, n_mels] holds the utterances' frames one after the other and
        `cu_frames` (host ints, F = cu_frames[-1]) their prefix sums; returns the VarlenOutput (packed result [R, 1] as `.packed`).
        ``seeds`` / ``offsets`` as for generate_varlen."""
        cu = [int(v) for v in (cu_frames.tolist() if hasattr(cu_frames, 'tolist') else cu_frames)]
        streams = noise_streams(seeds, offsets, len(cu) - 1, z)
        store = self.store or get_default_store()
        engine.raise_if_range_flag('an earlier call')
        engine.raise_if_persist_failed()
        mel = engine._require_cuda_f32(mel_packed, 'mel_packed')
        if len(cu) < 2 or cu[0] != 0 or any(b - a < 2 for a, b in zip(cu, cu[1:])):
            raise ValueError('cu_frames must start at 0 and give every utterance at least 2 frames, got %s' % (cu,))
        if mel.dim() != 2 or mel.shape[1] != hp.signal.n_mels or mel.shape[0] != cu[-1]:
            raise ValueError('mel_packed must be [%d, %d], got %s' % (cu[-1], hp.signal.n_mels, tuple(mel.shape)))
        hop = hp.signal.hop_length
        geom = engine.VarlenGeometry([(b - a - 1) * hop for a, b in zip(cu, cu[1:])], hop, mel.device)
        if streams is not None:     # one stream per utterance, drawn before the route is chosen: every route sees the same noise
            noise = engine.logistic_noise_packed_op(geom.cu_rows, geom.stream_table(streams), geom.rows)
        elif z is None:   # one draw of R counters, continuing the stream (a rerun sees the same noise)
            noise = engine.logistic_noise_op((geom.rows, 1), mel.device, seed=self._seed(), offset=self.noise_offset)
            self.noise_offset += geom.rows
        else:
            noise = engine._require_cuda_f32(z, 'z')
            if tuple(noise.shape) != (geom.rows, 1):
                raise ValueError('z must be [%d, 1], got %s' % (geom.rows, tuple(noise.shape)))
        out = engine.verified_call(lambda prec: self._forward_varlen(store, mel, noise, geom, prec or self.precision), verify)
        return VarlenOutput(out, geom)

    def _forward_varlen(self, store, mel, noise, geom, precision):
        """The packed forward: the prologue on the concatenated frames (per frame: nothing changes), then every flow as
        engine.run_flow_varlen.  Configurations whose stages are not row-local on the packed batch run the model's ordinary forward on
        the zero-padded batch (a materialised or normalised condition) or utterance by utterance (instance normalisation, whose
        statistics span the whole time axis)."""
        m = hp.model
        if 'in' in (m.get('normalize'), m.get('normalize_cond'), m.get('normalize_wavenet')):
            outs = [self._forward(store, mel[a:b].unsqueeze(0), noise[r0:r1].unsqueeze(0), False, 'iaf_vocoder', precision, length=r1 - r0)
                    for a, b, r0, r1 in zip(geom.cu_frames_host, geom.cu_frames_host[1:], geom.cu_rows_host, geom.cu_rows_host[1:])]
            return torch_cat([o.reshape(-1, 1) for o in outs])
        if m.cond_upsample_method != 'repeat' or m.normalize_cond:
            out = self._forward(store, geom.pad_frames(mel), geom.pad_rows(noise), False, 'iaf_vocoder', precision, length=geom.max_len)
            return geom.unpad_rows(out)
        return self._forward(store, mel.unsqueeze(0), noise, False, 'iaf_vocoder', precision, length=geom.rows, geom=geom)

    # -- streaming ("Streaming") ---------------------------------------------------------------------
    def open_stream(self, slots=1, hist_alloc=None, transposed_conv=False, use_skip_connection=False):
        """A stream.StreamingVocoder over this model's weights: `slots` independent sessions that take their mel frames in pushes
        and return each push's samples -- bit for bit the samples the one-shot forward gives for the whole utterance, at the cost
        of the pushed rows alone (every layer keeps the last `dilation` rows of its input per session).  The constructor's
        `batch_size` and `length` are not used.  Pays when many sessions advance per call (32 sessions x 1600 samples: 2.57x faster
        than overlap-and-discard).  One session (measured at chunks of 800 .. 8000 samples), two, or four with chunks under 1600
        samples: overlap-and-discard through __call__ (timeshard.chain_halo samples recomputed per chunk, one persistent launch per
        flow) is quicker than the ~65 launches of a push, which the host's enqueue bounds at ~0.7 ms; the crossover is at four
        sessions x 1600 samples -- DESIGN.md section 9 "Streaming" has the measured table.  A RAGGED tick -- sessions that got different
        numbers of frames, new sessions next to running ones, a short last chunk -- is one call too: ``s.push_varlen([mel_i [f_i,
        n_mels], ...], slots=[...])`` returns the [T_i, 1] pieces (views of one packed tensor, `.packed`) from ONE packed launch per flow
        instead of one push per (frame count, fresh or running) group; same bits, same transaction rule.  `hist_alloc` (tests):
        called with a float count, returns the zero-filled float32 buffer the histories live in.
        ``transposed_conv=True`` is the request to stream a model with model.cond_upsample_method 'transposed_conv' (the bare call
        refuses such hparams, and the request under 'repeat' hparams is a PwvError): every sample of the condition depends on one mel
        frame, so the chunks still equal the one-shot forward bit for bit; a flow is then L per-layer launches with the condition GEMM
        inside, the head launch and the affine (no persistent launch, no graph replay).  DESIGN.md section 9, "Streaming transposed-conv
        conditioning" has the routes and the measured ticks.
        ``use_skip_connection=True`` is the request to stream a model with model.use_skip_connection (the bare call refuses such
        hparams, the request under hparams without the switch is a PwvError, and so is the request together with transposed_conv):
        the skip sum is row-local, so the chunks equal the one-shot forward bit for bit; a flow is then a streaming causal front, L
        per-layer launches that accumulate the chunk's skip sums, the head launch and the affine (no persistent launch, no graph
        replay).  DESIGN.md section 9, "Streaming the skip-connection architecture"."""
        from .stream import StreamingVocoder
        return StreamingVocoder(self, slots, hist_alloc=hist_alloc, transposed_conv=transposed_conv, use_skip_connection=use_skip_connection)

    def verify(self):
        """For callers of the enqueue-only form (verify=False / PWV_ASYNC=1): wait for the enqueued forwards and raise
        PwvPersistError if a persistent launch gave up (the engine is on per-layer launches from then on: rerun) or
        PwvRangeError if one left the range of the split-fp16 arithmetic (rerun with precision='f32'; the reference computes
        in fp32, models.py:81-82; include/pwv_hip.h "Range guard")."""
        engine.verify_enqueued()

    def _mel_limit(self, weights, store):
        """Largest |mel| for which every operand of the conditioning GEMMs stays inside fp16's range: each stage is
        relu(x @ w), so |out| <= |x|max * max column sum of |w|.  Cached per store version."""
        import torch
        key = (store.uid, store.version, len(weights))
        if getattr(self, '_mel_limit_key', None) != key:
            norms = torch.stack([w.abs().sum(dim=0).max() for w in weights]).cpu().tolist()
            bound, worst = 1.0, 1.0
            for nrm in norms:
                bound *= nrm
                worst = max(worst, bound)
            self._mel_limit_key, self._mel_limit_val = key, engine.F16_LIMIT / worst
        return self._mel_limit_val

    # -- condition upsampling (models.py:105-136) ----------------------------------------------------
    def _condition(self, melspec, is_training, strides, store, precision=None, nets=None, length=None, crop=True):
        """The condition in the form the kernels want: a lazy RepeatedCondition for 'repeat'
        (projected at frame rate inside the nets), a materialised [N, T, C] tensor for
        'transposed_conv', None otherwise.  `length` overrides the constructor's.  crop=False ('transposed_conv', a ragged streaming
        chunk): the stages' output as it is, [N, t_mel * hop, C], without the crop of models.py:124."""
        precision = precision or self.precision
        n_samples = self.length if length is None else length
        hop = hp.signal.hop_length
        method = hp.model.cond_upsample_method
        # models.py:106 holds every method to prod(strides) == hop; only the transposed convolutions read the strides, so 'repeat' and no
        # conditioning run at any even hop here (the oracle draws the same line)
        assert method != 'transposed_conv' or np.prod(np.array(strides)) == hop
        if n_samples % hop != 0:
            raise ValueError('length (%d) must be a multiple of hop_length (%d): the crop at models.py:124,133 '
                             'yields (t_mel-1)*hop samples' % (n_samples, hop))
        if hop < 2 or hop % 2:
            raise ValueError('hop_length (%d) must be even and at least 2: the crop [hop//2 : -(hop//2)] at models.py:124,133 leaves '
                             '(t_mel-1)*hop + 1 samples of an odd hop (and nothing of hop 1), so the reference has no answer there' % hop)
        n, t_mel, n_mels = melspec.shape
        C = hp.model.condition_channels
        if method == 'transposed_conv':
            cond = melspec.reshape(n * t_mel, n_mels)
            length = t_mel
            input_channels = n_mels
            ws = [get_variable('transposed_conv_{}_weights'.format(i), (1, stride, C, input_channels if i == 0 else C), store=store)
                  for i, stride in enumerate(strides)]
            # kernel width == stride: out[t*s + j, co] = sum_ci in[t, ci] * w[0, j, co, ci]  (a GEMM); the [Cin, s*C] operand
            # is re-laid-out once per weight version, not per forward
            key = (store.uid, store.version, tuple(strides))
            if getattr(self, '_tconv_key', None) != key:
                self._tconv_key = key
                self._tconv_mats = [w[0].permute(2, 0, 1).reshape(w.shape[3], stride * C).contiguous() for w, stride in zip(ws, strides)]
            wmats = self._tconv_mats
            if (precision or engine.DEFAULT_PRECISION) == 'f16x3':
                engine.range_check_op(melspec, self._mel_limit(wmats, store))
            for i, stride in enumerate(strides):
                wmat = wmats[i]
                cond = engine.linear_op(cond, wmat, None, relu=True, precision=precision)   # models.py:118-120
                input_channels = C
                length *= stride
                cond = cond.reshape(n * length, C)
                if hp.model.normalize_cond:
                    cond = normalize(cond.reshape(n, length, C), is_training, hp.model.normalize_cond,
                                     name='normalize_transposed_conv_{}'.format(i), store=store).reshape(n * length, C)
            cond = cond.reshape(n, length, C)
            if not crop:
                return cond
            return engine.crop_time_op(cond, length - hop, hop // 2)            # models.py:124
        elif method == 'repeat':
            w = get_variable('dense', [1, n_mels, C], store=store)
            split = (precision or engine.DEFAULT_PRECISION) == 'f16x3'
            if nets and not hp.model.normalize_cond:
                # range check + dense / relu + the projections of every net of the forward: ONE launch (bit-identical to the three)
                fused = engine.repeat_condition_with_projections(nets, melspec, w[0], hop, n_samples, precision,
                                                                 self._mel_limit([w[0]], store) if split else None)
                if fused is not None:
                    return fused
            if split:
                engine.range_check_op(melspec, self._mel_limit([w[0]], store))
            frames = engine.linear_op(melspec.reshape(n * t_mel, n_mels), w[0], None, relu=True,
                                      precision=precision)                              # models.py:128-130
            return RepeatedCondition(frames.reshape(n, t_mel, C), hop, hop // 2, n_samples)      # models.py:131-133
        return None

    def _upsample_cond(self, melspec, is_training, strides):
        """Reference signature (models.py:105): returns the upsampled condition [N, T, C] tensor."""
        melspec = engine._require_cuda_f32(melspec, 'melspec')
        with variable_scope('iaf_vocoder'):
            with variable_scope('cond'):
                cond = self._condition(melspec, is_training, strides, self.store or get_default_store())
        if isinstance(cond, RepeatedCondition):
            cond = cond.materialize()
        return cond
