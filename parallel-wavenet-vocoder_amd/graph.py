"""The forward of an IAFVocoder captured once into a HIP graph and replayed.

The path is 16 dependent kernel launches per forward with the persistent stack launch (~115 on the per-layer path;
DESIGN.md section 4, "Launch structure": since round 5 one prologue launch or three plus ONE launch per flow); eager, every one costs a host enqueue and leaves a gap in front of the next
kernel.  Capturing the stream work (the launches of libpwv_hip.so on torch's current stream and, on the per-layer path,
on the two per-net side streams with their fork / join events) into one graph removes the host from the loop:
bit-identical results, 2 % faster at 160000 samples, 12 % at 16000 samples, 37 % for the one-flow configuration
(measured, tools/graph_bench.py).

No tracing and no compiler: the graph is exactly the launches `IAFVocoder.__call__` enqueues, with the buffers torch's
graph-private pool handed out during capture.  Shapes are fixed at capture (batch, length); the mel and the noise
are copied into static input tensors before each replay (or written there by the caller: `graphed.mel`), and the noise is
sampled by a node of the graph whose counter range lives in device memory (pwv_logistic_noise_stream_f32: a sampler with its
range passed by value would replay the same noise).

GraphedPackedVocoder does the same for packed batches of utterances of different lengths (IAFVocoder.generate_varlen with one noise
stream per utterance): captured once at a capacity of `slots` utterances and `rows` samples, replayed for any lengths that fit, the
layout and the streams rewritten in device tables before each replay and the free slots taken by filler utterances.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _lib, engine
from .hparam import hparam as hp
from .models import IAFVocoder, VarlenOutput, noise_streams


class GraphedVocoder(object):

    def __init__(self, model: IAFVocoder, device=None, warmup: int = 2):
        self.model = model
        store = model.store
        if store is None:
            from .variables import get_default_store
            store = get_default_store()
        self.store = store
        self.device = torch.device(device) if device is not None else store.device
        if self.device.type != 'cuda':
            raise engine._lib.PwvError('GraphedVocoder needs a GPU (cuda device); there is no CPU path')
        n, length = int(model.batch_size), int(model.length)
        self.mel = torch.zeros((n, model.t_mel, int(hp.signal.n_mels)), dtype=torch.float32, device=self.device)
        self.z = torch.zeros((n, length, 1), dtype=torch.float32, device=self.device)
        # the sampler is part of the graph: {seed, offset, ticket, skip} in device memory, advanced by the captured kernel itself
        # (pwv_logistic_noise_stream_f32), so a forward on sampled noise is ONE graph launch and nothing else
        self.noise_state = torch.zeros((4,), dtype=torch.int64, device=self.device)
        self._noise_mirror = (0, 0, 0)          # (seed, offset, skip) the device state holds
        self._last_drawn = 0                    # samples the replay that has not been verified yet took from the model's noise stream
        self._warmup = warmup
        self._capture()

    def _capture(self):
        # warm up on a side stream (plans packed, side streams created, allocator primed), as stream capture requires
        # (one stream for warm-up AND capture: what the warm-up forwards set up per stream -- the persistent launches' zeroed
        # workspace, engine._persist_ws -- is then found again by the captured forward instead of being allocated inside the graph)
        if getattr(self, '_stream', None) is None:
            self._stream = torch.cuda.Stream(device=self.device)
        side = self._stream
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            for _ in range(self._warmup):
                self.model(None, self.mel, is_training=False, z=self.z)
        torch.cuda.current_stream(self.device).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        # the captured launches carry THIS thread's sticky words (engine.current_words): verify() reads these, whoever replays
        self._words = engine.current_words(self.device)
        # thread_local: only this thread's calls are policed during capture (an RCCL watchdog thread of a multi-rank
        # job may touch the runtime meanwhile); everything captured here is enqueued from this thread
        with torch.cuda.graph(self.graph, stream=side, capture_error_mode='thread_local'):
            engine.logistic_noise_stream_op(self.z, self.noise_state)
            self.out = self.model(None, self.mel, is_training=False, z=self.z)
        self._version = self.store.version
        self._mode = self._launch_mode()

    @staticmethod
    def _launch_mode():
        """what decides WHICH launches a forward enqueues, besides the weights: a graph captured under another value is stale"""
        return engine.launch_knobs()

    def verify(self):
        """Replays only enqueue: wait for them and raise like IAFVocoder.verify().  After a PwvPersistError the engine has
        suspended the persistent launches (engine.suspend_persist); the graph is re-captured on the per-layer path here, so the
        caller's rerun replays launches that can complete -- and once the suspension has counted down (one tick per replay) the
        next call re-captures on the persistent path again (_launch_mode)."""
        try:
            engine.verify_enqueued(words=self._words)
        except engine._lib.PwvError as e:
            # the replay that failed drew its noise from the stream already: hand that range back, so that the caller's rerun
            # (z = None again) is a rerun ON THE SAME NOISE, like the eager path's (the device state is rewritten by the next call:
            # its mirror no longer matches)
            self.model.noise_offset -= self._last_drawn
            self._last_drawn = 0
            if isinstance(e, engine._lib.PwvPersistError):
                self._capture()
            raise
        self._last_drawn = 0

    def __call__(self, melspec: torch.Tensor, z: Optional[torch.Tensor] = None, seed: Optional[int] = None) -> torch.Tensor:
        """melspec [N, t_mel, n_mels] -- copied into the graph's input buffer, or that buffer itself (`graphed.mel`, filled by the caller:
        no copy); z [N, length, 1] or None (sample Logistic(0,1), models.py:32-33).
        Returns the graph's output buffer [N, length, 1]: valid until the next call (clone it to keep it).  Enqueue-only, like
        IAFVocoder.__call__(verify=False): call verify() before reading the result."""
        engine.note_forward()
        if self.store.version != self._version or self._mode != self._launch_mode():
            self._capture()      # weights changed (the captured launches point at stale packs) or the engine switched launch paths
        if tuple(melspec.shape) != tuple(self.mel.shape):
            raise ValueError('melspec must be %s (fixed at capture), got %s' % (tuple(self.mel.shape), tuple(melspec.shape)))
        if melspec is not self.mel:      # (a caller that writes its mel straight into the graph's input buffer `self.mel` passes that: no copy)
            self.mel.copy_(melspec, non_blocking=True)
        if z is None:
            # the captured sampler draws the model's next counter range (the stream IAFVocoder.sample_noise draws eagerly); the device
            # state is written from the host only when it is not what the previous replay left there (first call, another seed,
            # an eager draw in between, a call with explicit z before)
            want = (self.model._seed(seed), self.model.noise_offset, 0)
            self._set_noise_state(want)
            numel = self.z.numel()
            self.model.noise_offset += numel
            self._last_drawn = numel
            self._noise_mirror = (want[0], want[1] + numel, 0)
        else:
            if tuple(z.shape) != tuple(self.z.shape):
                raise ValueError('z must be %s, got %s' % (tuple(self.z.shape), tuple(z.shape)))
            self._last_drawn = 0
            self._set_noise_state((self._noise_mirror[0], self._noise_mirror[1], 1))      # skip: z is the caller's
            if z is not self.z:
                self.z.copy_(z, non_blocking=True)
        self.graph.replay()
        return self.out

    def _set_noise_state(self, want):
        if want != self._noise_mirror:
            # the state words are uint64 on the device (seeds up to 2**64 - 1, like the eager sampler's c_uint64): same bits as int64
            wrap = lambda v: (int(v) & ((1 << 64) - 1)) - (1 << 64) if (int(v) & (1 << 63)) else int(v) & ((1 << 64) - 1)  # noqa: E731
            self.noise_state.copy_(torch.tensor([wrap(want[0]), wrap(want[1]), 0, want[2]], dtype=torch.int64), non_blocking=False)
            self._noise_mirror = want


class GraphedPackedVocoder(object):
    """The packed forward of IAFVocoder.generate_varlen with one noise stream per utterance (seeds=), captured once at a capacity
    of `slots` utterances and `rows` samples and replayed for ANY lengths that fit it ("Graph replay of packed
    batches").  On the packed persistent route no launch argument depends on the individual lengths: the plan is made on N = 1,
    T = rows, the mel has rows / hop + slots frames, and the layout reaches the kernels only through the device tables cu_rows,
    cu_frames and the unit map.  So the graph holds the packed sampler (reading {seed_i, offset_i} from `streams`), the unit-map
    build, the prologue and the packed persistent flows, and a call rewrites the tables in place before the replay.

    A call with n < slots utterances adds slots - n FILLER utterances behind them: the first slots - n - 1 of `filler` rows (one hop,
    or the smallest multiple of hop of at least _lib.VARLEN_MIN_ROWS), the last one the remaining rows; zero mel, seed
    FILLER_SEED.  Every utterance's result depends on its own mel and stream only, so the fillers change no bit of the real ones.

    The model must take the packed persistent route on every flow at this capacity: anything else (a flow that would take the padded
    fallback, engine.varlen_fallback_reason, or that the library plans per layer; utterance-by-utterance instance normalisation;
    a materialised or normalised condition) is refused at construction with PwvError, since its launches depend on the lengths."""

    FILLER_SEED = 0

    def __init__(self, model: IAFVocoder, slots: int, rows: int, warmup: int = 2, device=None):
        self.model = model
        store = model.store
        if store is None:
            from .variables import get_default_store
            store = get_default_store()
        self.store = store
        self.device = torch.device(device) if device is not None else store.device
        if self.device.type != 'cuda':
            raise _lib.PwvError('GraphedPackedVocoder needs a GPU (cuda device); there is no CPU path')
        self.hop = hop = int(hp.signal.hop_length)
        self.filler = hop * -(-max(hop, _lib.VARLEN_MIN_ROWS) // hop)
        self.slots, self.rows = int(slots), int(rows)
        if self.slots < 1 or self.rows % hop or self.rows < self.slots * self.filler:
            raise ValueError('a capacity of %d slots needs rows a multiple of %d and at least %d, got %d'
                             % (self.slots, hop, self.slots * self.filler, self.rows))
        m = hp.model
        if 'in' in (m.get('normalize'), m.get('normalize_cond'), m.get('normalize_wavenet')):
            raise _lib.PwvError("GraphedPackedVocoder: instance normalisation ('in') runs packed batches utterance by utterance")
        if m.cond_upsample_method != 'repeat' or m.normalize_cond:
            raise _lib.PwvError('GraphedPackedVocoder: %r conditioning%s runs packed batches on the padded batch'
                                % (m.cond_upsample_method, ' with normalize_cond' if m.normalize_cond else ''))
        self.frames = self.rows // hop + self.slots
        self.mel = torch.zeros((self.frames, int(hp.signal.n_mels)), dtype=torch.float32, device=self.device)
        self.z = torch.zeros((self.rows, 1), dtype=torch.float32, device=self.device)
        # the three tables in ONE device buffer, written from one pinned staging copy per call: cu_rows, cu_frames (int32 [slots+1]
        # each), streams (int64 [slots, 2] = {seed_i, offset_i}, uint64 bits); two staging buffers, so that a call does not wait for
        # the copy of the previous one
        nt = 8 * (self.slots + 1) + 16 * self.slots
        self._tables = torch.zeros((nt,), dtype=torch.uint8, device=self.device)
        self.cu_rows = self._tables[:4 * (self.slots + 1)].view(torch.int32)
        self.cu_frames = self._tables[4 * (self.slots + 1):8 * (self.slots + 1)].view(torch.int32)
        self.streams = self._tables[8 * (self.slots + 1):].view(torch.int64).view(self.slots, 2)
        self._unit_map = torch.zeros(((self.rows + 31) // 32 * _lib.VARLEN_REC_INTS,), dtype=torch.int32, device=self.device)
        self._staging = [torch.zeros((nt,), dtype=torch.uint8).pin_memory() for _ in range(2)]
        self._staged = [None, None]
        self._flip = 0
        self._warmup = max(1, int(warmup))
        self._stream = None
        self._words = None
        self.graph = None
        self.captures = 0          # graphs captured so far (a weight or launch-knob change, or the end of a suspension, captures again)
        self.eager_calls = 0       # calls that ran the eager packed forward instead (a suspension, a layout that does not fit)
        self._capture()

    # -- layout ------------------------------------------------------------------------------------------------------------------
    def _layout(self, lengths):
        """The lengths of all `slots` utterances of a replay: the real ones, then the fillers; ValueError if they do not fit."""
        lengths = [int(v) for v in lengths]
        n = len(lengths)
        if not 1 <= n <= self.slots:
            raise ValueError('%d utterances for %d slots' % (n, self.slots))
        for v in lengths:
            if v < _lib.VARLEN_MIN_ROWS or v % self.hop:
                raise ValueError('utterance lengths must be multiples of hop_length (%d) of at least %d samples, got %d'
                                 % (self.hop, _lib.VARLEN_MIN_ROWS, v))
        k, left = self.slots - n, self.rows - sum(lengths)
        if k == 0:
            if left != 0:
                raise ValueError('%d utterances in all %d slots must fill the %d rows exactly, they hold %d' % (n, n, self.rows, self.rows - left))
            return lengths
        if left < k * self.filler:
            raise ValueError('%d rows and %d filler utterances of at least %d rows exceed the %d rows' % (self.rows - left, k, self.filler, self.rows))
        return lengths + [self.filler] * (k - 1) + [left - (k - 1) * self.filler]

    def fits(self, lengths) -> bool:
        """Can utterances of these lengths (samples) be replayed by this capture?"""
        try:
            self._layout(lengths)
        except ValueError:
            return False
        return True

    def _write_tables(self, lengths, streams):
        """cu_rows, cu_frames and streams of the layout `lengths` (fillers included) into the device tables: one copy from pinned
        staging, enqueued on the current stream."""
        k = self._flip
        self._flip ^= 1
        if self._staged[k] is not None:
            self._staged[k].synchronize()          # (the copy that last read this staging buffer has run)
        cu_rows, cu_frames = [0], [0]
        for v in lengths:
            cu_rows.append(cu_rows[-1] + v)
            cu_frames.append(cu_frames[-1] + v // self.hop + 1)
        pairs = list(streams) + [(self.FILLER_SEED, 0)] * (len(lengths) - len(streams))
        buf = self._staging[k].numpy()
        a = 4 * (self.slots + 1)
        buf[:a] = np.asarray(cu_rows, np.int32).view(np.uint8)
        buf[a:2 * a] = np.asarray(cu_frames, np.int32).view(np.uint8)
        buf[2 * a:] = np.asarray([engine.as_int64_bits(v) for p in pairs for v in p], np.int64).view(np.uint8)
        self._tables.copy_(self._staging[k], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._staged[k] = ev

    # -- capture -----------------------------------------------------------------------------------------------------------------
    def _enqueue(self):
        """The forward the graph holds: sampler, unit map, prologue, packed persistent flows (only enqueues)."""
        engine.logistic_noise_packed_op(self.cu_rows, self.streams, self.rows, out=self.z)
        self._geom.build_unit_map()
        m = self.model
        return engine.verified_call(lambda prec: m._forward_varlen(self.store, self.mel, self.z, self._geom, prec or m.precision),
                                    verify=False)

    def _capture(self):
        self.graph = None
        if engine.persist_suspended():
            return           # (no packed persistent route now: calls run eagerly until the suspension ends, then capture)
        if self._stream is None:
            self._stream = torch.cuda.Stream(device=self.device)
        side = self._stream
        layout = self._layout([self.filler])          # capture on an all-filler layout: any layout replays the same launches
        self._write_tables(layout, [])
        self._geom = engine.VarlenGeometry(layout, self.hop, self.device, tables=(self.cu_rows, self.cu_frames, self._unit_map))
        self.mel.zero_()
        # warm up on the capture stream (plans packed, allocator primed, that stream's persistent workspace created), as GraphedVocoder
        padded = engine.VARLEN_PADDED
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            for _ in range(self._warmup):
                self._enqueue()
        torch.cuda.current_stream(self.device).wait_stream(side)
        if engine.VARLEN_PADDED != padded:
            raise _lib.PwvError('GraphedPackedVocoder: a flow takes the padded fallback at %d slots / %d rows (%s): its launches depend on '
                                'the lengths, there is nothing to capture' % (self.slots, self.rows, engine.VARLEN_PADDED_WHY))
        engine.verify_enqueued('the warm-up of a packed graph')
        graph = torch.cuda.CUDAGraph()
        self._words = engine.current_words(self.device)
        with torch.cuda.graph(graph, stream=side, capture_error_mode='thread_local'):
            self.out = self._enqueue()
        self.graph = graph
        self._version = self.store.version
        self._mode = engine.launch_knobs()
        self.captures += 1

    # -- calls -------------------------------------------------------------------------------------------------------------------
    def __call__(self, melspecs, seeds, offsets=None):
        """Vocode n <= slots utterances (a list of [t_mel_i, n_mels] float32 mels on the GPU, len_i = (t_mel_i - 1) * hop samples)
        with noise streams (seeds[i], offsets[i]) -- the contract of IAFVocoder.generate_varlen(seeds=...): the same bits.  Returns
        a VarlenOutput of [len_i, 1] views of the graph's output buffer: valid until the next call (clone to keep).  Enqueue-only:
        call verify() before reading.  A layout that does not fit, or a call while the persistent launches are suspended, runs the
        eager generate_varlen(verify=False) instead and returns its result."""
        if not isinstance(melspecs, (list, tuple)) or not melspecs:
            raise ValueError('melspecs must be a non-empty list of [t_mel, n_mels] tensors')
        n_mels = int(hp.signal.n_mels)
        for i, m in enumerate(melspecs):
            if not hasattr(m, 'dim') or m.dim() != 2 or m.shape[1] != n_mels or m.shape[0] < 2:
                raise ValueError('melspecs[%d] must be [t_mel >= 2, %d], got %s' % (i, n_mels, tuple(getattr(m, 'shape', ()))))
        streams = noise_streams(seeds, offsets, len(melspecs))
        if streams is None:
            raise ValueError('a packed graph draws its noise from seeds: pass one per utterance')
        lengths = [(int(m.shape[0]) - 1) * self.hop for m in melspecs]
        if engine.persist_suspended():
            self.graph = None       # (the suspension retired the workspace the captured launches point at)
        if engine.persist_suspended() or not self.fits(lengths):
            self.eager_calls += 1
            return self.model.generate_varlen(list(melspecs), seeds=[s for s, _ in streams], offsets=[o for _, o in streams], verify=False)
        if self.graph is None or self.store.version != self._version or self._mode != engine.launch_knobs():
            self._capture()         # first call after a suspension, new weights (the launches point at stale packs), other launch knobs
        engine.note_forward()
        layout = self._layout(lengths)
        real_frames = sum(int(m.shape[0]) for m in melspecs)
        torch.cat([engine._require_cuda_f32(m, 'melspecs[%d]' % i) for i, m in enumerate(melspecs)], out=self.mel[:real_frames])
        self.mel[real_frames:].zero_()
        self._write_tables(layout, streams)
        self.graph.replay()
        geom = _Layout(lengths, self.hop)
        return VarlenOutput(self.out[:geom.rows], geom)

    def verify(self):
        """Wait for the enqueued calls and raise like IAFVocoder.verify(): PwvPersistError if a persistent launch gave up (the engine
        suspends the persistent launches; calls run eagerly meanwhile and the graph is captured again once the suspension ends),
        PwvRangeError if one left the range of the split-fp16 arithmetic.  The caller reruns with the same seeds: the same noise."""
        try:
            engine.verify_enqueued()
            if self._words is not None and self._words is not engine.current_words(self.device):
                engine.verify_enqueued(words=self._words)       # (a graph captured by another thread reports into that thread's words)
        except _lib.PwvPersistError:
            self.graph = None
            raise


class _Layout(object):
    """The layout of a replay's real utterances, in the shape VarlenOutput.geometry has (lengths, cu_rows_host, cu_frames_host)."""

    def __init__(self, lengths, hop):
        self.lengths, self.hop = list(lengths), hop
        self.cu_rows_host, self.cu_frames_host = [0], [0]
        for v in self.lengths:
            self.cu_rows_host.append(self.cu_rows_host[-1] + v)
            self.cu_frames_host.append(self.cu_frames_host[-1] + v // hop + 1)
        self.n, self.rows = len(self.lengths), self.cu_rows_host[-1]
