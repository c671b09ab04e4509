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

GraphedStream does it for a streaming tick (StreamingVocoder.push of n running sessions x f frames): the session state -- generation,
samples emitted, seed, kept frame -- lives on the device, a kernel at the head of the graph turns it into the tick's launch tables and a
kernel at its end commits the tick iff the sticky words are clean, so ticks are enqueued back to back without a host round trip.

GraphedRaggedStream is both at once: a RAGGED tick (StreamingVocoder.push_varlen of running sessions, every one its own frame count)
captured at a capacity of `slots` sessions and `rows` samples, the frame counts read from a device table by the kernel at the head of
the graph, the free entries taken by filler sessions, the commit on the device.

GraphedLiveStream puts the streaming mel front-end (audio_frontend.StreamingMel) in front of that ragged tick and the front-end's commit
behind it: wav chunks in, the sessions' next samples out, one graph launch, both halves committed or refused together on the device.
"""
from __future__ import annotations

import collections
import ctypes
import gc
from typing import Optional

import numpy as np
import torch

from . import _lib, engine
from .hparam import hparam as hp
from .models import IAFVocoder, VarlenOutput, check_packed_mels, noise_streams
from .stream import RaggedOutput
from .variables import get_default_store


class _Captured(object):
    """The capture lifecycle the three wrappers share ("The capture lifecycle").  A subclass provides _enqueue()
    -- the forward the graph holds, run `warmup` times and then captured, all on ONE side stream -- and, where it needs them, the
    hooks _before_capture(), _after_warmup() and _settle()."""

    PERSIST_ONLY = False       # the captured forward exists on the persistent route only: a suspension leaves nothing to capture

    def __init__(self, model, device, warmup):
        self.model = model
        self.store = model.store or get_default_store()
        self.device = torch.device(device) if device is not None else self.store.device
        if self.device.type != 'cuda':
            raise _lib.PwvError('%s needs a GPU (cuda device); there is no CPU path' % type(self).__name__)
        self._warmup = warmup
        self._stream = None
        self._words = None
        self.graph = None
        self.captures = 0          # graphs captured so far (new weights, other launch knobs or the end of a suspension capture again)
        self.eager_calls = 0       # calls that ran the eager forward instead (a suspension, a call that does not fit the capture)

    def _before_capture(self):
        """The state the warm-up and the capture run on (self._words is set)."""

    def _after_warmup(self):
        """What the warm-up has to have shown before its launches are captured."""

    def _settle(self):
        """Ahead of a re-capture: what is in flight on the stale graph."""

    def _capture(self):
        self.graph = None
        if self.PERSIST_ONLY and engine.persist_suspended():
            return           # (no persistent route now: calls run eagerly until the suspension ends, then capture)
        if self._stream is None:
            self._stream = torch.cuda.Stream(device=self.device)
        side = self._stream
        # the captured launches carry THIS thread's sticky words (engine.current_words): verify() reads these, whoever replays
        self._words = engine.current_words(self.device)
        self._before_capture()
        # warm up on a side stream (plans packed, side streams created, allocator primed), as stream capture requires
        # (one stream for warm-up AND capture: what the warm-up forwards set up per stream -- the persistent launches' zeroed
        # workspace, engine._persist_ws -- is then found again by the captured forward instead of being allocated inside the graph)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            for _ in range(self._warmup):
                self._enqueue()
        torch.cuda.current_stream(self.device).wait_stream(side)
        self._after_warmup()
        graph = torch.cuda.CUDAGraph()
        saved, engine.EVENT_LOG = engine.EVENT_LOG, None       # (the log brackets launches with timing events: not inside a capture)
        # No garbage collection inside the capture either: torch.cuda.graph does not collect before it begins, so a collection that
        # falls due while the forward is enqueued would run the finalizers of dead cycles from before -- device and pinned memory,
        # events -- as runtime calls of the capturing thread, which are none of the captured ones and which the runtime may refuse.
        # Whatever is due is collected behind the capture.
        collecting = gc.isenabled()
        gc.disable()
        try:
            # thread_local: only this thread's calls are policed during capture (an RCCL watchdog thread of a multi-rank
            # job may touch the runtime meanwhile); everything captured here is enqueued from this thread
            with torch.cuda.graph(graph, stream=side, capture_error_mode='thread_local'):
                self.out = self._enqueue()
        finally:
            engine.EVENT_LOG = saved
            if collecting:
                gc.enable()
        self.graph = graph
        self._version = self.store.version
        self._mode = engine.launch_knobs()
        self.captures += 1

    def _stale(self) -> bool:
        """No graph, new weights (the captured launches point at stale packs), or other values of what decides WHICH launches a forward
        enqueues (engine.launch_knobs; a suspension is one of them)."""
        return self.graph is None or self.store.version != self._version or self._mode != engine.launch_knobs()

    def _ready(self) -> bool:
        """Ahead of every replay: is there a graph that may be replayed now?  False: the caller runs eagerly (eager_calls)."""
        if self.PERSIST_ONLY and engine.persist_suspended():
            self.graph = None       # (the suspension retired the workspace the captured launches point at)
            return False
        if self._stale():
            self._settle()
            self._capture()
        return self.graph is not None

    def _verify_words(self, where: str = '') -> None:
        """engine.verify_enqueued on the captured pair of sticky words, then on the calling thread's where that is another pair (a graph
        captured by another thread reports into that thread's words)."""
        engine.verify_enqueued(where, words=self._words)
        if self._words is not None and self._words is not engine.current_words(self.device):
            engine.verify_enqueued(where)


class GraphedVocoder(_Captured):

    def __init__(self, model: IAFVocoder, device=None, warmup: int = 2):
        super().__init__(model, device, warmup)
        n, length = int(model.batch_size), int(model.length)
        self.mel = torch.zeros((n, model.t_mel, int(hp.signal.n_mels)), dtype=torch.float32, device=self.device)
        self.z = torch.zeros((n, length, 1), dtype=torch.float32, device=self.device)
        # the sampler is part of the graph: {seed, offset, ticket, skip} in device memory, advanced by the captured kernel itself
        # (pwv_logistic_noise_stream_f32), so a forward on sampled noise is ONE graph launch and nothing else
        self.noise_state = torch.zeros((4,), dtype=torch.int64, device=self.device)
        self._noise_mirror = (0, 0, 0)          # (seed, offset, skip) the device state holds
        self._last_drawn = 0                    # samples the replay that has not been verified yet took from the model's noise stream
        self._capture()

    def _enqueue(self):
        if torch.cuda.is_current_stream_capturing():      # (a node of the graph only: a warm-up forward leaves the device state alone)
            engine.logistic_noise_stream_op(self.z, self.noise_state)
        return self.model(None, self.mel, is_training=False, z=self.z)

    def verify(self):
        """Replays only enqueue: wait for them and raise like IAFVocoder.verify().  After a PwvPersistError the engine has
        suspended the persistent launches (engine.suspend_persist); the graph is re-captured on the per-layer path here, so the
        caller's rerun replays launches that can complete -- and once the suspension has counted down (one tick per replay) the
        next call re-captures on the persistent path again (_stale)."""
        try:
            self._verify_words()
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
        engine.note_forward()      # (ahead of _ready: the replay that ends a suspension re-captures on the persistent path)
        self._ready()
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
            self.noise_state.copy_(torch.tensor([engine.as_int64_bits(want[0]), engine.as_int64_bits(want[1]), 0, want[2]], dtype=torch.int64),
                                   non_blocking=False)
            self._noise_mirror = want


def packed_filler_rows(hop: int) -> int:
    """Rows of a filler utterance of GraphedPackedVocoder: one hop, or the smallest multiple of hop of at least _lib.VARLEN_MIN_ROWS."""
    hop = int(hop)
    return hop * -(-max(hop, _lib.VARLEN_MIN_ROWS) // hop)


def filler_layout(counts, entries: int, total: int, least: int, unit):
    """The counts of all `entries` entries of a replay at a fixed capacity: the caller's `counts`, then FILLERS -- all but the last of
    `least`, the last one what is left of `total`.  With every entry taken the counts fill `total` exactly.  unit = (what an entry is,
    what is counted), for the messages; ValueError if the counts do not fit."""
    counts, (whom, what) = [int(v) for v in counts], unit
    n = len(counts)
    if not 1 <= n <= entries:
        raise ValueError('%d %ss for %d slots' % (n, whom, entries))
    for v in counts:
        if v < least:
            raise ValueError('every %s needs at least %d %s, got %d' % (whom, least, what, v))
    k, left = entries - n, total - sum(counts)
    if k == 0:
        if left != 0:
            raise ValueError('%d %ss in all %d slots must fill the %d %s exactly, they hold %d' % (n, whom, n, total, what, total - left))
        return counts
    if left < k * least:
        raise ValueError('%d %s and %d filler %ss of at least %d %s exceed the %d %s' % (total - left, what, k, whom, least, what, total, what))
    return counts + [least] * (k - 1) + [left - (k - 1) * least]


def _fits(layout, counts) -> bool:
    try:
        layout(counts)
    except ValueError:
        return False
    return True


class GraphedPackedVocoder(_Captured):
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
    PERSIST_ONLY = True

    def __init__(self, model: IAFVocoder, slots: int, rows: int, warmup: int = 2, device=None):
        super().__init__(model, device, max(1, int(warmup)))
        self.hop = hop = int(hp.signal.hop_length)
        self.filler = packed_filler_rows(hop)
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
        self._capture()

    # -- layout ------------------------------------------------------------------------------------------------------------------
    def _layout(self, lengths):
        """The lengths of all `slots` utterances of a replay: the real ones, then the fillers; ValueError if they do not fit."""
        for v in lengths:          # (a multiple of hop of at least VARLEN_MIN_ROWS is at least a filler: filler_layout's own bound holds)
            if int(v) < _lib.VARLEN_MIN_ROWS or int(v) % self.hop:
                raise ValueError('utterance lengths must be multiples of hop_length (%d) of at least %d samples, got %d'
                                 % (self.hop, _lib.VARLEN_MIN_ROWS, v))
        return filler_layout(lengths, self.slots, self.rows, self.filler, ('utterance', 'rows'))

    def fits(self, lengths) -> bool:
        """Can utterances of these lengths (samples) be replayed by this capture?"""
        return _fits(self._layout, lengths)

    def _write_tables(self, lengths, streams):
        """cu_rows, cu_frames and streams of the layout `lengths` (fillers included) into the device tables: one copy from pinned
        staging, enqueued on the current stream."""
        k = self._flip
        self._flip ^= 1
        if self._staged[k] is not None:
            self._staged[k].synchronize()          # (the copy that last read this staging buffer has run)
        layout = engine.PackedLayout(lengths, self.hop)
        pairs = list(streams) + [(self.FILLER_SEED, 0)] * (len(lengths) - len(streams))
        buf = self._staging[k].numpy()
        a = 4 * (self.slots + 1)
        buf[:a] = np.asarray(layout.cu_rows_host, np.int32).view(np.uint8)
        buf[a:2 * a] = np.asarray(layout.cu_frames_host, np.int32).view(np.uint8)
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

    def _before_capture(self):
        layout = self._layout([self.filler])          # capture on an all-filler layout: any layout replays the same launches
        self._write_tables(layout, [])
        self._geom = engine.VarlenGeometry(layout, self.hop, self.device, tables=(self.cu_rows, self.cu_frames, self._unit_map))
        self.mel.zero_()
        self._padded = engine.VARLEN_PADDED

    def _after_warmup(self):
        if engine.VARLEN_PADDED != self._padded:
            raise _lib.PwvError('GraphedPackedVocoder: a flow takes the padded fallback at %d slots / %d rows (%s): its launches depend on '
                                'the lengths, there is nothing to capture' % (self.slots, self.rows, engine.VARLEN_PADDED_WHY))
        engine.verify_enqueued('the warm-up of a packed graph')

    # -- calls -------------------------------------------------------------------------------------------------------------------
    def __call__(self, melspecs, seeds, offsets=None):
        """Vocode n <= slots utterances (a list of [t_mel_i, n_mels] float32 mels on the GPU, len_i = (t_mel_i - 1) * hop samples)
        with noise streams (seeds[i], offsets[i]) -- the contract of IAFVocoder.generate_varlen(seeds=...): the same bits.  Returns
        a VarlenOutput of [len_i, 1] views of the graph's output buffer: valid until the next call (clone to keep).  Enqueue-only:
        call verify() before reading.  A layout that does not fit, or a call while the persistent launches are suspended, runs the
        eager generate_varlen(verify=False) instead and returns its result."""
        check_packed_mels(melspecs)
        streams = noise_streams(seeds, offsets, len(melspecs))
        if streams is None:
            raise ValueError('a packed graph draws its noise from seeds: pass one per utterance')
        lengths = [(int(m.shape[0]) - 1) * self.hop for m in melspecs]
        if not self._ready() or not self.fits(lengths):
            self.eager_calls += 1
            return self.model.generate_varlen(list(melspecs), seeds=[s for s, _ in streams], offsets=[o for _, o in streams], verify=False)
        engine.note_forward()
        layout = self._layout(lengths)
        real_frames = sum(int(m.shape[0]) for m in melspecs)
        torch.cat([engine._require_cuda_f32(m, 'melspecs[%d]' % i) for i, m in enumerate(melspecs)], out=self.mel[:real_frames])
        self.mel[real_frames:].zero_()
        self._write_tables(layout, streams)
        self.graph.replay()
        real = engine.PackedLayout(lengths, self.hop)
        return VarlenOutput(self.out[:real.rows], real)

    def verify(self):
        """Wait for the enqueued calls and raise like IAFVocoder.verify(): PwvPersistError if a persistent launch gave up (the engine
        suspends the persistent launches; calls run eagerly meanwhile and the graph is captured again once the suspension ends),
        PwvRangeError if one left the range of the split-fp16 arithmetic.  The caller reruns with the same seeds: the same noise."""
        try:
            self._verify_words()
        except _lib.PwvPersistError:
            self.graph = None
            raise


class _TickGraph(_Captured):
    """ONE tick of a StreamingVocoder captured into a HIP graph with the commit on the device -- what GraphedStream and
    GraphedRaggedStream are ("Graph replay of a streaming tick"):

        begin kernel (session table [+ frame counts] -> slot table, noise streams, cu_rows [, cu_frames], the chunk's frames)  ->
        packed sampler (sample=True)  ->  [pwv_varlen_unit_map]  ->  StreamingVocoder._enqueue (prologue, carry, one persistent
        streaming launch per flow)  ->  commit kernel

    The session table lives on the device; a tick's `entries` -- the called slots (live = 1), then FILLERS on other slots of the stream
    (live = 0: they read their slot's generation g and write generation 1 - g, which is scratch until a flip, and are never committed)
    -- and rewritten session rows go through pinned staging; at most `depth` ticks are in flight.  A subclass validates its capacity,
    allocates mel, z and _chunk, calls _start() and provides what differs: ARGS / ENTRY / FIRST_PUSH, _shape_args, _push_args,
    _capture_columns, _good_warmup, and the tick's _check_mel, _check_z, _columns, _eager and _copy_in."""

    PERSIST_ONLY = True
    PACKED = False             # the push is a packed one: cu_rows with or without a sampler, cu_frames and the unit map besides

    def __init__(self, stream, sample, depth, warmup):
        stream._refuse_graph(type(self).__name__)      # (per-sample conditioning: no whole-flow persistent launch to capture)
        self.stream = stream
        super().__init__(stream.model, stream.device, max(1, int(warmup)))
        self.sample, self.depth = bool(sample), max(1, int(depth))

    def _start(self, n: int):
        """The tables and the state of a tick of `n` entries, then the first capture (self.mel, self.z and self._chunk exist)."""
        st, dev, ints = self.stream, self.device, self.ENTRY_INTS
        self._n = n
        self._check_route()
        self._tab = torch.zeros((n, 2), dtype=torch.int32, device=dev)
        self._streams = torch.zeros((n, 2), dtype=torch.int64, device=dev) if self.sample else None
        self._cu_rows = torch.zeros((n + 1,), dtype=torch.int32, device=dev) if self.sample or self.PACKED else None
        self._cu_frames = torch.zeros((n + 1,), dtype=torch.int32, device=dev) if self.PACKED else None
        self._unit_map = torch.zeros(((self.z.numel() + 31) // 32 * _lib.VARLEN_REC_INTS,), dtype=torch.int32, device=dev) if self.PACKED else None
        self._entries = torch.zeros((n, ints), dtype=torch.int32, device=dev)
        self._counters = torch.zeros((2,), dtype=torch.int64, device=dev)      # {ticks committed, ticks refused}
        # pinned staging of the entries and of rewritten session rows: one pair per tick that may be in flight
        self._entries_host = [torch.zeros((n, ints), dtype=torch.int32).pin_memory() for _ in range(self.depth)]
        self._rows_host = [torch.zeros((n, 4), dtype=torch.int64).pin_memory() for _ in range(self.depth)]
        self._entries_dev = None                # the entries the device table holds, column by column (slots, live flags[, frames])
        self._counters_host = torch.zeros((2,), dtype=torch.int64).pin_memory()
        self._sess_back = torch.zeros((st.n_slots, 4), dtype=torch.int64).pin_memory()
        self._events = collections.deque()      # the end events of the ticks in flight (at most `depth`)
        self._inflight = set()                  # the slots ticks in flight were called with
        self._ticks = 0
        self._seen = [0, 0]                     # the counters at the last verify()
        self._carry = 0                         # eager ticks settled on the way (counted by the next verify())
        self._dirty_rows = 0                    # leading rows of mel (and their part of z) that may hold a previous tick's values
        # starts in flight (GraphedRaggedStream.tick(starts=)): the graphed ticks replayed since the last verify(), (the tick's number
        # among them, slot, the seed the call gave) per start, and the slots that have one
        self._window = 0
        self._starts_log = []
        self._started = set()
        self._capture()

    def _refusal(self, rows: int) -> Optional[str]:
        m = hp.model
        if engine.PERSIST is False:
            return 'PWV_PERSIST=0 (engine.PERSIST False): pushes run on per-layer streaming launches'
        for i, d in enumerate(m.dilations[:m.n_iaf]):
            if len(d) < 4:
                return 'flow %d has %d layers (L < 4): the library plans it per layer' % (i, len(d))
        if engine.PERSIST == 'auto' and rows > engine.PERSIST_AUTO_MAX_ROWS:
            return '%d rows are above PERSIST_AUTO_MAX_ROWS (%d)' % (rows, engine.PERSIST_AUTO_MAX_ROWS)
        return None

    def _fillers(self, called, count: int):
        """`count` filler slots for a tick of the slots `called`: other slots of the stream, running ones first."""
        st = self.stream
        others = sorted((s for s in range(st.n_slots) if s not in called), key=lambda s: not st._running[s])[:count]
        for s in others:
            if not st._running[s]:
                st._scratch_dirty[s] = True       # (a fresh slot's other generation is zeros no longer: StreamingVocoder._commit)
        return others

    def _capture(self):
        # the warm-up is judged by what it enqueued (_after_warmup): it runs under a log of its own where none is live
        own = engine.EVENT_LOG is None
        if own:
            engine.EVENT_LOG = []
        try:
            super()._capture()
        finally:
            if own:
                engine.EVENT_LOG = None

    def _settle(self):
        if self.stream._pending is not None:
            self._carry = self.verify()        # (what it returns counts the carry in)

    def _begin_tick(self) -> int:
        """Ahead of a replay: what others left in flight is settled, at most `depth` ticks of ours stay in flight.  Returns the staging
        pair of this tick."""
        if self.stream._ticker is not self:
            self._settle()          # an eager push that only enqueued (or another graph's ticks): settled first
        engine.note_forward()
        if len(self._events) >= self.depth:
            self._events.popleft().synchronize()       # bounds the work that can pile up behind a refused tick (and frees staging j)
        j = self._ticks % self.depth
        self._ticks += 1
        return j

    def _replay(self, slots) -> None:
        st = self.stream
        self.graph.replay()
        ev = torch.cuda.Event()
        ev.record()
        self._events.append(ev)
        self._window += 1
        self._inflight.update(slots)
        st._pending, st._ticker = self.verify, self

    def _sync_rows(self, j: int, slots, fillers, starts=()) -> None:
        """The session rows of the tick's entries -- the called slots, then the fillers --, rewritten where the host's view says the device
        row differs (first tick, an eager push, reset or load_state since).  A filler needs its row as much as a called slot: the
        generation it WRITES must be the one the session does not stand on.  A slot with ticks in flight is the device's: its row is
        what those ticks leave.  A slot in `starts` begins an utterance in this tick: its seed and counter come from the starts table."""
        st, rows = self.stream, self._rows_host[j]
        for i, s in enumerate(list(slots) + list(fillers)):
            if s in self._inflight:
                continue
            have, seed = st._sess_host[s], st._seed[s]
            if i >= len(slots) or s in starts:
                # a filler's noise is nobody's (a start brings its own): only the generation and the counter have to be the session's
                if have is not None and have[:2] == (st._gen[s], st._emitted[s]):
                    continue
                seed = seed if seed is not None else 0
            elif seed is None:
                seed = engine.os_seed() if self.sample else 0
            want = (st._gen[s], st._emitted[s], engine.as_int64_bits(seed))
            if have != want:
                rows[i, 0], rows[i, 1], rows[i, 2], rows[i, 3] = want[0], want[1], want[2], 0
                st._sess[s].copy_(rows[i], non_blocking=True)
                st._sess_host[s] = want

    def verify(self) -> int:
        """Wait for the ticks in flight, make the host's view of their sessions (generation, emitted, seed, running) equal to the device
        table and return the number of ticks committed since the last verify().  Raises PwvRangeError / PwvPersistError, with that
        number as `.committed`, if a sticky word is raised: the committed ticks are the first `.committed` ones, the sessions stand
        behind them.  After a PwvPersistError the graph is dropped: ticks run eagerly until the suspension ends, then capture again."""
        st = self.stream
        if st._ticker is not self:
            if st._ticker is not None:
                return st._ticker.verify()
            had = st._pending is not None          # an eager tick (push(verify=False)) of ours
            try:
                st.verify()
            except _lib.PwvError as e:
                e.committed, self._carry = self._carry, 0
                if isinstance(e, _lib.PwvPersistError):
                    self.graph = None
                raise
            done, self._carry = self._carry + (1 if had else 0), 0
            return done
        if self._events:
            torch.cuda.current_stream(self.device).wait_event(self._events[-1])      # (verify() from another stream than the ticks')
        self._counters_host.copy_(self._counters, non_blocking=True)
        self._sess_back.copy_(st._sess, non_blocking=True)
        torch.cuda.synchronize()
        counters = [int(v) for v in self._counters_host.tolist()]
        committed, refused = counters[0] - self._seen[0], counters[1] - self._seen[1]
        self._seen = counters
        table = self._sess_back.tolist()
        # the committed ticks are a prefix: a start is committed iff its tick is among the first `committed` of this window
        began = {s: seed for k, s, seed in self._starts_log if k < committed}
        for s in self._inflight:
            gen, emitted, seed = int(table[s][0]) & 1, int(table[s][1]), int(table[s][2])
            st._gen[s], st._emitted[s] = gen, emitted
            st._sess_host[s] = (gen, emitted, seed)
            if s in self._started and s not in began and not st._running[s]:
                # a refused start leaves a fresh slot fresh (seed and all); the generation it wrote is scratch, as after a filler
                st._scratch_dirty[s] = True
                continue
            st._running[s] = True
            if self.sample:
                st._seed[s] = engine.from_int64_bits(seed)
            elif s in began:
                st._seed[s] = began[s]          # (the caller's noise: the seed is kept as reset(slot, seed) would keep it)
            if s in began:
                st._scratch_dirty[s] = False
        self._window, self._starts_log = 0, []
        self._started.clear()
        self._inflight.clear()
        self._events.clear()
        st._pending, st._ticker = None, None
        committed, self._carry = committed + self._carry, 0
        try:
            self._verify_words('a graphed streaming tick')
            if refused:
                raise _lib.PwvError('%d graphed ticks were refused by their commit (a sticky word was raised and has been cleared since)' % refused)
        except _lib.PwvError as e:
            e.committed = committed
            if isinstance(e, _lib.PwvPersistError):
                self.graph = None
            raise
        return committed

    # -- capture -----------------------------------------------------------------------------------------------------------------
    def _check_route(self):
        why = self._refusal(self.z.numel())
        if why is not None:
            raise _lib.PwvError('%s: %s: %s' % (type(self).__name__, self._not_one_launch(), why))

    def _tick_args(self):
        st, ta = self.stream, self.ARGS()
        ta.sess, ta.kept, ta.entries, ta.mel = st._sess.data_ptr(), st._kept.data_ptr(), self._entries.data_ptr(), self.mel.data_ptr()
        ta.n_slots, ta.N, ta.n_mels = st.n_slots, self._n, st.n_mels
        ta.slot_tab, ta.chunk = self._tab.data_ptr(), self._chunk.data_ptr()
        for name in ('streams', 'cu_rows', 'cu_frames'):
            if getattr(self, '_' + name) is not None:
                setattr(ta, name, getattr(self, '_' + name).data_ptr())
        ta.words, ta.counters = self._words.addr, self._counters.data_ptr()
        self._shape_args(ta)
        return ta

    def _enqueue(self):
        """The tick the graph holds (only enqueues): begin, sampler, unit map (a packed push), the push's own launches, commit."""
        st, lib, ta = self.stream, _lib.lib(), self._tick_args()
        _lib.check(getattr(lib, self.ENTRY + '_begin')(ctypes.byref(ta), engine._stream()), self.ENTRY + '_begin')
        if self.sample:
            engine.logistic_noise_packed_op(self._cu_rows, self._streams, self.z.numel(), out=self.z.view(-1, 1))
        if self.PACKED:
            self._geom.build_unit_map()
        out = engine.verified_call(lambda prec: st._enqueue(prec or self.model.precision, *self._push_args()), verify=False)
        _lib.check(getattr(lib, self.ENTRY + '_commit')(ctypes.byref(ta), engine._stream()), self.ENTRY + '_commit')
        return out

    def _write_entries(self, k: int, called, *columns):
        """The tick's entry table through pinned staging `k`: {slot, live[, one int of every one of `columns`], 0 ...} -- the called slots
        with live = 1, then fillers -- other slots of the stream, running ones first -- with live = 0.  Returns the fillers' slots."""
        others = self._fillers(called, self._entries.shape[0] - len(called))
        # (the key is the whole table, live flags included: the same slots [and frames] with another number of called sessions differ in them)
        table = (tuple(called) + tuple(others), (1,) * len(called) + (0,) * len(others)) + tuple(tuple(c) for c in columns)
        if table != self._entries_dev:          # (else the device table holds these entries already: the previous tick's)
            buf = self._entries_host[k].numpy()
            buf[:] = 0
            for c, column in enumerate(table):
                buf[:, c] = column
            self._entries.copy_(self._entries_host[k], non_blocking=True)
            self._entries_dev = table
        return others

    def _before_capture(self):
        self._check_route()
        # warm up and capture on an all-filler table: no session is touched, any entries replay the same launches
        self._sync_rows(0, [], self._write_entries(0, [], *self._capture_columns()))
        self.mel.zero_()
        self.z.zero_()
        self._dirty_rows = 0
        self._log_mark = len(engine.EVENT_LOG)

    @staticmethod
    def _one_launch(e) -> bool:
        """An event of the log: a whole-flow persistent launch of one workgroup set, streaming."""
        return e[0] == 'persist' and e[8] == 1 and e[5] == 1 and e[6] == 1

    def _after_warmup(self):
        log = engine.EVENT_LOG[self._log_mark:]
        if not self._good_warmup(log, self._warmup * int(hp.model.n_iaf)):
            raise _lib.PwvError('%s: %s (the warm-up enqueued %s)' % (type(self).__name__, self._not_one_launch(),
                                                                      [e[0] if e[0] != 'stream_ragged' else e[:5] for e in log]))
        engine.verify_enqueued('the warm-up of a graphed streaming tick')
        self._counters.zero_()
        self._seen = [0, 0]

    # -- ticks -------------------------------------------------------------------------------------------------------------------
    def tick(self, mel, slots, z=None):
        """Give the distinct RUNNING sessions in `slots` their next frames `mel` (the subclass says in which form) and return their next
        samples as views of the graph's output buffer, valid until the next tick (a caller that pipelines ticks copies them out on the
        stream).  sample=False: z is the noise; sample=True: every slot draws from its own counter stream (a slot without a seed gets
        one from the OS, as in push).  Enqueue-only; before tick j is enqueued the host waits for the end of tick j - depth.  A tick
        that does not fit the capture, or one while the persistent launches are suspended, settles what is in flight (verify()) and
        runs the eager push instead (eager_calls)."""
        return self._tick(mel, slots, z, None)

    def _check_starts(self, starts, slots, frames) -> dict:
        """{slot: seed or None} of the sessions that begin an utterance in this tick ({}: none; the ragged tick alone takes any)."""
        return {}

    def _write_starts(self, j: int, slots, starts, first) -> None:
        """The starts of the tick into the device tables the graph reads (the ragged tick alone has them)."""

    def _split_starts(self, mel, frames, slots, starts):
        """(the sessions' new frames, their counts, {i: the first frame of starting entry i}) of a tick with starts."""
        first = {i: mel[i][:1] for i, s in enumerate(slots) if s in starts}
        return ([m[1:] if i in first else m for i, m in enumerate(mel)], [f - 1 if i in first else f for i, f in enumerate(frames)], first)

    def _tick(self, mel, slots, z, starts):
        st = self.stream
        slots = [st._slot(v) for v in slots]
        if not slots or len(set(slots)) != len(slots):
            raise ValueError('slots must be a non-empty list of distinct slots, got %r' % (slots,))
        mel, frames = self._check_mel(mel, len(slots))          # (frames: every session's count)
        starts = self._check_starts(starts, slots, frames)

        def fresh():
            return [s for s in slots if not st._running[s] and s not in starts and s not in self._started]

        if fresh() and st._pending is not None and st._ticker is not self:
            self._settle()          # (an eager push that only enqueued -- a start that did not fit the capture -- may be what began them)
        if fresh():
            raise ValueError('slot %d is fresh: a session starts with the eager one-frame push (%s keeps the frame and marks the '
                             'slot running) and takes graphed ticks from then on' % (fresh()[0], self.FIRST_PUSH % fresh()[0]))
        whole, first = mel, {}
        if starts:          # a starting session's first frame stands in for a kept frame: the rest are its new frames, like anyone's
            mel, frames, first = self._split_starts(mel, frames, slots, starts)
        if self.sample and z is not None:
            raise ValueError('this graph samples its own noise (sample=True): z is not taken')
        if not self.sample:
            z = self._check_z(z, [f * st.hop for f in frames])
        columns = self._columns(frames)          # (None: the tick does not fit the capture)
        if not self._ready() or columns is None:
            self._settle()
            self.eager_calls += 1
            for s, seed in starts.items():          # (a fresh slot keeps the seed its own reset gave it)
                st.reset(s, seed if seed is not None or st._running[s] else st._seed[s])
            return self._eager(whole, slots=slots, z=z, verify=False)
        j = self._begin_tick()
        self._sync_rows(j, slots, self._write_entries(j, slots, *columns), starts)
        self._write_starts(j, slots, starts, first)
        used, out = self._copy_in(mel, z, frames)          # (used: the leading rows of self.mel the tick's sessions take)
        if self._dirty_rows > used:          # (a filler runs on zeros: nothing of a previous tick's session may reach the range guard)
            per = self.z.shape[0] // self.mel.shape[0]
            self.mel[used:self._dirty_rows].zero_()
            self.z[used * per:self._dirty_rows * per].zero_()
        self._dirty_rows = used
        self._replay(slots)
        return out


class GraphedStream(_TickGraph):
    """The UNIFORM tick -- `n` running sessions x `frames` mel frames, T = frames * hop samples each -- as one graph (_TickGraph;
    StreamingVocoder.graphed): the [n, T] streaming persistent launch of push.

    tick(mel [k, frames, n_mels], slots, z=None) replays it for 1 <= k <= n distinct RUNNING slots and only enqueues; the other n - k
    entries are fillers.  It returns the sessions' next samples [k, T, 1]; sample=False: z [k, T, 1] is the noise.  Ticks may follow
    each other with no synchronisation: the commit kernel flips a session only if both sticky words are clean, and the words are
    sticky, so the committed ticks are a PREFIX of the enqueued ones.  verify() waits, makes the host's view of the sessions equal to
    the device table and returns the number of ticks committed; it raises PwvRangeError / PwvPersistError (with that number as
    `.committed`) where a tick was refused: push the failed chunk again with the eager push and carry on.  While ticks are in flight
    the stream is pending: push / reset / state refuse until verify().  A tick of another frame count runs push(verify=False).

    Refused at construction (PwvError) wherever a flow of an [n, T] push is not the whole-flow persistent streaming launch."""

    ARGS, ENTRY, ENTRY_INTS = _lib.StreamTickArgs, 'pwv_stream_tick', 2
    FIRST_PUSH = 'push(mel[:, :1], slots=[%d])'

    def __init__(self, stream, n: int, frames: int, sample: bool = True, depth: int = 4, warmup: int = 2):
        super().__init__(stream, sample, depth, warmup)
        st, dev = stream, self.device
        self.n, self.frames = n, frames = int(n), int(frames)
        if n < 1 or frames < 1:
            raise ValueError('a graphed tick needs n >= 1 sessions and frames >= 1, got %r / %r' % (n, frames))
        if n > st.n_slots:
            raise ValueError('a graph for %d sessions needs a stream of at least %d slots (this one has %d): the entries a tick does not '
                             'use are fillers on OTHER slots of the stream' % (n, n, st.n_slots))
        self.T = frames * st.hop
        self.mel = torch.zeros((n, frames, st.n_mels), dtype=torch.float32, device=dev)
        self.z = torch.zeros((n, self.T, 1), dtype=torch.float32, device=dev)
        self._chunk = torch.zeros((n, frames + 1, st.n_mels), dtype=torch.float32, device=dev)
        self._start(n)

    def _not_one_launch(self):
        return 'a flow of a %d x %d push is not one persistent streaming launch' % (self.n, self.T)

    def _shape_args(self, ta):
        ta.frames, ta.T = self.frames, self.T

    def _push_args(self):
        return self._chunk, self.z, self._tab, self.T

    def _capture_columns(self):
        return ()

    def _good_warmup(self, log, launches):
        return len(log) == launches and all(self._one_launch(e) for e in log)

    def _check_mel(self, mel, k):
        mel = engine._require_cuda_f32(mel, 'mel')
        if mel.dim() != 3 or mel.shape[0] != k or mel.shape[1] < 1 or mel.shape[2] != self.stream.n_mels:
            raise ValueError('mel must be [%d, f >= 1, %d], got %s' % (k, self.stream.n_mels, tuple(mel.shape)))
        return mel, [int(mel.shape[1])] * k

    def _check_z(self, z, samples):
        if z is None:
            raise ValueError('this graph has no sampler (sample=False): z [%d, %d, 1] is required' % (len(samples), samples[0]))
        z = engine._require_cuda_f32(z, 'z')
        if tuple(z.shape) != (len(samples), samples[0], 1):
            raise ValueError('z must be [%d, %d, 1], got %s' % (len(samples), samples[0], tuple(z.shape)))
        return z

    def _columns(self, frames):
        return () if frames[0] == self.frames and len(frames) <= self.n else None

    def _eager(self, *args, **kw):
        return self.stream.push(*args, **kw)

    def _copy_in(self, mel, z, frames):
        k = len(frames)
        self.mel[:k].copy_(mel, non_blocking=True)
        if z is not None:
            self.z[:k].copy_(z, non_blocking=True)
        return k, self.out[:k]


class GraphedRaggedStream(_TickGraph):
    """The RAGGED tick -- up to `slots` running sessions, every one its own number of frames, `rows` samples in all -- as one graph
    (_TickGraph; StreamingVocoder.graphed_varlen): the packed persistent streaming launch of push_varlen.

    The packed persistent launch is length-agnostic (GraphedPackedVocoder): the layout reaches the kernels only through cu_rows,
    cu_frames and the unit map in device memory, and here the begin kernel writes them from the tick's `entries` = {slot, live, frames}.
    tick(mels, slots, z=None), mels[i] [f_i, n_mels], replays the graph for 1 <= k <= `slots` distinct RUNNING sessions whose frames fit
    (fits()): k < slots adds slots - k fillers on zero mel, the first slots - k - 1 of min_frames frames, the last one the frames that are
    left; with k = slots the frames fill rows / hop exactly.  It returns a RaggedOutput of the sessions' next samples [f_i * hop, 1];
    sample=False: z is the noise, the packed [sum f_i * hop, 1] or a list of [f_i * hop, 1].  A tick that does not fit runs
    push_varlen(verify=False).  Ticks in flight, the committed prefix and verify() are GraphedStream's.

    tick(..., starts={slot: seed}) BEGINS an utterance on the named slots of the tick, fresh or running (a running one is cut off: reset
    and the first push in one step): mels[i] then holds the utterance's opening f_i + 1 frames and the slot yields f_i * hop samples,
    what push_varlen gives a fresh session.  The first frame goes into the `first` table in the kept frame's stead, the begin kernel of the
    graph lets the entry read the stream's zero block and draw from {seed, 0}, the commit kernel sets its counter and seed (include/
    pwv_hip.h, "STARTS"): no verify(), no eager push, the ticks stay pipelined.  The graph always holds the starts instantiations of the
    two kernels; a tick without starts finds an all-zero flag column.

    Refused at construction (PwvError) wherever a flow of such a push is not one packed streaming persistent launch."""

    ARGS, ENTRY, ENTRY_INTS = _lib.StreamTickRaggedArgs, 'pwv_stream_tick_ragged', 4
    FIRST_PUSH = 'push_varlen([mel[:1]], slots=[%d])'
    PACKED = True

    def __init__(self, stream, slots: int, rows: int, sample: bool = True, depth: int = 4, warmup: int = 2):
        super().__init__(stream, sample, depth, warmup)
        st, dev = stream, self.device
        self.hop = hop = st.hop
        self.filler = packed_filler_rows(hop)
        self.min_frames = self.filler // hop
        self.slots, self.rows = n, rows = int(slots), int(rows)
        self._check_capacity(st, n, rows)
        self.in_frames = rows // hop
        self.mel = torch.zeros((self.in_frames, st.n_mels), dtype=torch.float32, device=dev)
        self.z = torch.zeros((rows, 1), dtype=torch.float32, device=dev)
        self._chunk = torch.zeros((self.in_frames + n, st.n_mels), dtype=torch.float32, device=dev)
        # the starts of a tick: {flag, seed bits} and the first frame per entry, the flags through pinned staging like the entries (a
        # stream without a zero block -- its histories are a caller's allocation -- has neither: its ticks take no starts)
        self._starts = self._first = None
        if st._zero_block is not None:
            self._starts = torch.zeros((n, 2), dtype=torch.int64, device=dev)
            self._first = torch.zeros((n, st.n_mels), dtype=torch.float32, device=dev)
            self._starts_host = [torch.zeros((n, 2), dtype=torch.int64).pin_memory() for _ in range(self.depth)]
        self._starts_zero = True                # the device table holds no flag
        self._start(n)

    @staticmethod
    def _check_capacity(st, n: int, rows: int) -> None:
        """The refusals of a capacity of `n` slots and `rows` samples on the stream `st`."""
        hop, filler = st.hop, packed_filler_rows(st.hop)
        if n < 1:
            raise ValueError('a graphed ragged tick needs slots >= 1, got %r' % (n,))
        if rows % hop or rows < n * filler:
            raise _lib.PwvError('GraphedRaggedStream: a capacity of %d slots needs rows a multiple of hop_length (%d) and at least %d '
                                '(%d frames per session), got %d' % (n, hop, n * filler, filler // hop, rows))
        if n > st.n_slots:
            raise _lib.PwvError('GraphedRaggedStream: a capacity of %d slots needs a stream of at least %d slots (this one has %d): the '
                                'entries a tick does not use are fillers on OTHER slots of the stream' % (n, n, st.n_slots))

    def _layout(self, frames):
        """The frame counts of all `slots` entries of a tick: the called sessions', then the fillers'; ValueError if they do not fit."""
        return filler_layout(frames, self.slots, self.in_frames, self.min_frames, ('session', 'frames'))

    def fits(self, frames) -> bool:
        """Can sessions with these frame counts be advanced by one replay of this capture?"""
        return _fits(self._layout, frames)

    def _not_one_launch(self):
        return 'a flow of a ragged push of %d slots / %d rows is not one packed persistent streaming launch' % (self.slots, self.rows)

    def _shape_args(self, ta):
        ta.in_frames, ta.hop, ta.min_frames = self.in_frames, self.hop, self.min_frames
        if self._starts is not None:
            ta.starts, ta.first, ta.zero_block = self._starts.data_ptr(), self._first.data_ptr(), self.stream._zero_block

    def _before_capture(self):
        if not self._starts_zero:          # fillers, warm-up and capture have no starts
            self._starts.zero_()
            self._starts_zero = True
        super()._before_capture()

    def _push_args(self):
        return self._chunk[None], self.z, self._tab, 0, self._geom

    def _capture_columns(self):
        # the layout holds a session of min_frames frames wherever one is admissible (slots >= 2), so StreamingVocoder._enqueue, which
        # sizes nothing else on the host lengths, puts the packed carry launch into the graph whenever a tick can need it
        layout = [self.min_frames] * (self.slots - 1) + [self.in_frames - (self.slots - 1) * self.min_frames]
        self._geom = engine.VarlenGeometry([f * self.hop for f in layout], self.hop, self.device,
                                           tables=(self._cu_rows, self._cu_frames, self._unit_map))
        return (layout,)

    def _good_warmup(self, log, launches):
        return len(log) == 2 * launches and all(a[0] == 'stream_ragged' and a[3] == 'packed' and self._one_launch(b)
                                                for a, b in zip(log[0::2], log[1::2]))

    def _check_mel(self, mels, k):
        if not isinstance(mels, (list, tuple)) or len(mels) != k:
            raise ValueError('mels must be a list of [f, n_mels] tensors, one per slot (%d slots)' % k)
        mels = [engine._require_cuda_f32(m, 'mels[%d]' % i) for i, m in enumerate(mels)]
        for i, m in enumerate(mels):
            if m.dim() != 2 or m.shape[0] < 1 or m.shape[1] != self.stream.n_mels:
                raise ValueError('mels[%d] must be [f >= 1, %d], got %s' % (i, self.stream.n_mels, tuple(m.shape)))
        return mels, [int(m.shape[0]) for m in mels]

    def _check_z(self, z, samples):
        if z is None:
            raise ValueError('this graph has no sampler (sample=False): z, the packed [%d, 1] or one [f_i * %d, 1] per session, is required'
                             % (sum(samples), self.hop))
        if isinstance(z, (list, tuple)):
            if len(z) != len(samples) or any(tuple(getattr(v, 'shape', ())) != (t, 1) for v, t in zip(z, samples)):
                raise ValueError('z must hold one [f_i * %d, 1] piece per session' % self.hop)
            return [engine._require_cuda_f32(v, 'z[%d]' % i) for i, v in enumerate(z)]
        z = engine._require_cuda_f32(z, 'z')
        if tuple(z.shape) != (sum(samples), 1):
            raise ValueError('z must be the packed [%d, 1], got %s' % (sum(samples), tuple(z.shape)))
        return z

    def _columns(self, frames):
        try:
            return (self._layout(frames),)
        except ValueError:
            return None

    def _eager(self, *args, **kw):
        return self.stream.push_varlen(*args, **kw)

    def tick(self, mels, slots, z=None, starts=None):
        """_TickGraph.tick for the frames mels[i] [f_i, n_mels] of the distinct sessions `slots`.  `starts` = {slot: seed}: these slots of
        the tick -- fresh or running -- begin a new utterance with it; mels[i] then holds its opening f_i + 1 frames (f_i >= min_frames),
        the slot yields f_i * hop samples (sample=False: z[i] is [f_i * hop, 1]) and, with sample=True, draws from `seed` at counter 0
        (None: the seed the slot's reset was given, else one from the OS -- push_varlen's rule).  A fresh slot that `starts` does not
        name is refused as ever.  A tick with starts that does not fit the capture, or one during a suspension, settles what is in
        flight and runs reset(slot, seed) and push_varlen(verify=False)."""
        return self._tick(mels, slots, z, starts)

    def _check_starts(self, starts, slots, frames) -> dict:
        if starts is None:
            return {}
        if not isinstance(starts, dict):
            raise ValueError('starts must be a dict {slot: seed or None}, got %r' % (starts,))
        st, out = self.stream, {}
        for k, v in starts.items():
            s = st._slot(k)
            if s not in slots:
                raise ValueError('starts names slot %d, which is not among the slots of this tick (%r): a seed goes with a slot that '
                                 'starts in it' % (s, slots))
            out[s] = None if v is None else st._check_seed(v)
            f = frames[slots.index(s)]
            if f < self.min_frames + 1:
                raise ValueError('slot %d starts an utterance with %d frames: it needs its first frame and at least %d more (%d in all; '
                                 'a shorter start is the eager push_varlen\'s)' % (s, f, self.min_frames, self.min_frames + 1))
        if out and self._starts is None:
            raise _lib.PwvError('GraphedRaggedStream: this stream has no zero block (its histories are a caller\'s allocation, '
                                'hist_alloc): its graphed ticks take no starts')
        return out

    def _write_starts(self, j, slots, starts, first):
        if self._starts is None or (not starts and self._starts_zero):
            return          # (the device table holds an all-zero flag column already)
        st, staged = self.stream, self._starts_host[j]
        buf = staged.numpy()
        buf[:] = 0
        for i, s in enumerate(slots):
            if s not in starts:
                continue
            seed = starts[s]
            if seed is None and not st._running[s] and s not in self._started:
                seed = st._seed[s]          # push_varlen's rule: a fresh slot has the seed of its reset
            self._starts_log.append((self._window, s, seed))          # (what reset(slot, seed) would keep)
            if seed is None and self.sample:          # ... else one from the OS
                seed = engine.os_seed()
            buf[i, 0], buf[i, 1] = 1, engine.as_int64_bits(seed or 0)
            if first[i] is not None:          # (None: a kernel of the graph writes the row -- the live tick)
                self._first[i:i + 1].copy_(first[i], non_blocking=True)
            self._started.add(s)
        self._starts.copy_(staged, non_blocking=True)
        self._starts_zero = not starts

    def _copy_in(self, mels, z, frames):
        real = sum(frames)
        torch.cat(mels, out=self.mel[:real])
        if isinstance(z, list):
            torch.cat(z, out=self.z[:real * self.hop])
        elif z is not None:
            self.z[:real * self.hop].copy_(z, non_blocking=True)
        return real, RaggedOutput(self.out[:real * self.hop], [f * self.hop for f in frames])


class GraphedLiveStream(GraphedRaggedStream):
    """The LIVE tick -- wav chunks in, the sessions' next samples out -- as one graph (StreamingVocoder.graphed_live; DESIGN.md section 9,
    "Graph replay of a live tick"): the ragged tick of GraphedRaggedStream with the streaming mel front-end in front of it and the
    front-end's commit behind it (include/pwv_hip_live_tick.h):

        mel tick kernel (records + front-end session table -> the frames, straight into the ragged tick's mel and first rows; carries)  ->
        the ragged tick (begin, sampler, unit map, the push, commit)  ->  front-end commit

    Slot k of the StreamingMel `fe` and slot k of the stream are ONE session.  tick(chunks, slots, starts=, ends=, z=) gives session
    slots[i] its next samples chunks[i] [n_i] and returns a RaggedOutput of [f_i * hop, 1] pieces, f_i the frames that became ready
    (frames_ready: host arithmetic; possibly none).  `starts` = {slot: seed or None}: the slot begins an utterance with this chunk (the
    front-end's reset; the vocoder session starts, as by GraphedRaggedStream.tick(starts=), in the first tick in which the utterance has a
    frame -- the seed is remembered until then -- and that tick yields (frames - 1) * hop samples).  `ends` = [slot, ...]: the utterance
    ends with this chunk (n_i = 0 allowed): the tick emits every frame that is left, the right reflection taken at the length received.
    Both halves are committed or refused together on the device; verify() is GraphedRaggedStream's and makes the front-end's view of the
    sessions stand behind the committed prefix as well; it raises the PwvError naming top_db for the slots that went over the limit.

    `slots` and `rows` are graphed_varlen's capacity; the wav buffer holds rows + slots * (n_fft / 2 + hop) samples.  Where the stream has
    more slots than `slots` (and the rows hold one filler more) the capture has one entry more than sessions, so that a tick of all
    `slots` sessions leaves its remaining frames to a filler; else such a tick has to fill the rows exactly, as in graphed_varlen.

    A tick runs the eager sequence fe.push / fe.finish / push_varlen(verify=False) instead (eager_calls; same bits) where it does not fit
    the capture (more slots, samples or frames than the capacity, fewer frames than min_frames in a session, no session with a frame),
    during a suspension of the persistent launches, or where a vocoder start has fewer than min_frames + 1 frames."""

    def __init__(self, stream, fe, slots: int, rows: int, sample: bool = True, depth: int = 4, warmup: int = 2):
        for name, a, b in (('slots', fe.n_slots, stream.n_slots), ('hop_length', fe.hop, stream.hop), ('n_mels', fe.n_mels, stream.n_mels)):
            if a != b:
                raise _lib.PwvError('GraphedLiveStream: the front-end and the stream disagree on %s (%d against %d): slot k of both is one '
                                    'session' % (name, a, b))
        if stream._zero_block is None:
            raise _lib.PwvError('GraphedLiveStream: this stream has no zero block (its histories are a caller\'s allocation, hist_alloc): '
                                'its graphed ticks take no starts')
        self.fe = fe
        self.sessions, rows = int(slots), int(rows)
        self._check_capacity(stream, self.sessions, rows)
        # one entry more than sessions wherever the stream has a slot and the rows a filler for it: a tick of all `slots` sessions then
        # leaves its remaining frames to a filler, where the ragged tick would have to fill the rows exactly
        spare = self.sessions < stream.n_slots and rows >= (self.sessions + 1) * packed_filler_rows(stream.hop)
        super().__init__(stream, self.sessions + (1 if spare else 0), rows, sample=sample, depth=depth, warmup=warmup)

    def _start(self, n: int):
        fe, dev = self.fe, self.device
        self.wav_cap = self.rows + self.sessions * (fe.n_fft // 2 + fe.hop)
        self._wav = torch.zeros((self.wav_cap,), dtype=torch.float32, device=dev)
        self._rec = torch.zeros((n, _lib.LIVE_TICK_REC), dtype=torch.int64, device=dev)
        self._scratch = torch.full((n,), -(1 << 31), dtype=torch.int32, device=dev)
        self._rec_host = [torch.zeros((n, _lib.LIVE_TICK_REC), dtype=torch.int64).pin_memory() for _ in range(self.depth)]
        self._fe_rows_host = [torch.zeros((n, 4), dtype=torch.int64).pin_memory() for _ in range(self.depth)]
        self._rec_zero = True                   # the device table holds no active record
        self._fe_view = {}                      # slot -> (received, emitted) behind the ticks in flight
        self._seed_wait = {}                    # slot -> the seed of an utterance that has begun and has no frame yet
        self._undo = []                         # per graphed tick since the last verify(): what it changed of _seed_wait
        self._eager_undo = None                 # the front-end sessions in front of an eager tick that only enqueued
        self._ctx = None
        super()._start(n)

    def _live_args(self):
        from .audio_frontend import AMIN, TOP_DB
        fe, la = self.fe, _lib.LiveTickArgs()
        la.wav, la.window, la.mel_basis = self._wav.data_ptr(), fe._window.data_ptr(), fe._basis.data_ptr()
        la.mel, la.first = self.mel.data_ptr(), self._first.data_ptr()
        la.state, la.max_key, la.scratch, la.sess = fe._state.data_ptr(), fe._max.data_ptr(), self._scratch.data_ptr(), fe._sess.data_ptr()
        la.rec, la.rec_host, la.words = self._rec.data_ptr(), None, self._words.addr
        la.wav_cap, la.mel_rows = self.wav_cap, self.in_frames
        la.N, la.n_slots, la.n_first, la.n_fft, la.hop, la.n_mels = self._n, fe.n_slots, self._n, fe.n_fft, fe.hop, fe.n_mels
        la.amin, la.max_db, la.min_db, la.limit_db = AMIN, fe.max_db, fe.min_db, fe.min_db + TOP_DB
        return la

    def _before_capture(self):
        if not self._rec_zero:          # warm-up and capture have no record: the front-end's sessions are not touched
            self._rec.zero_()
            self._rec_zero = True
        super()._before_capture()

    def _enqueue(self):
        lib, la = _lib.lib(), self._live_args()
        _lib.check(lib.pwv_live_tick_mel(ctypes.byref(la), engine._stream()), 'pwv_live_tick_mel')
        out = super()._enqueue()
        _lib.check(lib.pwv_live_tick_commit(ctypes.byref(la), engine._stream()), 'pwv_live_tick_commit')
        return out

    # -- the hooks of _TickGraph._tick: the frames are counts here, a kernel of the graph writes them ------------------------------------
    def _check_mel(self, counts, k):
        return counts, list(counts)

    def _split_starts(self, mel, frames, slots, starts):
        first = {i: None for i, s in enumerate(slots) if s in starts}
        frames = [f - 1 if i in first else f for i, f in enumerate(frames)]
        return frames, frames, first

    def _begin_tick(self) -> int:
        self._j = super()._begin_tick()
        return self._j

    def _eager(self, whole, slots, z, verify):
        return self._eager_live(self._ctx, reset_vocoder=False)

    def _copy_in(self, mel, z, frames):
        """The front-end half of the tick through pinned staging: the records, the chunks into the wav buffer, the front-end session rows
        where the host's view says the device row differs (an eager push, finish or reset since)."""
        fe, j, c = self.fe, self._j, self._ctx
        buf = self._rec_host[j].numpy()
        buf[:] = 0
        off = row = entry = 0
        undo = {}
        for i, s in enumerate(c['slots']):
            r, n = c['recs'][i], int(c['chunks'][i].shape[0])
            flags = _lib.LIVE_ACTIVE | (_lib.LIVE_START if s in c['starts'] else 0) | (_lib.LIVE_FIRST if c['vstart'][i] else 0)
            part = r.frames >= 1
            buf[i] = (r.carry_first, r.carry_len, off, n, r.first_frame, r.frames, r.final_len, s, flags, row, r.new_carry_first,
                      entry if part else 0)
            off += n
            if part:
                row, entry = row + r.frames - (1 if c['vstart'][i] else 0), entry + 1
        self._rec.copy_(self._rec_host[j], non_blocking=True)
        self._rec_zero = False
        given = [ch for ch in c['chunks'] if ch.shape[0]]
        if given:
            torch.cat(given, out=self._wav[:off])
        rows = self._fe_rows_host[j]
        for i, s in enumerate(c['slots']):
            if s not in self._fe_view:          # (a slot with ticks in flight is the device's)
                want = (fe._gen[s], fe._received[s], fe._emitted[s])
                if fe._sess_host[s] != want:
                    rows[i, 0], rows[i, 1], rows[i, 2] = want
                    fe._sess[s, :3].copy_(rows[i, :3], non_blocking=True)          # (the sticky `over` word stays the device's)
                    fe._sess_host[s] = want
            self._fe_view[s] = (c['recs'][i].received, c['recs'][i].emitted)
            undo[s] = self._seed_wait.get(s, self)          # (self: no entry)
        self._note_seeds(c)
        self._undo.append(undo)
        fe._live = self
        real = sum(frames)
        if isinstance(z, list):
            torch.cat(z, out=self.z[:real * self.hop])
        elif z is not None:
            self.z[:real * self.hop].copy_(z, non_blocking=True)
        return real, RaggedOutput(self.out[:real * self.hop], [f * self.hop for f in frames])

    def _note_seeds(self, c) -> None:
        """The seeds that wait for their utterance's first frame, after the tick `c`."""
        for i, s in enumerate(c['slots']):
            if c['vstart'][i] or c['recs'][i].final_len >= 0:
                self._seed_wait.pop(s, None)
            elif s in c['starts']:
                self._seed_wait[s] = c['starts'][s]

    # -- a tick ------------------------------------------------------------------------------------------------------------------
    def tick(self, chunks, slots, starts=None, ends=None, z=None):
        """Session slots[i] receives its next samples chunks[i], [n_i >= 1] float32 on the GPU (n_i = 0 for a slot in `ends`); see the
        class.  Returns a RaggedOutput of [f_i * hop, 1] views of the graph's output buffer, valid until the next tick.  Enqueue-only."""
        from .audio_frontend import live_record
        st, fe = self.stream, self.fe
        slots = [st._slot(v) for v in slots]
        if not slots or len(set(slots)) != len(slots):
            raise ValueError('slots must be a non-empty list of distinct slots, got %r' % (slots,))
        if not isinstance(chunks, (list, tuple)) or len(chunks) != len(slots):
            raise ValueError('chunks must be a list of [n] tensors, one per slot (%d slots)' % len(slots))
        if starts is not None and not isinstance(starts, dict):
            raise ValueError('starts must be a dict {slot: seed or None}, got %r' % (starts,))
        starts = {st._slot(k): (None if v is None else st._check_seed(v)) for k, v in (starts or {}).items()}
        ends = [st._slot(v) for v in (ends or [])]
        for s in list(starts) + ends:
            if s not in slots:
                raise ValueError('starts / ends name slot %d, which is not among the slots of this tick (%r)' % (s, slots))
        for i, c in enumerate(chunks):
            if not hasattr(c, 'dim') or c.dim() != 1 or (c.shape[0] < 1 and slots[i] not in ends):
                raise ValueError('chunks[%d] must be [n >= 1] (n = 0 only for a slot in ends), got %s' % (i, tuple(getattr(c, 'shape', ()))))
        chunks = [engine._require_cuda_f32(c, 'chunks[%d]' % i) for i, c in enumerate(chunks)]
        if st._pending is not None and st._ticker is not self:
            self._settle()          # an eager tick that only enqueued, or another graph's ticks
        if fe._live is not None and fe._live is not self:
            fe._live.verify()
        recs, vstart = [], []
        for i, s in enumerate(slots):
            received, emitted = (0, 0) if s in starts else self._fe_view.get(s, (fe._received[s], fe._emitted[s]))
            recs.append(live_record(received, emitted, int(chunks[i].shape[0]), s in ends, fe.n_fft, fe.hop))
            vstart.append(emitted == 0 and recs[i].frames >= 1)          # the utterance's first frame: the vocoder side starts
        part = [i for i in range(len(slots)) if recs[i].frames >= 1]
        samples = [(recs[i].frames - (1 if vstart[i] else 0)) * self.hop for i in range(len(slots))]
        if self.sample and z is not None:
            raise ValueError('this graph samples its own noise (sample=True): z is not taken')
        if not self.sample:
            if z is None:
                raise ValueError('this graph has no sampler (sample=False): z, one [f_i * %d, 1] per slot or the packed [%d, 1], is required'
                                 % (self.hop, sum(samples)))
            if not isinstance(z, (list, tuple)):
                z = engine._require_cuda_f32(z, 'z')
                if tuple(z.shape) != (sum(samples), 1):
                    raise ValueError('z must be the packed [%d, 1], got %s' % (sum(samples), tuple(z.shape)))
                z = list(RaggedOutput(z, samples))
            if len(z) != len(slots) or any(tuple(getattr(v, 'shape', ())) != (t, 1) for v, t in zip(z, samples)):
                raise ValueError('z must hold one [f_i * %d, 1] piece per slot: %r samples' % (self.hop, samples))
            z = [engine._require_cuda_f32(z[i], 'z[%d]' % i) for i in part]
        vslots = [slots[i] for i in part]
        vstarts = {slots[i]: (starts[slots[i]] if slots[i] in starts else self._seed_wait.get(slots[i])) for i in part if vstart[i]}
        self._ctx = c = dict(slots=slots, chunks=chunks, starts=starts, ends=ends, recs=recs, vstart=vstart, part=part, z=z,
                             vslots=vslots, vstarts=vstarts, samples=samples)
        short = any(vstart[i] and recs[i].frames < self.min_frames + 1 for i in part)
        fits = (bool(part) and not short and len(slots) <= self.sessions and sum(int(ch.shape[0]) for ch in chunks) <= self.wav_cap
                and self._ready() and self._columns([t // self.hop for t in (samples[i] for i in part)]) is not None)
        if fits:
            out = self._tick([recs[i].frames for i in part], vslots, z, vstarts or None)
        else:
            self._settle()
            self.eager_calls += 1
            out = self._eager_live(c, reset_vocoder=True)
        return RaggedOutput(out.packed, samples)

    def _eager_live(self, c, reset_vocoder: bool):
        """The tick `c` as the eager sequence: reset / push / finish of the front-end, then reset and push_varlen(verify=False) of the
        sessions that have a frame.  What is in flight has been settled."""
        st, fe, slots = self.stream, self.fe, c['slots']
        self._eager_undo = ({s: (fe._gen[s], fe._received[s], fe._emitted[s]) for s in slots}, {s: self._seed_wait.get(s, self) for s in slots})
        for s in c['starts']:
            fe.reset(s)
        fed = [i for i in range(len(slots)) if c['chunks'][i].shape[0]]
        pieces = {i: [] for i in range(len(slots))}
        if fed:
            for i, p in zip(fed, fe.push([c['chunks'][i] for i in fed], slots=[slots[i] for i in fed])):
                pieces[i].append(p)
            fe._note_over([slots[i] for i in fed])
        for s in c['ends']:
            pieces[slots.index(s)].append(fe._launch([s], [None], True)[0])
            fe._note_over([s])
            fe.reset(s)
        self._note_seeds(c)
        if not c['part']:          # nobody has a frame: the vocoder sits the tick out
            self._carry += 1          # (a tick all the same: the next verify() counts it)
            return RaggedOutput(torch.empty((0, 1), dtype=torch.float32, device=self.device), [])
        if reset_vocoder:
            for s, seed in c['vstarts'].items():          # (a fresh slot keeps the seed its own reset gave it)
                st.reset(s, seed if seed is not None or st._running[s] else st._seed[s])
        mels = [pieces[i][0] if len(pieces[i]) == 1 else torch.cat(pieces[i]) for i in c['part']]
        out = st.push_varlen(mels, slots=c['vslots'], z=c['z'] if not self.sample else None, verify=False)
        if st._pending is None:          # (first frames alone: kept at once, nothing enqueued -- a tick all the same)
            self._carry += 1
        return out

    def verify(self) -> int:
        """GraphedRaggedStream.verify(), for both halves: the front-end's received / emitted / generation of the sessions of the ticks in
        flight are read back from its device table -- they stand behind the committed prefix, like the vocoder's --, and a PwvError
        naming top_db is raised for the slots whose utterance went over min_db + top_db since the last verify() (checked when nothing
        else is reported)."""
        from .audio_frontend import TOP_DB
        st, fe = self.stream, self.fe
        mine, carry, err = st._ticker is self, self._carry, None
        try:
            done = super().verify()
        except _lib.PwvError as e:
            if not hasattr(e, 'committed'):
                raise
            err, done = e, e.committed
        table = fe._sess.cpu().tolist()
        if mine:
            for s in self._fe_view:
                gen, received, emitted = int(table[s][0]) & 1, int(table[s][1]), int(table[s][2])
                fe._gen[s], fe._received[s], fe._emitted[s] = gen, received, emitted
                fe._sess_host[s] = (gen, received, emitted)
            for undo in reversed(self._undo[max(done - carry, 0):]):          # the refused ticks changed nothing
                self._restore_seeds(undo)
        elif err is not None and self._eager_undo is not None:          # an eager tick whose push did not commit
            for s, (gen, received, emitted) in self._eager_undo[0].items():
                fe._gen[s], fe._received[s], fe._emitted[s] = gen, received, emitted
            self._restore_seeds(self._eager_undo[1])
        self._fe_view, self._undo, self._eager_undo = {}, [], None
        if fe._live is self:
            fe._live = None
        if err is not None:
            raise err
        over = [s for s in range(fe.n_slots) if table[s][3]]
        if over:
            fe._sess[:, 3].zero_()
            e = _lib.PwvError('GraphedLiveStream: the top_db floor of the one-shot front-end would have been active for slot(s) %s: an '
                              'utterance\'s largest raw dB went over min_db + top_db = %g; its frames are not the one-shot\'s'
                              % (over, fe.min_db + TOP_DB))
            e.committed = done
            raise e
        return done

    def _restore_seeds(self, undo) -> None:
        for s, seed in undo.items():
            if seed is self:
                self._seed_wait.pop(s, None)
            else:
                self._seed_wait[s] = seed
