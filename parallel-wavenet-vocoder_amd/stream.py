"""Streaming generation: audio out while the mel frames are still coming in ("Streaming").

The model is a chain of causal FIR layers: a layer with dilation d needs, besides the chunk it is given, only the last d rows of
its own input from before the chunk.  A StreamingVocoder keeps those rows per layer and session (the HISTORY; layout in
include/pwv_hip.h, "STREAMING"), so a push costs exactly its own rows, and -- every row going through the instructions of the
one-shot per-layer kernels in their order -- the pushes of a session concatenate to ``IAFVocoder(1, L)(None, mel, z=z)`` bit for bit.

State per session: two GENERATIONS of the history block (a push reads one and writes the other; the flip is the commit), the last
mel frame it was given (the first frame of the next chunk: sample t is conditioned on frame (t + hop/2) // hop), its noise seed
and the number of samples emitted.  Its size does not depend on the chunk length.
"""
from __future__ import annotations

import ctypes
from typing import List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _lib, engine
from .hparam import hparam as hp
from .variables import get_default_store, variable_scope


def round32(d: int) -> int:
    return (int(d) + 31) // 32 * 32


class HistoryLayout:
    """Where every history of the model lies inside a block (float offsets): per flow the d0 + 1 scalars of layer 0's input
    (padded to 64 floats), then per net and layer j >= 1 a tile32 buffer of round32(d_j) rows x 64 channels.  `carry` lists every
    history as (offset, rows, floats per row): the table of pwv_stream_carry_f32.  `nets_per_flow`: 2 for the default architecture,
    1 for the shared-net one (one two-output net per flow: one row history per layer).
    skip=True (a stream of a model with use_skip_connection): layer 0 is a plain layer behind the streaming front
    (pwv_iaf_front_stream_f32), so per flow ONE scalar, x[-1] (padded to 64 floats; carry entry (offset, 1, 1)), and per net a row
    history for layer 0 too -- round32(d_0) rows of the causal layer's output -- at row_off[flow][net][0].  The skip sums themselves are
    row-local and keep no history."""

    def __init__(self, dilations: Sequence[Sequence[int]], nets_per_flow: int = 2, skip: bool = False):
        self.scalar_off: List[int] = []
        self.row_off: List[List[List[int]]] = []       # [flow][net][layer] (layer 0: unused, -1, unless skip)
        self.carry: List[tuple] = []
        off = 0
        for dil in dilations:
            scalars = 1 if skip else int(dil[0]) + 1
            self.scalar_off.append(off)
            self.carry.append((off, scalars, 1))
            off += (scalars + 63) // 64 * 64
            per_net = []
            for _ in range(nets_per_flow):
                offs = [] if skip else [-1]
                for d in (dil if skip else dil[1:]):
                    offs.append(off)
                    self.carry.append((off, int(d), 64))
                    off += round32(d) * 64
                per_net.append(offs)
            self.row_off.append(per_net)
        self.block_floats = off
        self.max_rows = max(rows for _, rows, _ in self.carry)


def advance_history(old: np.ndarray, chunk: np.ndarray) -> np.ndarray:
    """(numpy restatement, tests) The history of a layer after a chunk: the last len(old) rows of old ++ chunk."""
    return np.concatenate([old, chunk])[len(chunk):]


def history_sources(length: int, T: int):
    """(numpy restatement of the kernels' index arithmetic, tests) For a history of `length` rows and a chunk of T rows: where every
    row k of the NEXT history comes from -- ('carry', k + T) = row k + T of the old history (moved by the carry launch, k < length - T)
    or ('chunk', t) = the chunk's row t, stored by the layer launch at k = t + length - T (t >= T - length)."""
    src = {}
    for k in range(max(length - T, 0)):
        src[k] = ('carry', k + T)
    for t in range(T):
        k = t + length - T
        if k >= 0:
            assert k not in src
            src[k] = ('chunk', t)
    return [src[k] for k in range(length)]


def push_samples(frames: int, fresh: bool, hop: int) -> int:
    """Samples a push of `frames` frames yields: a fresh session keeps its last frame back ((f - 1) * hop), a running one has the
    kept frame in front (f * hop)."""
    return (frames - (1 if fresh else 0)) * hop


class RaggedPlan(NamedTuple):
    """ragged_plan: the bookkeeping of one push_varlen that needs no device."""
    samples: List[int]       # T_i per session of the call
    launch: List[int]        # the sessions (indices into the call) that take part in the launches: T_i > 0, in call order
    cu_rows: List[int]       # prefix sums of T_i over `launch` (len(launch) + 1 entries): session launch[k] holds rows cu_rows[k] .. cu_rows[k+1]-1
    cu_frames: List[int]     # ... and of its T_i / hop + 1 frames in the packed mel (a running session: the kept frame + its f_i, a fresh one: its f_i)


def ragged_plan(frames: Sequence[int], fresh: Sequence[bool], hop: int) -> RaggedPlan:
    """What a push of frames[i] >= 1 mel frames to session i (fresh[i]: no frame kept yet) comes to: T_i = push_samples(frames[i],
    fresh[i], hop) samples each; the sessions with T_i > 0 form the packed launch, session k of it with T / hop + 1 frames -- the
    packed layout's t_mel = len / hop + 1.  A fresh session given one frame has T = 0: it is committed (its frame kept) and launches
    nothing."""
    if len(frames) != len(fresh):
        raise ValueError('%d frame counts for %d sessions' % (len(frames), len(fresh)))
    for f in frames:
        if int(f) < 1:
            raise ValueError('every session of a push needs at least one frame, got %r' % (f,))
    samples = [push_samples(int(f), bool(fr), hop) for f, fr in zip(frames, fresh)]
    launch = [i for i, t in enumerate(samples) if t > 0]
    if not launch:
        return RaggedPlan(samples, launch, [0], [0])
    layout = engine.PackedLayout([samples[i] for i in launch], hop)
    return RaggedPlan(samples, launch, layout.cu_rows_host, layout.cu_frames_host)


def _as_ragged_tick(entries, mel):
    """A uniform tick as the ragged tick it is: entries {slot, live} x mel [N, f, n_mels] -> entries {slot, live, f, 0}, mel [N * f, n_mels]
    and min_frames = f (no count needs the clamp; in_frames = N * f)."""
    entries, mel = np.asarray(entries, np.int32).reshape(-1, 2), np.asarray(mel, np.float32)
    n, f = mel.shape[:2]
    wide = np.concatenate([entries, np.full((n, 1), f, np.int32), np.zeros((n, 1), np.int32)], axis=1)
    return wide, mel.reshape(n * f, mel.shape[2]), f


def tick_begin_tables(sess, kept, entries, mel, hop: int, sample: bool = True):
    """(numpy restatement of stream_tick_begin_kernel, csrc/pwv_stream_tick.hip; tests, and the definition of the tables)  The tables of
    ragged_tick_begin_tables for the tick's `entries` (int32 [N, 2] = {slot, live}) and its mel [N, f, n_mels], every session f frames:
    (slot_tab int32 [N, 2], streams int64 [N, 2] = {seed, emitted}, cu_rows int32 [N + 1] = i * f * hop, frames float32 [N, f + 1, n_mels])
    -- what push builds on the host for the same sessions; there is no cu_frames.  sample=False (the tick has no sampler): streams and
    cu_rows go together, both None."""
    wide, flat, f = _as_ragged_tick(entries, mel)
    slot_tab, streams, cu_rows, _, chunk = ragged_tick_begin_tables(sess, kept, wide, flat, hop, f, sample=sample)
    return slot_tab, streams, cu_rows if sample else None, chunk.reshape(len(wide), f + 1, flat.shape[1])


def tick_commit(sess, kept, entries, mel, T: int, words):
    """(numpy restatement of stream_tick_commit_kernel)  ragged_tick_commit for the uniform tick of T = f * hop samples per session:
    (sess, kept, committed) after the tick's last node.  Returns copies."""
    wide, flat, f = _as_ragged_tick(entries, mel)
    if int(T) % f:
        raise ValueError('T = %d samples are no whole number of samples for each of %d frames' % (T, f))
    return ragged_tick_commit(sess, kept, wide, flat, int(T) // f, f, words)


def ragged_tick_counts(entries, in_frames: int, min_frames: int):
    """(numpy restatement of ragged_prefix, csrc/pwv_stream_tick.hip)  cu_in int64 [N + 1]: the prefix sums of the frame counts as the
    device reads them from `entries` (int32 [N, 4] = {slot, live, frames, 0}) at a capacity of `in_frames` frames -- every count
    clamped to min_frames .. what leaves min_frames for each entry behind it, the last entry the remainder."""
    entries = np.asarray(entries, np.int32).reshape(-1, 4)
    n = entries.shape[0]
    if n < 1 or min_frames < 1 or in_frames < n * min_frames:
        raise ValueError('%d entries of at least %d frames do not fit %d frames' % (n, min_frames, in_frames))
    cu = np.zeros((n + 1,), np.int64)
    for i in range(n - 1):
        most = in_frames - int(cu[i]) - (n - 1 - i) * min_frames
        cu[i + 1] = cu[i] + min(max(int(entries[i, 2]), min_frames), most)
    cu[n] = in_frames
    return cu


def ragged_tick_starting(entries, starts, n_slots: int):
    """(numpy restatement of tick_starting, csrc/pwv_stream_tick.hip)  bool [N]: the entries that START an utterance in this tick -- the flag
    of `starts` (int64 [N, 2] = {flag, seed bits}; None: nobody starts) is set and the entry is no filler (live, slot in range)."""
    entries = np.asarray(entries, np.int32).reshape(-1, 4)
    if starts is None:
        return np.zeros((entries.shape[0],), bool)
    starts = np.asarray(starts, np.int64).reshape(-1, 2)
    return (starts[:, 0] != 0) & (entries[:, 1] != 0) & (entries[:, 0] >= 0) & (entries[:, 0] < int(n_slots))


def ragged_tick_begin_tables(sess, kept, entries, mel, hop: int, min_frames: int, touched: Optional[dict] = None, sample: bool = True,
                             starts=None, first=None, zero_block: Optional[int] = None):
    """(numpy restatement of stream_tick_ragged_begin_kernel; tests, and the definition of the tables)  From the device session table
    `sess` (int64 [n_slots, 4]), the kept frames `kept` [n_slots, n_mels], the tick's `entries` (int32 [N, 4] = {slot, live, frames, 0})
    and its mel [in_frames, n_mels] (the sessions' new frames in entry order): (slot_tab int32 [N, 2], streams int64 [N, 2] = {seed,
    emitted}, cu_rows int32 [N + 1], cu_frames int32 [N + 1], chunk float32 [in_frames + N, n_mels]) -- what push_varlen builds on the
    host for the same running sessions.  `live` plays no part here: a filler reads and writes like any other entry.  sample=False (the
    tick has no sampler, `streams` NULL): streams is None.  `touched` (tests): a dict that receives, per array name, every index the
    restatement reads or writes.
    `starts` (int64 [N, 2] = {flag, seed bits}), `first` (float32 [N, n_mels]) and `zero_block`: stream_tick_starts_begin_kernel.  An entry
    that starts (ragged_tick_starting) reads `zero_block`, draws from {its seed, 0} and has first[i] where the kept frame would stand."""
    sess, kept, mel = np.asarray(sess, np.int64), np.asarray(kept, np.float32), np.asarray(mel, np.float32)
    entries = np.asarray(entries, np.int32).reshape(-1, 4)
    n, in_frames = entries.shape[0], mel.shape[0]
    starting = ragged_tick_starting(entries, starts, sess.shape[0])
    if starts is not None:
        starts, first = np.asarray(starts, np.int64).reshape(-1, 2), np.asarray(first, np.float32)
        if zero_block is None or int(zero_block) < 2 * sess.shape[0]:
            raise ValueError('zero_block must be >= 2 * n_slots = %d (no session\'s block), got %r' % (2 * sess.shape[0], zero_block))
    cu = ragged_tick_counts(entries, in_frames, int(min_frames))
    slots = np.where((entries[:, 0] >= 0) & (entries[:, 0] < sess.shape[0]), entries[:, 0], 0)      # (out of range: a filler of slot 0)
    g = sess[slots, 0] & 1
    slot_tab = np.stack([2 * slots + g, 2 * slots + 1 - g], axis=1).astype(np.int32)
    streams = np.stack([sess[slots, 2], sess[slots, 1]], axis=1).astype(np.int64) if sample else None
    if starting.any():
        slot_tab[starting, 0] = int(zero_block)
        if sample:
            streams[starting, 0], streams[starting, 1] = starts[starting, 1], 0
    cu_rows = (cu * int(hop)).astype(np.int32)
    cu_frames = (cu + np.arange(n + 1)).astype(np.int32)
    chunk = np.zeros((in_frames + n, mel.shape[1]), np.float32)
    seen = {'sess': [], 'kept': [], 'mel': [], 'chunk': []} if touched is None else touched
    for name in ('sess', 'kept', 'mel', 'chunk'):
        seen.setdefault(name, [])
    written = np.zeros((in_frames + n,), bool)
    for i in range(n):
        s, at = int(slots[i]), int(cu_frames[i])
        seen['sess'].append(s), seen['chunk'].append(at)
        if starting[i]:
            seen.setdefault('first', []).append(i)
            chunk[at] = first[i]
        else:
            seen['kept'].append(s)
            chunk[at] = kept[s]
        written[at] = True
        for f in range(int(cu[i + 1] - cu[i])):
            seen['mel'].append(int(cu[i]) + f), seen['chunk'].append(at + 1 + f)
            chunk[at + 1 + f] = mel[int(cu[i]) + f]
            written[at + 1 + f] = True
    assert bool(written.all())          # the N sessions tile the chunk
    return slot_tab, streams, cu_rows, cu_frames, chunk


def ragged_tick_commit(sess, kept, entries, mel, hop: int, min_frames: int, words, touched: Optional[dict] = None, starts=None,
                       first=None, zero_block: Optional[int] = None):
    """(numpy restatement of stream_tick_ragged_commit_kernel)  (sess, kept, committed) after the tick's last node: with both sticky
    `words` (give-up, range) zero every LIVE entry's session flips its generation, has emitted hop * f_i more samples and keeps the
    last of its frames; otherwise -- and for every filler -- nothing changes.  Returns copies.
    `starts` (int64 [N, 2] = {flag, seed bits}): stream_tick_starts_commit_kernel.  A live entry that starts has emitted hop * f_i samples
    in all (set, not added) and its seed is the table's (`first` and `zero_block`, the begin kernel's, are taken and not read)."""
    sess, kept = np.array(sess, np.int64), np.array(kept, np.float32)
    mel = np.asarray(mel, np.float32)
    if int(words[0]) != 0 or int(words[1]) != 0:
        return sess, kept, False
    entries = np.asarray(entries, np.int32).reshape(-1, 4)
    cu = ragged_tick_counts(entries, mel.shape[0], int(min_frames))
    starting = ragged_tick_starting(entries, starts, sess.shape[0])
    seen = {} if touched is None else touched
    for i, (slot, live) in enumerate(entries[:, :2]):
        if live and 0 <= slot < sess.shape[0]:
            seen.setdefault('sess', []).append(int(slot)), seen.setdefault('kept', []).append(int(slot))
            seen.setdefault('mel', []).append(int(cu[i + 1]) - 1)
            sess[slot, 0] ^= 1
            if starting[i]:
                sess[slot, 1], sess[slot, 2] = 0, np.asarray(starts, np.int64).reshape(-1, 2)[i, 1]
            sess[slot, 1] += int(hop) * int(cu[i + 1] - cu[i])
            kept[slot] = mel[int(cu[i + 1]) - 1]
    return sess, kept, True


class RaggedOutput(list):
    """What StreamingVocoder.push_varlen returns: the [T_i, 1] pieces of the call's sessions (views; empty for a fresh session given one
    frame), with the packed [sum T_i, 1] result as `.packed` (as models.VarlenOutput)."""

    def __init__(self, packed, samples):
        pieces, r = [], 0
        for t in samples:
            pieces.append(packed[r:r + t])
            r += t
        super().__init__(pieces)
        self.packed = packed


class StreamingVocoder(object):
    """IAFVocoder.open_stream(slots): `slots` independent sessions over the model's weights.

        wav = s.push(mel, slots=[0, 3])      # mel [n, f, n_mels] -> wav [n, samples, 1]
        wavs = s.push_varlen([mel_a, mel_b], slots=[1, 2])      # a RAGGED tick: [f_i, n_mels] each, fresh and running mixed -> [T_i, 1] each
        s.reset(3); s.emitted(0); st = s.state(0); s.load_state(1, st)

    New weights in the store (store.version) re-plan the kernels' packed weights at the next push; open sessions KEEP their
    history -- it is activations, not weights (what they then produce is the new weights' continuation of the old context).

    Two architectures stream, on the same routes and with the same contract: the default one (two scalar-input nets per flow) and the
    shared-net one (model.shared_nets: True -- ONE net of two outputs per flow, out = x y[..., 0] + y[..., 1]; every launch then
    carries one net, G = 1, the tail or the fused head two outputs, and the affine reads them interleaved).  A shared-net session keeps
    one row history per layer and flow instead of two (HistoryLayout(dilations, nets_per_flow=1)): at the default dilations (bench/c2)
    2 x 1,737,728 B + 320 B = 3,475,776 B (3.48 MB) per session against 6,949,184 B (6.95 MB) for the default model; state_bytes,
    state and load_state follow the layout, and a state of the other architecture is turned away by its block_floats.

    A third streams on request, ``open_stream(slots, transposed_conv=True)`` under model.cond_upsample_method 'transposed_conv' (the
    reference's test/tran; with or without shared_nets): the three transposed convolutions have kernel width == stride, so sample t of
    the condition depends on mel frame (t + hop/2) // hop alone -- the frame geometry of the 'repeat' streams, kept frame included.  The
    chunk's frames go through the stage GEMMs, the T rows enter every layer per sample (pwv_wavenet_layer_stream_cond_f32), and a flow is
    L layer launches, the head launch and the affine: the persistent launch has no LDS for the condition weights.  push, push_varlen
    (the grouped route), state / load_state, reset, verify and the noise contract are the same; graphed / graphed_varlen / graphed_live
    refuse by name (they capture the persistent launch).  The request under 'repeat' hparams is a PwvError, and so is hop_length != 80.

    A fourth streams on request, ``open_stream(slots, use_skip_connection=True)`` under model.use_skip_connection (bench/skip; with or
    without shared_nets): the skip sum of a sample is row-local, so it has no history -- a chunk accumulates it in a buffer of its own
    and the head launch reads it.  Layer 0 runs, as in the one-shot skip forward, on the rows of the causal front (a streaming front
    that keeps x[-1] per session) and has a row history like every other layer (HistoryLayout(..., skip=True)); a flow is the front, L
    per-layer launches (pwv_wavenet_layer_stream_skip_f32), the head launch and the affine.  push, push_varlen (the grouped route),
    state / load_state, reset, verify and the noise contract are the same; the graph wrappers refuse by name.  The request under
    hparams without the switch is a PwvError; together with transposed_conv=True it is refused by name.

    Refused with a PwvError that names the reason (nothing is launched): per-sample (transposed-conv) conditioning without that
    request, skip accumulation without that request (a shared-net model with skip connections is refused as a skip model), precision 'f16', any normaliser -- instance
    normalisation's statistics span the whole time axis --, nets outside the fused shape."""

    def __init__(self, model, slots: int, hist_alloc=None, transposed_conv: bool = False, use_skip_connection: bool = False):
        m = hp.model
        why = None
        per_sample, skip = bool(transposed_conv), bool(use_skip_connection)
        if skip and not m.use_skip_connection:
            raise _lib.PwvError("open_stream(use_skip_connection=True) does not match these hparams: model.use_skip_connection is %r"
                                % (m.use_skip_connection,))
        if per_sample and m.cond_upsample_method != 'transposed_conv':
            raise _lib.PwvError("open_stream(transposed_conv=True) does not match these hparams: model.cond_upsample_method is %r"
                                % (m.cond_upsample_method,))
        if 'in' in (m.get('normalize'), m.get('normalize_cond'), m.get('normalize_wavenet')):
            why = "instance normalisation ('in'): its statistics span the whole time axis, a chunk does not have them"
        elif m.cond_upsample_method != 'repeat' and not per_sample:
            why = "per-sample (transposed-conv) conditioning: only 'repeat' conditioning streams (frames enter at frame rate)"
        elif per_sample and int(hp.signal.hop_length) != 80:
            why = 'hop_length %d: the transposed convolutions (strides 4, 4, 5) upsample by 80' % int(hp.signal.hop_length)
        elif per_sample and m.condition_channels != 80:
            why = 'condition_channels %r: the per-sample layer kernels take 80' % (m.condition_channels,)
        elif m.use_skip_connection and not skip:
            why = 'skip accumulation (use_skip_connection: True): the per-layer kernels stream without skip sums only'
        elif skip and per_sample:
            why = ('use_skip_connection=True together with transposed_conv=True: skip accumulation with a per-sample condition has no '
                   'streaming kernels (one or the other)')
        elif (model.precision or engine.DEFAULT_PRECISION) == 'f16':
            why = "precision 'f16': the fp16 storage mode has no streaming kernels ('f16x3' and 'f32' have)"
        elif m.get('normalize') or m.get('normalize_cond') or m.get('normalize_wavenet'):
            why = 'a normaliser (normalize / normalize_cond / normalize_wavenet): outside the fused shape that streams'
        elif not (m.filter_width == 2 and m.residual_channels == 64 and m.dilation_channels == 64 and m.skip_channels == 128
                  and all(len(d) >= 2 for d in m.dilations[:m.n_iaf])):
            why = 'nets outside the fused shape (W = 2, R = D = 64, S = 128, at least 2 layers per net)'
        if why is not None:
            raise _lib.PwvError('open_stream: this model has no streaming form: ' + why)
        if int(slots) < 1:
            raise ValueError('slots must be >= 1, got %r' % (slots,))
        self.model = model
        self.per_sample = per_sample                # a transposed-conv model: the condition enters every layer per sample (_enqueue)
        self.skip = skip                            # a skip-connection model: per-layer launches on per-chunk skip accumulators (_enqueue)
        self.n_slots = int(slots)
        self.hop = int(hp.signal.hop_length)
        self.n_mels = int(hp.signal.n_mels)
        self.layout = HistoryLayout([list(d) for d in m.dilations[:m.n_iaf]], nets_per_flow=1 if m.get('shared_nets', False) else 2,
                                    skip=skip)
        store = model.store or get_default_store()
        self.device = store.device
        # two blocks per slot and, behind them in the same allocation, the ZERO BLOCK: what a session that starts inside a graphed tick
        # reads as its history (include/pwv_hip.h, "STARTS").  Nothing ever writes it -- every write index is 2 s + 1 - g -- and _hist
        # is the view of the sessions' blocks alone.  A caller's hist_alloc (tests) is asked for the sessions' blocks and no more, as it
        # always was: such a stream has no zero block (_zero_block None) and its graphed ticks take no starts.
        blocks, floats = 2 * self.n_slots, self.layout.block_floats
        if hist_alloc is not None:
            self._hist_all, self._zero_block = hist_alloc(blocks * floats).view(blocks, floats), None
        else:
            self._hist_all, self._zero_block = torch.zeros(((blocks + 1) * floats,), dtype=torch.float32, device=self.device).view(blocks + 1, floats), blocks
            self._hist_all[blocks].zero_()
        self._hist = self._hist_all[:blocks]
        self._carry_tab = torch.tensor([[o, r, w, 0] for o, r, w in self.layout.carry], dtype=torch.int32).to(self.device)
        self._kept = torch.zeros((self.n_slots, self.n_mels), dtype=torch.float32, device=self.device)
        self._gen = [0] * self.n_slots              # the generation a push READS
        self._running = [False] * self.n_slots      # a frame is kept (the slot has been pushed to since its last reset)
        self._emitted = [0] * self.n_slots
        self._seed: List[Optional[int]] = [None] * self.n_slots
        self._pending = None                        # the commit of an un-verified push (verify=False / PWV_ASYNC=1)
        # graph replay of a tick (graph.GraphedStream): the sessions as the device sees them -- int64 [n_slots, 4] = {generation read,
        # samples emitted, seed bits, 0} --, per slot what that row is known to hold (None: never written), the graph whose ticks are
        # in flight, and the fresh slots a FILLER entry has written generation 1 - g of (zeros no longer: see _commit)
        self._sess = torch.zeros((self.n_slots, 4), dtype=torch.int64, device=self.device)
        self._sess_host: List[Optional[tuple]] = [None] * self.n_slots
        self._ticker = None
        self._scratch_dirty = [False] * self.n_slots

    # -- bookkeeping -----------------------------------------------------------------------------------------------------
    def _slot(self, slot) -> int:
        s = int(slot)
        if not 0 <= s < self.n_slots:
            raise ValueError('slot %r out of range (0 .. %d)' % (slot, self.n_slots - 1))
        return s

    def _settled(self, what: str) -> None:
        if self._pending is not None:
            raise _lib.PwvError('%s: the previous push was only enqueued (verify=False / PWV_ASYNC=1): call verify() first' % what)

    def emitted(self, slot) -> int:
        """Samples produced so far by `slot` since its last reset."""
        return self._emitted[self._slot(slot)]

    def state_bytes(self, slot=0) -> int:
        """Bytes of device memory one session holds: two generations of the history block and the kept frame."""
        self._slot(slot)
        return 2 * self.layout.block_floats * 4 + self.n_mels * 4

    def reset(self, slot, seed: Optional[int] = None) -> None:
        """`slot` starts a new utterance: zero history (the one-shot left edge), no kept frame, emitted = 0.  `seed`: the noise
        stream of the new utterance (else given at its first push, else drawn from the OS)."""
        self._settled('reset')
        s = self._slot(slot)
        self._hist[2 * s:2 * s + 2].zero_()
        self._gen[s], self._running[s], self._emitted[s], self._scratch_dirty[s] = 0, False, 0, False
        self._seed[s] = None if seed is None else self._check_seed(seed)

    @staticmethod
    def _check_seed(v) -> int:
        return engine.check_u64(v, 'a seed')

    def state(self, slot) -> dict:
        """A copy of the session in `slot` (to park it, or to bring another stream to the same point): load_state takes it."""
        self._settled('state')
        s = self._slot(slot)
        return {'hist': self._hist[2 * s + self._gen[s]].clone(), 'kept': self._kept[s].clone(), 'running': self._running[s],
                'emitted': self._emitted[s], 'seed': self._seed[s], 'block_floats': self.layout.block_floats}

    def load_state(self, slot, st: dict) -> None:
        self._settled('load_state')
        s = self._slot(slot)
        if st['block_floats'] != self.layout.block_floats or st['kept'].numel() != self.n_mels:
            raise ValueError('the state was taken from a model of another shape')
        self._hist[2 * s + self._gen[s]].copy_(st['hist'])
        self._kept[s].copy_(st['kept'])
        self._running[s], self._emitted[s], self._seed[s] = bool(st['running']), int(st['emitted']), st['seed']

    def verify(self) -> None:
        """For pushes that only enqueued (verify=False / PWV_ASYNC=1): wait, raise PwvRangeError if the chunk left the range of the
        split-fp16 arithmetic (the sessions then stand where they stood before the push: push the chunk again on a precision='f32'
        stream of the same state), else advance the sessions."""
        if self._ticker is not None:          # graphed ticks are in flight: their graph settles them (and returns how many committed)
            return self._ticker.verify()
        commit, self._pending = self._pending, None
        engine.verify_enqueued('a streaming push')
        if commit is not None:
            commit()

    def _refuse_graph(self, what: str) -> None:
        """The graph wrappers capture the whole-flow persistent launch, which can host neither a per-sample condition nor skip sums."""
        if self.skip:
            raise _lib.PwvError('%s: skip accumulation (use_skip_connection) streams on per-layer launches only; a graphed tick needs the '
                                'whole-flow persistent launch.  Nothing was captured: push / push_varlen go on as before' % what)
        if self.per_sample:
            raise _lib.PwvError('%s: per-sample (transposed-conv) conditioning streams on per-layer launches only; a graphed tick needs the '
                                'whole-flow persistent launch.  Nothing was captured: push / push_varlen go on as before' % what)

    def graphed(self, n: int, frames: int, sample: bool = True, depth: int = 4, warmup: int = 2):
        """One tick of `n` running sessions x `frames` frames captured into a HIP graph with the commit on the device
        (graph.GraphedStream; DESIGN.md section 9, "Graph replay of a streaming tick")."""
        self._refuse_graph('graphed')
        from .graph import GraphedStream
        return GraphedStream(self, n, frames, sample=sample, depth=depth, warmup=warmup)

    def graphed_varlen(self, slots: int, rows: int, sample: bool = True, depth: int = 4, warmup: int = 2):
        """A RAGGED tick -- up to `slots` running sessions, `rows` samples in all, every session its own frame count -- captured into a HIP
        graph with the frame counts read and the commit made on the device (graph.GraphedRaggedStream; DESIGN.md section 9, "Graph
        replay of a ragged tick").  Its tick(..., starts={slot: seed}) begins utterances inside a tick, on fresh or running slots."""
        self._refuse_graph('graphed_varlen')
        from .graph import GraphedRaggedStream
        return GraphedRaggedStream(self, slots, rows, sample=sample, depth=depth, warmup=warmup)

    def graphed_live(self, fe, slots: int, rows: int, sample: bool = True, depth: int = 4, warmup: int = 2):
        """A LIVE tick -- wav chunks in, wav chunks out -- captured into a HIP graph: the ragged tick of graphed_varlen at a capacity of
        `slots` sessions and `rows` samples with the streaming mel front-end `fe` (audio_frontend.StreamingMel; slot k of both is one
        session) at its head and the front-end's commit at its end (graph.GraphedLiveStream; DESIGN.md section 9, "Graph replay of a
        live tick")."""
        self._refuse_graph('graphed_live')
        from .graph import GraphedLiveStream
        return GraphedLiveStream(self, fe, slots, rows, sample=sample, depth=depth, warmup=warmup)

    # -- a push ----------------------------------------------------------------------------------------------------------
    def _slots(self, slots) -> List[int]:
        return list(range(self.n_slots)) if slots is None else [self._slot(v) for v in slots]

    def _noise_seeds(self, slots, given=None) -> List[int]:
        """The noise seed of every slot of a push that draws its own noise: given[i] where the call brings one, else the one kept
        from the slot's reset or first push, else drawn from the OS."""
        return [given[i] if (given is not None and given[i] is not None) else
                (self._seed[s] if self._seed[s] is not None else engine.os_seed()) for i, s in enumerate(slots)]

    def _commit(self, slots, samples, new_seeds, idx, last):
        """The commit of a push that gave slots[i] samples[i] samples: the generation flip, running, emitted, the seeds (where the
        push drew its own noise) and the kept frames `last` [n, n_mels] (idx: the slots as a device index vector, None = all in order)."""
        def commit():
            for i, s in enumerate(slots):
                if samples[i] == 0 and self._scratch_dirty[s]:
                    # a fresh slot given one frame flips without having written the other generation, which counts on the zeros a
                    # reset left there; a filler entry of a graphed tick has used that block as scratch since: zeros again first
                    self._hist[2 * s + 1 - self._gen[s]].zero_()
                self._scratch_dirty[s] = False
                self._gen[s] ^= 1
                self._running[s] = True
                self._emitted[s] += samples[i]
                if new_seeds is not None:
                    self._seed[s] = new_seeds[i]
            if idx is None:
                self._kept.copy_(last)
            else:
                self._kept.index_copy_(0, idx, last)
        return commit

    def _transact(self, enqueue, commit, verify):
        """The ending of a push: `enqueue(precision)` as a verified call (engine.verified_call), then the commit -- now, or left in
        _pending for verify() where the call only enqueued."""
        out = engine.verified_call(lambda prec: enqueue(prec or self.model.precision), verify)
        verified = ((not engine.ASYNC) if verify is None else bool(verify)) and getattr(engine._tls, 'depth', 0) == 0
        if verified and not torch.cuda.is_current_stream_capturing():
            commit()
        else:
            self._pending = commit
        return out

    def push(self, mel, slots=None, z=None, seeds=None, verify=None):
        """Give the sessions in `slots` (default: all) their next `f` mel frames, mel [n, f, n_mels]; returns their next samples
        [n, samples, 1]: (f - 1) * hop for fresh sessions (the last frame is kept back: the samples around it need the frame after
        it), f * hop afterwards.  All slots of a call get the same f and are in the same state (all fresh or all running).
        ``z`` [n, samples, 1] is the chunk's noise; without it slot i draws from its own counter stream: ``seeds[i]`` (first push
        after a reset; default: from the OS) at counter = samples emitted so far -- what IAFVocoder(1, L) with noise_seed = seeds[i],
        noise_offset = 0 draws.  The model's own noise_offset does not move.

        A push is a transaction and, by default, a verified call (engine.verified_call): the sessions advance only after the chunk
        has completed in range; a chunk that trips the range guard of the split-fp16 arithmetic is rerun in exact fp32 from the same
        pre-chunk state on the same noise (with the usual `pwv:` warning).  verify=False / PWV_ASYNC=1 only enqueue: call verify()
        before the next push."""
        self._settled('push')
        slots = self._slots(slots)
        n = len(slots)
        if n == 0 or len(set(slots)) != n:
            raise ValueError('slots must be a non-empty list of distinct slots, got %r' % (slots,))
        mel = engine._require_cuda_f32(mel, 'mel')
        if mel.dim() != 3 or mel.shape[0] != n or mel.shape[1] < 1 or mel.shape[2] != self.n_mels:
            raise ValueError('mel must be [%d, f >= 1, %d], got %s' % (n, self.n_mels, tuple(mel.shape)))
        running = [self._running[s] for s in slots]
        if any(running) != all(running):
            raise ValueError('the slots of one push must be in one state: all fresh or all running (got %r)' % (dict(zip(slots, running)),))
        fresh = not running[0]
        T = push_samples(mel.shape[1], fresh, self.hop)
        if seeds is not None:
            if z is not None:
                raise ValueError('seeds and z exclude each other: seeds draw the noise, z is the noise')
            if not fresh:
                raise ValueError('seeds are given at a slot\'s first push (or reset): these slots are running')
            seeds = [self._check_seed(v) for v in (seeds.tolist() if hasattr(seeds, 'tolist') else seeds)]
            if len(seeds) != n:
                raise ValueError('seeds holds %d values for %d slots' % (len(seeds), n))
        if z is not None:
            z = engine._require_cuda_f32(z, 'z')
            if tuple(z.shape) != (n, T, 1):
                raise ValueError('z must be [%d, %d, 1], got %s' % (n, T, tuple(z.shape)))
        engine.raise_if_range_flag('an earlier call')
        idx = torch.tensor(slots, dtype=torch.int64).to(self.device) if n != self.n_slots or slots != list(range(n)) else None
        new_seeds = self._noise_seeds(slots, seeds) if z is None else None
        commit = self._commit(slots, [T] * n, new_seeds, idx, mel[:, -1])
        if T == 0:            # one frame to a fresh slot: nothing to generate yet
            commit()
            return torch.empty((n, 0, 1), dtype=torch.float32, device=self.device)
        kept = self._kept if idx is None else self._kept.index_select(0, idx)
        frames = mel if fresh else torch.cat([kept[:, None], mel], dim=1)
        if z is None:
            cu = torch.arange(0, (n + 1) * T, T, dtype=torch.int32).pin_memory().to(self.device, non_blocking=True)
            table = torch.tensor([[engine.as_int64_bits(sd), engine.as_int64_bits(self._emitted[s])] for sd, s in zip(new_seeds, slots)],
                                 dtype=torch.int64).pin_memory().to(self.device, non_blocking=True)
            z = engine.logistic_noise_packed_op(cu, table, n * T).view(n, T, 1)
        # utterance i of the launches reads block 2 s + gen, writes block 2 s + 1 - gen
        tab = torch.tensor([[2 * s + self._gen[s], 2 * s + 1 - self._gen[s]] for s in slots],
                           dtype=torch.int32).pin_memory().to(self.device, non_blocking=True)
        return self._transact(lambda prec: self._enqueue(prec, frames, z, tab, T), commit, verify)

    def _enqueue(self, precision, frames, z, tab, T, geom=None):
        """The chunk's launches on the current stream: the prologue on the chunk's frames [n, f, n_mels], the carry-over of the histories
        the chunk does not push out (one launch, only when T is below the largest history), then per flow engine.run_flow_stream, which
        picks the flow's route ("Routes"): by default ONE persistent streaming launch.  With `geom` the chunk is
        RAGGED: `frames` is the packed mel [1, F, n_mels] (the prologue is per frame, as in the packed one-shot forward), the carry-over
        runs in its packed form (session n's own T_n decides what it moves; skipped when every T_n reaches the largest history) and
        every flow gets the geometry.  Reads the sessions' current generation, writes the other one: may be enqueued again from the
        same state, on any route."""
        model = self.model
        store = model.store or get_default_store()
        lay = self.layout
        rows, shortest = (T, T) if geom is None else (geom.rows, min(geom.lengths))
        sa = _lib.StreamArgs()
        sa.hist_rd = sa.hist_wr = self._hist.data_ptr()
        sa.block_stride, sa.slot_tab = lay.block_floats, tab.data_ptr()
        sa.carry_tab, sa.n_carry = self._carry_tab.data_ptr(), len(lay.carry)
        with variable_scope('iaf_vocoder'):
            flows = model._flows(store, False, precision)
            nets = [net for iaf in flows for net in iaf.nets()]
            with variable_scope('cond'):
                if self.per_sample:
                    # sample t of the cropped condition depends on frame (t + hop/2) // hop alone (kernel width == stride in every stage):
                    # the chunk's T / hop + 1 frames give its T rows.  A ragged chunk runs the stages once over the packed frames,
                    # uncropped, and every group of sessions gathers its own crops (engine.PackedSampleCondition)
                    cond = model._condition(frames, False, strides=[4, 4, 5], store=store, precision=precision, length=rows, crop=geom is None)
                    if geom is not None:
                        cond = engine.PackedSampleCondition(cond.reshape(-1, cond.shape[2]), self.hop)
                else:
                    cond = model._condition(frames, False, strides=[4, 4, 5], store=store, precision=precision, nets=nets, length=rows)
            engine.project_all(nets, cond, precision=precision)
            if shortest < lay.max_rows:
                sa.cu_rows = None if geom is None else geom.cu_rows.data_ptr()      # (packed form: T = 0, every session's own length)
                _lib.check(_lib.lib().pwv_stream_carry_f32(ctypes.byref(sa), tab.shape[0], T, engine._stream()), 'pwv_stream_carry_f32')
                sa.cu_rows = None
            x = z
            for i, iaf in enumerate(flows):
                x = engine.run_flow_stream(iaf.nets(), x, cond, precision, sa, lay.scalar_off[i], lay.row_off[i], geom=geom, slot_tab=tab,
                                           per_sample=self.per_sample, skip=self.skip)
        return x

    # -- a ragged push ---------------------------------------------------------------------------------------------------
    def push_varlen(self, mels, slots=None, z=None, seeds=None, verify=None):
        """A RAGGED tick: session slots[i] (default: all slots, in order) gets the f_i >= 1 frames mels[i] [f_i, n_mels] -- every session
        its own count, fresh and running sessions mixed freely -- in ONE launch per flow.  Session i yields T_i = push_samples(f_i,
        fresh_i, hop) samples; returns a RaggedOutput: the list of [T_i, 1] pieces, views of one packed [sum T_i, 1] tensor (`.packed`).  A
        fresh session given one frame yields an empty piece: its frame is kept, it is running afterwards, and it takes part in no launch.
        ``z``: the noise, packed [sum T_i, 1] or a list of [T_i, 1].  ``seeds``: one entry per slot, an integer for a fresh slot (its
        noise stream; None: the seed given at reset, else drawn from the OS), None for a running one (an integer there is a ValueError,
        as in push).  Without ``z`` slot i draws from its own stream at counter emitted(i).
        Everything push promises holds: a transaction (reads generation g, writes 1 - g, the flip after verification), the range guard's
        rerun in exact fp32 from the same state on the same noise, the rerun of a give-up on the fallback route, verify=False /
        PWV_ASYNC=1 with verify().  A session may be advanced by push and push_varlen alternately: same bits either way."""
        self._settled('push_varlen')
        if not isinstance(mels, (list, tuple)) or not mels:
            raise ValueError('mels must be a non-empty list of [f, n_mels] tensors')
        slots = self._slots(slots)
        n = len(slots)
        if n != len(mels) or len(set(slots)) != n:
            raise ValueError('slots must be distinct, one per mel (%d mels), got %r' % (len(mels), slots))
        for i, m in enumerate(mels):
            if not hasattr(m, 'dim') or m.dim() != 2 or m.shape[0] < 1 or m.shape[1] != self.n_mels:
                raise ValueError('mels[%d] must be [f >= 1, %d], got %s' % (i, self.n_mels, tuple(getattr(m, 'shape', ()))))
        fresh = [not self._running[s] for s in slots]
        plan = ragged_plan([m.shape[0] for m in mels], fresh, self.hop)
        total = plan.cu_rows[-1]
        if seeds is not None:
            if z is not None:
                raise ValueError('seeds and z exclude each other: seeds draw the noise, z is the noise')
            seeds = list(seeds.tolist() if hasattr(seeds, 'tolist') else seeds)
            if len(seeds) != n:
                raise ValueError('seeds holds %d values for %d slots' % (len(seeds), n))
            for i, v in enumerate(seeds):
                if v is not None and not fresh[i]:
                    raise ValueError('seeds[%d]: a seed is given at a slot\'s first push (or reset): slot %d is running' % (i, slots[i]))
            seeds = [None if v is None else self._check_seed(v) for v in seeds]
        if isinstance(z, (list, tuple)):      # (each piece against its own session: a split that only adds up would misassign)
            if len(z) != n:
                raise ValueError('z holds %d pieces for %d sessions' % (len(z), n))
            for i, v in enumerate(z):
                if tuple(getattr(v, 'shape', ())) != (plan.samples[i], 1):
                    raise ValueError('z[%d] must be %s, got %s' % (i, (plan.samples[i], 1), tuple(getattr(v, 'shape', ()))))
            parts = [engine._require_cuda_f32(z[i], 'z[%d]' % i) for i in plan.launch]
            z = (parts[0] if len(parts) == 1 else torch.cat(parts)) if parts else torch.empty((0, 1), dtype=torch.float32, device=self.device)
        elif z is not None:
            z = engine._require_cuda_f32(z, 'z')
            if tuple(z.shape) != (total, 1):
                raise ValueError('z must be the packed [%d, 1], got %s' % (total, tuple(z.shape)))
        mels = [engine._require_cuda_f32(m, 'mels[%d]' % i) for i, m in enumerate(mels)]
        engine.raise_if_range_flag('an earlier call')
        new_seeds = self._noise_seeds(slots, seeds) if z is None else None
        idx = torch.tensor(slots, dtype=torch.int64).pin_memory().to(self.device, non_blocking=True)
        commit = self._commit(slots, plan.samples, new_seeds, idx, torch.stack([m[-1] for m in mels]))
        if not plan.launch:            # one frame each to fresh slots: nothing to generate yet
            commit()
            return RaggedOutput(torch.empty((0, 1), dtype=torch.float32, device=self.device), plan.samples)
        geom = engine.VarlenGeometry([plan.samples[i] for i in plan.launch], self.hop, self.device)
        # the packed mel: a running session brings its kept frame in front of its frames, a fresh one does not
        pieces = []
        for i in plan.launch:
            if not fresh[i]:
                pieces.append(self._kept[slots[i]:slots[i] + 1])
            pieces.append(mels[i])
        mel = (pieces[0] if len(pieces) == 1 else torch.cat(pieces)).unsqueeze(0)
        if z is None:
            z = engine.logistic_noise_packed_op(geom.cu_rows, geom.stream_table([(new_seeds[i], self._emitted[slots[i]]) for i in plan.launch]),
                                                geom.rows)
        # session k of the launches reads block 2 s + gen, writes block 2 s + 1 - gen
        tab = geom._upload([[2 * slots[i] + self._gen[slots[i]], 2 * slots[i] + 1 - self._gen[slots[i]]] for i in plan.launch], torch.int32)
        return RaggedOutput(self._transact(lambda prec: self._enqueue(prec, mel, z, tab, 0, geom), commit, verify), plan.samples)
