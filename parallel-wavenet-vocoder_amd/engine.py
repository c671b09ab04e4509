"""Host-side orchestration of the HIP kernels for one or two WaveNets evaluated side by side.

This is plumbing: it owns no arithmetic.  It packs TF-layout weights once per variable-store
version (pwv_pack_*), allocates the ping-pong activation buffers in HBM through torch's caching
allocator, and enqueues the per-layer launches of libpwv_hip.so on torch's current HIP stream.

Data layout in HBM (float32):
  residual stream   2 x (N*T rows x 64) per net in the "tile32" layout of include/pwv_hip.h (blocks of 32 rows
                    stored [16 channel quads][32 rows][4]: every wave-level load/store is 1 KB contiguous);
                    ping-pong: a layer reads x[t], x[t-d] and writes out[t].  fp16 blocks with precision 'f16'.
  projection P      [N*t_mel, 128*L] per net: relu(mel@dense) @ [gc_filter‖gc_gate] + biases for
                    all L layers at FRAME rate (hoisted: modules.py:216-228 are the same dot
                    products for all 80 samples of a frame), columns in the kernel's order
  net output        [N, T, Q]
"""
from __future__ import annotations

import ctypes
import numbers
import os
import threading
import weakref
from ctypes import c_void_p
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import StackArgs, check

# 'f32'  : v_mfma_f32_32x32x2_f32, exact fp32 fma chains (157 TFLOP/s class)
# 'f16x3': 3-term split-fp16 MFMA with fp32 accumulation (w*x ~= wh*xh + wh*xl + wl*xh, ~22-bit
#          mantissa products): same measured accuracy vs fp64 as 'f32' (~3e-6 on the full model,
#          bar 2e-5), 5.3x fewer matrix-pipe cycles.  Default; PWV_PRECISION overrides.
# 'f16'  : BUILD EXTENSION (BASELINE.json config 5; the reference is fp32 only): fp16 residual stream in HBM,
#          one fp16 MFMA product, fp32 accumulate.  ~1e-3 of the fp32 result -- never the default, never the
#          headline benchmark; tolerance stated in tests/test_gpu_f16.py.
PRECISIONS = {'f32': _lib.PREC_F32, 'f16x3': _lib.PREC_F16X3, 'f16': _lib.PREC_F16}
DEFAULT_PRECISION = os.environ.get('PWV_PRECISION', 'f16x3')

# When a list, run_nets brackets every fused-layer launch with HIP events recorded on the
# launch stream and appends (tag, start_event, end_event): bench.py's live kernel timing.
EVENT_LOG = None

# Environment knobs (seven, all read once at import into the module attributes a forward reads): PWV_PRECISION (above), PWV_PERSIST,
# PWV_TWO_STREAMS, PWV_FOLD_FIRST, PWV_FUSE_TAIL, PWV_ASYNC, PWV_FUSE_PROLOGUE.  Everything else below is a module attribute that
# tests / tools set directly.  launch_knobs() lists every attribute that decides which launches a forward enqueues.
#
# The scalar and shifter nets of a flow are independent dependency chains.  On the per-layer path (PWV_PERSIST=0, or a shape
# the persistent launch does not cover) TWO_STREAMS gives each chain its own HIP stream and half of the CUs per launch
# (G = 1), so one chain's launch gap / tail is covered by the other's bulk; otherwise both nets share one G = 2 launch.
TWO_STREAMS = os.environ.get('PWV_TWO_STREAMS', '1') != '0'
# layer 0 rebuilds the causal layer from the flow's scalar input / the head runs behind the last layer (tests switch them
# off to check the fused forms bit for bit against the separate launches)
FUSE_FIRST = True
FUSE_HEAD = True
# the net's last layer + head -- and the flow's affine -- run INSIDE the persistent launch (pwv_persist_args.tail_*, split-fp16 path):
# a flow is one launch instead of three.  Tests switch it off to check the fused form bit for bit against the separate launches.
FUSE_TAIL = os.environ.get('PWV_FUSE_TAIL', '1') != '0'      # (PWV_FUSE_TAIL=0: A/B runs)
HOIST_P = True               # one projection GEMM per forward (project_all); False: every net projects for itself (cross-check in tests)
# PWV_FOLD_FIRST=0: layer 0 runs its filter|gate GEMM on the rebuilt causal-layer rows (eight MFMA k-steps) instead of on the
# four scalars they are a function of (one k-step); default: folded.  The only knob that changes bits (measured in HISTORY.md section 4, K2).
FOLD_FIRST = os.environ.get('PWV_FOLD_FIRST', '1') != '0'
# The residual layers of a stack as ONE persistent launch (csrc/pwv_stack_persist.hip, bit-identical results) instead of one
# launch per layer.  PWV_PERSIST = 0 | 1 | auto (default: wherever the library supports the shape; '1' forces it).
_pm = os.environ.get('PWV_PERSIST', 'auto')
PERSIST = {'0': False, '1': True}.get(_pm, 'auto')
PERSIST_AUTO_MAX_ROWS = 750000     # rows (N*T) per launch up to which 'auto' takes the persistent launch: measured on C3's model, same box, per-layer vs
                                   # persistent -- round 4: 160000 rows -5.5 %, 320000 -3.5 %, 480000 -0.6 %, 640000 +0.3 %, 960000 +1.5 % per step; round 5, with
                                   # the last layer + head + affine riding in the launch: 480000 -0.5 %, 640000 -0.6 %, 960000 +1.1 % (profiles/r05_ab_experiments.md r05_i)
PERSIST_MIN_UNITS = 0         # short inputs: fewer workgroups rather than ranges below this many units (0 = the library's default, 4)
PERSIST_MAX_LAYERS = 32       # longest run of layers in one persistent launch (a stack is cut into equal runs that hand the ring on)
# PWV_ASYNC=1: the reference-shaped calls (IAFVocoder / WaveNet / LinearIAFLayer __call__) only ENQUEUE, like the C ABI; the
# caller then owns IAFVocoder.verify() / engine.verify_enqueued().  Default: a call returns only after its own launches
# have completed and the library's sticky words (range guard, persistent give-up) are clean -- or it has rerun itself on
# the path that is (per-layer launches / exact fp32).  bench.py and graph.py opt out per call (verify=False) and verify for
# themselves; generate() passes verify=True, which outranks this knob: nothing unverified is ever written to disk.
ASYNC = os.environ.get('PWV_ASYNC', '0') == '1'
_persist_ws = {}          # (device, stream) -> zeroed workspace of the persistent launches on that stream
_persist_ws_retired = []  # workspaces a launch that gave up may still be writing to (kept alive, never handed out again)
_side_streams = {}

# ---- the library's two sticky words (pinned host memory, read without a device -> host copy) -----------------------------------
# words[0]: a persistent stack launch gave up (pwv_persist_args.status);  words[1]: an operand left the range of the split-fp16
# arithmetic (the `range_flag` argument of every entry point that checks).  Every THREAD has its own pair per device
# (pwv_status_words_alloc): everything a thread enqueues -- on any stream, eagerly or while capturing a graph -- reports into its
# own words, and its verification reads only those, so two threads serving two streams cannot consume or clear each other's
# flags.  (A captured graph keeps reporting into the words of the thread that captured it: graph.GraphedVocoder remembers them.)
_tls = threading.local()      # .words: {device index: StatusWords};  .depth: nesting of reference-shaped calls (verified_call)


# pinned pairs whose owners (threads, graphs) are gone: handed out again instead of allocated.  No lock: list.pop() / append are
# atomic under the GIL, and a lock would deadlock when the GC collects a StatusWords (__del__) inside another's __init__.
_free_words: List[int] = []


class StatusWords(object):
    """One pinned, mapped pair {give-up word, range word}.  Pairs are POOLED: a serving process that spawns short-lived worker
    threads would otherwise leave one page-granular pinned allocation behind per thread.  A pair goes back to the
    pool when its last owner is collected -- the thread's table (a thread-local) and every GraphedVocoder that captured launches
    carrying it hold references -- and is cleared when it is handed out again.  A launch the dead owner left in flight can still
    write into the recycled pair after that: a stale give-up word costs the next owner one rerun on per-layer launches, a stale
    range word one rerun in exact fp32 -- or, for a caller that does not verify (verify=False, PWV_ASYNC=1), a PwvPersistError /
    PwvRangeError from verify_enqueued().  Never a wrong result."""
    __slots__ = ('addr', '__weakref__')

    def __init__(self):
        try:
            addr = _free_words.pop()
        except IndexError:
            p = c_void_p()
            check(_lib.lib().pwv_status_words_alloc(ctypes.byref(p)), 'pwv_status_words_alloc')
            addr = p.value
        self.addr = addr
        self.persist = 0
        self.range = 0

    def __del__(self):
        try:
            _free_words.append(self.addr)
        except Exception:      # interpreter shutdown
            pass

    def _w(self, k):
        return ctypes.c_int.from_address(self.addr + 4 * k)

    persist = property(lambda self: self._w(0).value, lambda self, v: setattr(self._w(0), 'value', int(v)))
    range = property(lambda self: self._w(1).value, lambda self, v: setattr(self._w(1), 'value', int(v)))


def current_words(device=None) -> StatusWords:
    """This thread's pair of sticky words for `device` (default: the current device); allocated on first use, kept for the life of
    the process (a launch that was handed them may outlive any scope here)."""
    idx = torch.cuda.current_device() if device is None else (device.index if isinstance(device, torch.device) and device.index is not None
                                                               else (device if isinstance(device, int) else torch.cuda.current_device()))
    d = getattr(_tls, 'words', None)
    if d is None:
        d = _tls.words = {}
    w = d.get(idx)
    if w is None:
        w = d[idx] = StatusWords()
    return w


def persist_status_ptr() -> int:
    return current_words().addr


def persist_status(words: Optional[StatusWords] = None) -> int:
    """The sticky give-up word of this thread's persistent stack launches: 0 = every launch that has completed so far ran to its
    end; otherwise a launch gave up and its outputs are invalid."""
    return (words or current_words()).persist


def poke_persist_status(code: int, words: Optional[StatusWords] = None) -> None:
    """(tests / tools) Write the give-up word as a launch that gave up would: a real give-up needs a second process on the GPU."""
    (words or current_words()).persist = code


def clear_persist_status(words: Optional[StatusWords] = None) -> None:
    (words or current_words()).persist = 0


# A give-up means the launch's workgroups were not all resident -- another process held CUs.  That is a condition, not a property of
# this process: the engine SUSPENDS the persistent launches for a number of forwards (per-layer launches: same arithmetic, same
# bits, ~5 % slower), then tries them again; consecutive give-ups double the pause (16, 32, ... 1024 forwards), a forward that
# completes on persistent launches resets it.
PERSIST_RETRY_AFTER = 16
_persist_cooldown = 0
_persist_backoff = PERSIST_RETRY_AFTER


# NOTE the suspension below is PROCESS-wide (one counter for all threads) although the sticky words are per thread: a give-up means
# the chip is shared with somebody, which concerns every thread's launches alike; the other threads' graphs are re-captured
# on the per-layer path at their next call (graph._Captured._stale).
def persist_suspended() -> bool:
    return _persist_cooldown > 0


def suspend_persist() -> None:
    global _persist_cooldown, _persist_backoff
    _persist_cooldown = _persist_backoff
    _persist_backoff = min(2 * _persist_backoff, 1024)
    # the launch that gave up may still have workgroups to start (they see the abort word and leave), and it did not clean up
    # after itself: its workspace is retired, the next persistent launch gets fresh zeros
    _persist_ws_retired.extend(_persist_ws.values())
    del _persist_ws_retired[:-8]
    _persist_ws.clear()


def resume_persist() -> None:
    """(tests / tools) End a suspension now."""
    global _persist_cooldown, _persist_backoff
    _persist_cooldown, _persist_backoff = 0, PERSIST_RETRY_AFTER


def note_forward() -> None:
    """One forward has been enqueued (an outermost reference-shaped call, a graph replay): the suspension counts down."""
    global _persist_cooldown
    if _persist_cooldown > 0:
        _persist_cooldown -= 1


def raise_if_persist_failed(words: Optional[StatusWords] = None) -> None:
    """A give-up of the persistent kernel (its workgroups were not all resident, a poll ran into its bound) suspends the
    persistent launches (suspend_persist) and raises: the caller reruns the forward, which then takes per-layer launches.  The
    range word is cleared with it: whatever consumed the invalid rows may have raised it, and the rerun must not meet it."""
    w = words or current_words()
    code = w.persist
    if code != 0:
        w.persist = 0
        w.range = 0
        suspend_persist()
        raise _lib.PwvPersistError('the persistent stack kernel gave up (code %d); its outputs are invalid -- per-layer launches are used '
                                   'for the next %d forwards, then the persistent launch is tried again; rerun the forward' % (code, _persist_cooldown))


def verify_enqueued(where: str = '', words: Optional[StatusWords] = None) -> None:
    """Wait for everything enqueued on this device and raise PwvPersistError / PwvRangeError if a launch that has completed
    left one of this thread's sticky words raised (what a caller of the enqueue-only forms owes before it reads a result)."""
    torch.cuda.synchronize()
    raise_if_persist_failed(words)
    raise_if_range_flag(where, words)


def verified_call(run, verify: Optional[bool] = None):
    """The contract of the reference-shaped entry points (IAFVocoder / WaveNet / LinearIAFLayer / SharedIAFLayer __call__):
    `run(precision_override)` enqueues the forward and returns its result tensor.  By default the OUTERMOST such call then waits
    for its launches and looks at this thread's two sticky words (pinned host memory: no device -> host copy):
      * a persistent stack launch gave up (its workgroups were not all resident): the engine suspends the persistent launches
        (suspend_persist: per-layer launches -- same arithmetic, same bits -- for a while, then another try) and the forward is rerun;
      * an operand left the range of the split-fp16 arithmetic (the reference computes in fp32, models.py:81-82): the forward
        is rerun with precision 'f32'.
    So `pred = model(wav, mel, is_training=False); pred.cpu()` (generate.py:38,68) yields a correct result or an exception,
    never inf from a silent fp16 overflow.  verify=False (or PWV_ASYNC=1, or a call under stream capture, or a call nested in
    another reference-shaped call) only enqueues; the caller then owns verify_enqueued() / IAFVocoder.verify()."""
    global _persist_backoff
    if verify is None:
        verify = not ASYNC
    depth = getattr(_tls, 'depth', 0)
    if depth == 0:
        note_forward()
    if depth > 0 or not verify or torch.cuda.is_current_stream_capturing():
        _tls.depth = depth + 1
        try:
            return run(None)
        finally:
            _tls.depth = depth
    _tls.depth = 1
    try:
        out = run(None)
        torch.cuda.current_stream().synchronize()
        if persist_status() != 0:
            clear_persist_status()
            clear_range_flag()          # (whatever consumed the invalid rows may have raised it)
            suspend_persist()
            import warnings
            warnings.warn('pwv: a persistent stack launch gave up (its workgroups were not all resident -- another process on this GPU?); '
                          'the forward is rerun on per-layer launches (same arithmetic, same bits), which the next %d forwards use too '
                          'before the persistent launch is tried again' % _persist_cooldown)
            out = run(None)
            torch.cuda.current_stream().synchronize()
            raise_if_persist_failed()
        elif _persist_cooldown == 0:
            _persist_backoff = PERSIST_RETRY_AFTER      # (a forward on persistent launches -- or one that never needed them -- went through)
        if range_flag_raised():
            clear_range_flag()
            import warnings
            warnings.warn("pwv: an input or activation left the exponent range of the split-fp16 arithmetic; the forward is rerun in exact fp32 "
                          "(precision='f32', the reference's arithmetic) on the same noise")
            out = run('f32')
            torch.cuda.current_stream().synchronize()
            raise_if_persist_failed()
            raise_if_range_flag("its rerun in precision 'f32'")
        return out
    finally:
        _tls.depth = 0


def _persist_runs(L: int, first: int = 1) -> List[Tuple[int, int]]:
    """(first layer, count) of the persistent launches that cover the residual layers `first` .. L-2 (first = 0: layer 0
    rebuilds the causal layer from the scalar input inside the launch, pwv_persist_args.x_first)."""
    Lp = L - 1 - first
    nchunks = -(-Lp // max(2, PERSIST_MAX_LAYERS))
    runs, j0 = [], first
    for c in range(nchunks):
        cnt = Lp // nchunks + (1 if c < Lp % nchunks else 0)
        runs.append((j0, cnt))
        j0 += cnt
    if len(runs) > 1 and runs[-1][1] < 2:       # (a run has at least two layers)
        runs[-2:] = [(runs[-2][0], runs[-2][1] + runs[-1][1])]
    return runs


def _persist_launches(G: int, n: int, t: int, dilations, first: int = 1, tail_q: int = 0, prec: int = 0, layer_stride: int = 0,
                      cond_geom=(0, 0, 0)) -> Optional[List[Tuple[int, _lib.PersistArgs]]]:
    """(first layer, pwv_persist_args) of the persistent launches that run layers first .. L-2 (with tail_q > 0: and the last layer +
    head behind the last run), one per run of _persist_runs, with every field but the buffers filled in, workspace_bytes included --
    or None (per-layer launches) where the policy or the library (0 bytes for some run) refuses.  The launch only adds the buffers."""
    L = len(dilations)
    if PERSIST is False or _persist_cooldown > 0 or L < 4:
        return None
    if PERSIST == 'auto' and n * t > PERSIST_AUTO_MAX_ROWS:
        return None
    lib = _lib.lib()
    runs, out, rot = _persist_runs(L, first), [], 0
    for j0, cnt in runs:
        pa = _lib.PersistArgs()
        pa.G, pa.n_layers, pa.N, pa.T = G, cnt, n, t
        pa.dilations = (ctypes.c_int * cnt)(*[int(d) for d in dilations[j0:j0 + cnt]])
        pa.min_units_per_workgroup, pa.precision, pa.packed_layer_stride = PERSIST_MIN_UNITS, prec, layer_stride
        pa.cond_hop, pa.cond_offset, pa.cond_frames = cond_geom
        pa.ring_rotation = rot              # input in buffer (2 + rot) % 3, output in buffer (cnt - 1 + rot) % 3
        rot = (cnt + rot) % 3               # the next run reads this run's output: (2 + rot') % 3 == (cnt - 1 + rot) % 3
        if tail_q > 0 and (j0, cnt) == runs[-1]:      # the tail's own look-back (the LAST dilation) is part of the answer
            pa.tail_q, pa.tail_dilation = tail_q, int(dilations[L - 1])
        pa.workspace_bytes = lib.pwv_persist_workspace_bytes(ctypes.byref(pa))
        if pa.workspace_bytes == 0:         # the library cannot run this shape persistently
            return None
        out.append((j0, pa))
    return out


def _use_persist(G: int, n: int, t: int, dilations, first: int = 1, tail_q: int = 0) -> bool:
    """Can layers first .. L-2 (and, with tail_q > 0, the last layer + head behind the last run) run as persistent launches?"""
    return _persist_launches(G, n, t, dilations, first, tail_q) is not None


PERSIST_ARGS_HOOK = None      # tests: called with the filled-in pwv_persist_args right before every persistent launch


def launch_knobs() -> tuple:
    """Every module attribute that decides WHICH launches a forward enqueues (read by _choose_path, get_plan, the launch helpers and
    the prologue): a graph captured under other values is stale (graph._Captured._stale).  A new such knob goes here."""
    return (PERSIST, persist_suspended(), TWO_STREAMS, FOLD_FIRST, FUSE_FIRST, FUSE_HEAD, FUSE_TAIL, HOIST_P, PERSIST_MAX_LAYERS,
            PERSIST_MIN_UNITS, DEFAULT_PRECISION, FUSE_PROLOGUE, FUSE_PROLOGUE_MAX_OUTPUTS, PERSIST_AUTO_MAX_ROWS)


def _net_streams(device):
    key = (device.type, device.index)
    if key not in _side_streams:
        _side_streams[key] = [torch.cuda.Stream(device=device), torch.cuda.Stream(device=device)]
    return _side_streams[key]


# ---- range guard of the split-fp16 arithmetic (include/pwv_hip.h, "Range guard") -------------------------------
F16_LIMIT = 65000.0          # fp16 max is 65504; stay below the value that rounds up to inf
_range_warned = set()
RANGE_LOG = None             # a list: every run-time check of a split-fp16 forward appends (kind, observed max, limit, pack-time bounds)
                             # -- diagnostics only (range_report): each entry costs a device -> host read


def _log_range(kind: str, x: torch.Tensor, limit: float, bounds=None) -> None:
    if RANGE_LOG is not None:
        RANGE_LOG.append((kind, float(x.abs().max()), float(limit), bounds))


def range_report(forward) -> dict:
    """How far a split-fp16 forward stays from fp16's exponent range, per operand class: runs `forward()` (eager, precision 'f16x3')
    with RANGE_LOG on and returns, per class, the limit the guard derived, the maximum it observed (run-time classes) or bounded
    (pack-time classes), and their quotient -- `range_margin` = the smallest quotient: the factor by which every weight / input of that
    class could grow before the guard (deliberately conservative) would send the forward to the exact-fp32 kernels.
      weights         max |w| after the exp2 scale folding              vs 65000            (pack time)
      residual        sum_i (||dense_i||_1 + |bias_i|) + |h|max bound   vs 65000            (pack time + observed flow input)
      head_operand    ||skip||_1 + |bias| (relu(skip) feeds postprocess1) vs 65000          (pack time)
      flow_input      max |x| entering a flow                           vs x_limit           (run time, checked on the device)
      mel             max |mel|                                         vs mel_limit         (run time, checked on the device)"""
    global RANGE_LOG
    saved, RANGE_LOG = RANGE_LOG, []
    try:
        forward()
        torch.cuda.synchronize()
        log = RANGE_LOG
    finally:
        RANGE_LOG = saved
    classes = {}

    def put(name, limit, observed):
        cur = classes.get(name)
        q = limit / observed if observed > 0 else float('inf')
        if cur is None or q < cur['margin']:
            classes[name] = {'limit': limit, 'observed': observed, 'margin': q}

    for kind, seen, limit, bounds in log:
        put(kind, limit, seen)
        for b in bounds or ():
            put('weights', F16_LIMIT, b['w_max'])
            put('head_operand', F16_LIMIT, b['skip_bound'])
            put('residual', F16_LIMIT, b['res_bound'] + b['c0_max'] + b['c_causal'] * seen)
    return {'classes': classes, 'range_margin': min((c['margin'] for c in classes.values()), default=float('inf'))}


def range_flag_ptr() -> int:
    """Address of this thread's sticky overflow flag (pinned host memory, also valid on the device)."""
    return current_words().addr + 4


def range_flag_raised(words: Optional[StatusWords] = None) -> bool:
    """True once a split-fp16 forward of this thread that has COMPLETED met an out-of-range operand (no synchronisation here)."""
    return (words or current_words()).range != 0


def clear_range_flag(words: Optional[StatusWords] = None) -> None:
    (words or current_words()).range = 0


def raise_if_range_flag(where: str = '', words: Optional[StatusWords] = None) -> None:
    if range_flag_raised(words):
        clear_range_flag(words)
        raise _lib.PwvRangeError("a split-fp16 ('f16x3') forward%s met an activation or input beyond fp16's exponent range "
                                 "(or a non-finite one): its result is not trustworthy -- rerun with precision='f32'"
                                 % (' (%s)' % where if where else ''))


def range_check_op(x: torch.Tensor, limit: float, kind: Optional[str] = 'mel') -> None:
    """Enqueue the check |x| <= limit (and finite) on the current stream; a violation raises the sticky flag."""
    if kind:
        _log_range(kind, x, limit)
    check(_lib.lib().pwv_range_check_f32(_ptr(x), x.numel(), float(limit), range_flag_ptr(), _stream()), 'pwv_range_check_f32')


def _stream() -> c_void_p:
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _require_cuda_f32(t: torch.Tensor, what: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError('%s must be a torch.Tensor' % what)
    if not t.is_cuda:
        raise _lib.PwvError('%s must live on the GPU (cuda device); there is no CPU path' % what)
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


class RepeatedCondition:
    """Frame-rate condition + the 'repeat' upsampling rule (models.py:131-133), kept lazy:
    sample t of the upsampled condition is ``frames[:, (t + offset) // hop, :]``.  WaveNet layers
    project it at frame rate instead of materialising the [N, T, C] tensor."""

    def __init__(self, frames: torch.Tensor, hop: int, offset: int, length: int):
        self.frames = frames          # [N, t_mel, C]
        self.hop, self.offset, self.length = int(hop), int(offset), int(length)
        if (self.length - 1 + self.offset) // self.hop >= frames.shape[1]:
            raise ValueError('length %d needs more than %d frames' % (length, frames.shape[1]))

    @property
    def shape(self):
        return (self.frames.shape[0], self.length, self.frames.shape[2])

    def materialize(self) -> torch.Tensor:
        n, t_mel, c = self.frames.shape
        out = torch.empty((n, self.length, c), dtype=torch.float32, device=self.frames.device)
        check(_lib.lib().pwv_upsample_repeat_f32(_ptr(self.frames), _ptr(out), n, t_mel, c, self.length,
                                                 self.hop, self.offset, _stream()), 'pwv_upsample_repeat_f32')
        return out


# --------------------------------------------------------------------------------------------
# thin op wrappers
# --------------------------------------------------------------------------------------------
def causal_conv_op(value: torch.Tensor, filter_: torch.Tensor, dilation: int) -> torch.Tensor:
    value = _require_cuda_f32(value, 'value')
    filter_ = _require_cuda_f32(filter_, 'filter_')
    if value.dim() != 3 or filter_.dim() != 3 or value.shape[2] != filter_.shape[1]:
        raise ValueError('causal_conv: value [N,T,Cin] / filter [W,Cin,Cout] mismatch: %s vs %s'
                         % (tuple(value.shape), tuple(filter_.shape)))
    n, t, cin = value.shape
    w, _, cout = filter_.shape
    out = torch.empty((n, t, cout), dtype=torch.float32, device=value.device)
    if out.numel() == 0:
        return out
    check(_lib.lib().pwv_causal_conv_f32(_ptr(value), _ptr(filter_), _ptr(out), n, t, cin, cout, w, int(dilation),
                                         _stream()), 'pwv_causal_conv_f32')
    return out


def linear_op(x2d: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], relu: bool,
              precision: Optional[str] = None) -> torch.Tensor:
    """y = act(x @ w + bias).  precision 'f32': exact fp32 MFMA; otherwise (default) split-fp16 MFMA -- the
    arithmetic of the fused kernels in the same mode."""
    m, k = x2d.shape
    nout = w.shape[1]
    y = torch.empty((m, nout), dtype=torch.float32, device=x2d.device)
    fn = _lib.lib().pwv_linear_f32 if (precision or DEFAULT_PRECISION) == 'f32' else _lib.lib().pwv_linear_split_f32
    check(fn(_ptr(x2d), _ptr(w), _ptr(bias), _ptr(y), m, k, nout, int(relu), _stream()), 'pwv_linear')
    return y


def crop_time_op(x: torch.Tensor, t_out: int, offset: int) -> torch.Tensor:
    n, t_in, c = x.shape
    out = torch.empty((n, t_out, c), dtype=torch.float32, device=x.device)
    check(_lib.lib().pwv_crop_time_f32(_ptr(x), _ptr(out), n, t_in, c, t_out, offset, _stream()), 'pwv_crop_time_f32')
    return out


def logistic_noise_op(shape: Sequence[int], device, seed: int, offset: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    z = out if out is not None else torch.empty(tuple(shape), dtype=torch.float32, device=device)
    if out is not None and (tuple(out.shape) != tuple(shape) or out.dtype != torch.float32 or not out.is_contiguous()):
        raise ValueError('out must be a contiguous float32 tensor of shape %s' % (tuple(shape),))
    check(_lib.lib().pwv_logistic_noise_f32(_ptr(z), z.numel(), seed, offset, _stream()), 'pwv_logistic_noise_f32')
    return z


def logistic_noise_stream_op(z: torch.Tensor, state: torch.Tensor) -> torch.Tensor:
    """The sampler in its capturable form (pwv_logistic_noise_stream_f32): `state` = int64[4] on the device, {seed, offset, 0, skip};
    every launch -- every replay of a captured one -- draws the next z.numel() counters of the stream and moves the offset on."""
    if state.dtype != torch.int64 or state.numel() != 4 or not state.is_cuda or not z.is_contiguous() or z.dtype != torch.float32:
        raise ValueError('state must be int64[4] on the GPU, z a contiguous float32 tensor')
    check(_lib.lib().pwv_logistic_noise_stream_f32(_ptr(z), z.numel(), state.data_ptr(), _stream()), 'pwv_logistic_noise_stream_f32')
    return z


def as_int64_bits(v: int) -> int:
    """A uint64 (a seed or a counter offset, 0 .. 2**64 - 1) as the int64 with the same bits: how a torch.int64 tensor carries it."""
    v = int(v) & ((1 << 64) - 1)
    return v - (1 << 64) if v >> 63 else v


def from_int64_bits(v: int) -> int:
    """The inverse of as_int64_bits: the uint64 an int64 read back from a device table stands for."""
    return int(v) & ((1 << 64) - 1)


def check_u64(v, what: str) -> int:
    """`v` as the sampler's uint64 -- an integer in [0, 2**64), not a bool -- or ValueError('<what> must be an integer in ...')."""
    if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not 0 <= int(v) < (1 << 64):
        raise ValueError('%s must be an integer in [0, 2**64), got %r' % (what, v))
    return int(v)


def os_seed() -> int:
    """A noise seed from the OS: what a model, a session or a tool draws where the caller gave none."""
    return int.from_bytes(os.urandom(7), 'little')


def logistic_noise_packed_op(cu_rows: torch.Tensor, streams: torch.Tensor, rows: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[rows, 1] Logistic(0,1) noise of a packed batch with one counter stream per utterance (pwv_logistic_noise_packed_f32): `cu_rows`
    int32 [n+1] on the GPU (the batch's prefix sums, cu_rows[n] = rows), `streams` int64 [n, 2] on the GPU = {seed_i, offset_i} (uint64
    bits, as_int64_bits).  Rows cu_rows[i] .. cu_rows[i+1]-1 equal logistic_noise_op((len_i, 1), seed=seed_i, offset=offset_i) bit for bit.
    The tables are read on the device: a captured launch replays with what they hold then."""
    for t, what, dt in ((cu_rows, 'cu_rows', torch.int32), (streams, 'streams', torch.int64)):
        if not isinstance(t, torch.Tensor) or t.dtype != dt or not t.is_contiguous():
            raise ValueError('%s must be a contiguous %s tensor' % (what, dt))
    for t, what in ((cu_rows, 'cu_rows'), (streams, 'streams')):
        if not t.is_cuda:
            raise _lib.PwvError('%s must live on the GPU (cuda device); there is no CPU path' % what)
    n = cu_rows.numel() - 1
    if cu_rows.dim() != 1 or n < 1 or tuple(streams.shape) != (n, 2):
        raise ValueError('cu_rows must be [n+1] (n >= 1) and streams [n, 2], got %s and %s' % (tuple(cu_rows.shape), tuple(streams.shape)))
    rows = int(rows)
    if not 0 <= rows < (1 << 31):
        raise ValueError('rows must be in [0, 2**31), got %d' % rows)
    if streams.device != cu_rows.device:
        raise ValueError('cu_rows and streams must be on one device')
    z = out if out is not None else torch.empty((rows, 1), dtype=torch.float32, device=cu_rows.device)
    if out is not None and (tuple(out.shape) != (rows, 1) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != cu_rows.device):
        raise ValueError('out must be a contiguous float32 [%d, 1] tensor on %s' % (rows, cu_rows.device))
    check(_lib.lib().pwv_logistic_noise_packed_f32(_ptr(z), _ptr(cu_rows), _ptr(streams), n, rows, _stream()), 'pwv_logistic_noise_packed_f32')
    return z


def logistic_noise_window(n: int, total_length: int, first_sample: int, window: int, device, seed: int, first_item: int = 0) -> torch.Tensor:
    """[n, window, 1] Logistic(0,1) noise for the samples [first_sample, first_sample + window) of the utterances
    first_item .. first_item + n - 1 of ONE counter-based stream in which utterance i, sample t is counter
    i * total_length + t: what a rank needs for its share of a sharded job (utterance shards: first_item = the rank's first
    utterance; time shards: first_sample = the window's start) -- every rank draws exactly the values an unsharded run
    with the same seed would have drawn there, with no communication."""
    z = torch.empty((n, window, 1), dtype=torch.float32, device=device)
    for i in range(n):
        logistic_noise_op((1, window, 1), device, seed=seed, offset=(first_item + i) * total_length + first_sample, out=z[i:i + 1])
    return z


def instance_norm_op(x: torch.Tensor, gamma: Optional[torch.Tensor], beta: Optional[torch.Tensor], eps: float = 1e-8) -> torch.Tensor:
    """modules.instance_normalization (modules.py:274-284) on a channels-last [N, T, C] tensor."""
    x = _require_cuda_f32(x, 'input')
    n, t, c = x.shape
    y = torch.empty_like(x)
    if x.numel() == 0:
        return y
    lib = _lib.lib()
    nbytes = lib.pwv_instance_norm_workspace_bytes(n, t, c)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=x.device)
    check(lib.pwv_instance_norm_f32(_ptr(x), _ptr(y), n, t, c, _ptr(gamma), _ptr(beta), float(eps), ws.data_ptr(), nbytes, _stream()),
          'pwv_instance_norm_f32')
    return y


def channel_affine_op(x: torch.Tensor, scale: Optional[torch.Tensor], bias: Optional[torch.Tensor], relu: bool = False,
                      tile32_rows: int = 0, channels: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = act(x * scale[c] + bias[c]) over the last axis (or over a tile32 buffer of `tile32_rows` x `channels`)."""
    y = out if out is not None else torch.empty_like(x)
    if x.numel() == 0:
        return y
    if tile32_rows:
        rows, c, tiled = tile32_rows, channels, 1
    else:
        c = x.shape[-1]
        rows, tiled = x.numel() // c, 0
    check(_lib.lib().pwv_channel_affine_f32(_ptr(x), _ptr(y), rows, c, _ptr(scale), _ptr(bias), tiled, int(relu), _stream()),
          'pwv_channel_affine_f32')
    return y


def add_op(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    out = torch.empty_like(a)
    if a.numel() % 4 == 0:
        check(_lib.lib().pwv_add_f32(_ptr(a), _ptr(b), _ptr(out), a.numel(), _stream()), 'pwv_add_f32')
        return out
    # odd sizes (scalar-channel tensors): the affine kernel's scalar path with a per-element "bias" is not available;
    # pad-free fallback through two launches on the multiple-of-4 prefix and the tail
    n4 = a.numel() // 4 * 4
    af, bf, of = a.reshape(-1), b.reshape(-1), out.reshape(-1)
    if n4:
        check(_lib.lib().pwv_add_f32(_ptr(af), _ptr(bf), _ptr(of), n4, _stream()), 'pwv_add_f32')
    of[n4:] = af[n4:] + bf[n4:]
    return out


def gate_op(f: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    out = torch.empty_like(f)
    check(_lib.lib().pwv_gate_f32(_ptr(f), _ptr(g), _ptr(out), f.numel(), _stream()), 'pwv_gate_f32')
    return out


def iaf_affine_op(z: torch.Tensor, s: torch.Tensor, b: torch.Tensor, sb_stride: int = 1) -> torch.Tensor:
    """out = z*s + b (modules.py:59); s/b may be strided views (shared net: stride 2)."""
    n, t = z.shape[0], z.shape[1]
    out = torch.empty_like(z)
    check(_lib.lib().pwv_iaf_front_f32(_ptr(z), s.data_ptr(), b.data_ptr(), sb_stride, _ptr(out), 0, None, None,
                                       n, t, 1, 4, _stream()), 'pwv_iaf_front_f32')
    return out


# --------------------------------------------------------------------------------------------
# per-net plan: packed weights resident in HBM
# --------------------------------------------------------------------------------------------
class NetPlan:
    def __init__(self, net, cond_mode: str, precision: int):
        """cond_mode: 'none' | 'frames' (hoisted projection) | 'samples' (per-sample cond GEMM)."""
        lib = _lib.lib()
        self.cond_mode = cond_mode
        self.precision = precision
        L = len(net.dilations)
        dev = net.device()
        use_skip = bool(net.use_skip_connection)
        cond_c = net.condition_channels if cond_mode == 'samples' else 0
        self.with_skip = use_skip
        self.layer_floats = lib.pwv_layer_packed_floats(int(use_skip), cond_c)
        self.packed_layers = torch.empty((L, self.layer_floats), dtype=torch.float32, device=dev)
        s = _stream()
        # the frame-rate projection operands (gc_filter|gc_gate and filter_bias|gate_bias of every layer, in the kernels'
        # column order, exp2 scales folded in) are packed by one small HIP launch per layer (pwv_pack_proj_f32)
        cc = net.condition_channels if cond_mode == 'frames' else 0
        self.proj_b = torch.empty((128 * L,), dtype=torch.float32, device=dev)
        self.proj_w = torch.empty((cc, 128 * L), dtype=torch.float32, device=dev) if cc else None
        # normalize='bn' (inference): every batch norm of the net is folded into these tensors (WaveNet.folded_variables)
        folded = net.folded_variables(cond_mode != 'none') if net.normalize == 'bn' else None
        self._lv = (lambda j: folded['layers'][j]) if folded else (lambda j: net.layer_variables(j, with_cond=cond_mode != 'none'))
        self._hv = folded['head'] if folded else net.head_variables()
        for j in range(L):
            v = self._lv(j)
            check(lib.pwv_pack_layer_f32(_ptr(v['filter']), _ptr(v['gate']), _ptr(v['dense']), _ptr(v.get('dense_bias')),
                                         _ptr(v['skip']) if use_skip else None,
                                         _ptr(v.get('skip_bias')) if use_skip else None,
                                         _ptr(v.get('gc_filter')) if cond_c else None,
                                         _ptr(v.get('gc_gate')) if cond_c else None,
                                         int(use_skip), cond_c, precision, _ptr(self.packed_layers[j]), s),
                  'pwv_pack_layer_f32')
            check(lib.pwv_pack_proj_f32(_ptr(v['gc_filter']) if cc else None, _ptr(v['gc_gate']) if cc else None,
                                        _ptr(v.get('filter_bias')), _ptr(v.get('gate_bias')), cc, j, L, _ptr(self.proj_w), _ptr(self.proj_b), s),
                  'pwv_pack_proj_f32')
        hv = self._hv
        last = self._lv(L - 1)
        self.head_floats = lib.pwv_head_packed_floats(net.out_channels)
        self.packed_head = torch.empty((self.head_floats,), dtype=torch.float32, device=dev)
        check(lib.pwv_pack_head_f32(None if use_skip else _ptr(last['skip']),
                                    None if use_skip else _ptr(last.get('skip_bias')),
                                    _ptr(hv['postprocess1']), _ptr(hv.get('postprocess1_bias')),
                                    _ptr(hv['postprocess2']), _ptr(hv.get('postprocess2_bias')),
                                    net.out_channels, precision, _ptr(self.packed_head), s), 'pwv_pack_head_f32')
        self.causal_bias = folded['causal_bias'] if folded else None      # batch norm behind the causal layer: its shift
        self._causal_filter_folded = folded['causal_filter'].contiguous() if folded else None
        self.causal_filter = self._causal_filter_folded if self._causal_filter_folded is not None else net.causal_filter()
        self.n_layers = L
        self.f16x3_ok, self.x_limit = True, 3.0e38
        if precision == _lib.PREC_F16X3:
            self._range_analysis(net, L, use_skip, cond_mode)
        # scalar-input nets (split-fp16 and fp32 paths): layer 0's filter|gate GEMM folded onto the four scalars it is a function
        # of (first_fold in the C ABI's argument structs); on the split-fp16 path the scalars themselves are then fp16 operands,
        # hence the extra bound on them
        self.first_fold = None
        if (FOLD_FIRST and self.f16x3_ok and net.in_channels == 1 and net.filter_width == 2
                and net.residual_channels == 64 and net.dilation_channels == 64 and self.causal_bias is None):
            v0 = self._lv(0)
            ff = torch.zeros((_lib.FIRST_FOLD_FLOATS,), dtype=torch.float32, device=dev)
            # (the fp16 storage mode reads the `hi` fragments of the split-fp16 layout, as it does for every other weight)
            pack = lib.pwv_pack_first_fold_f32 if precision == _lib.PREC_F32 else lib.pwv_pack_first_fold_f16x3
            check(pack(_ptr(self.causal_filter), _ptr(v0['filter']), _ptr(v0['gate']), _ptr(ff), s), 'pwv_pack_first_fold')
            if precision == _lib.PREC_F32:
                self.first_fold = ff
            elif bool(torch.isfinite(ff.view(torch.float16).float()).all()):
                self.first_fold = ff
                if precision == _lib.PREC_F16X3:
                    self.x_limit = min(self.x_limit, F16_LIMIT)

    def _range_analysis(self, net, L, use_skip, cond_mode):
        """Bound every operand the split-fp16 kernels convert to fp16 (weights after the exp2 scale folding; the residual
        stream |x_j| <= |h| + sum_i (||dense_i||_1 + |dense_bias_i|) because |tanh * sigmoid| < 1; relu(skip) feeding the
        head) from the weights alone.  What remains is a limit on the flow input, checked on the device at run time."""
        kf, kg = 2.8853900817779268, 1.4426950408889634
        lib = _lib.lib()
        dev = self.causal_filter.device
        stats = torch.zeros((L, 8), dtype=torch.float32, device=dev)
        for j in range(L):          # one small HIP launch per layer (pwv_range_stats_f32) instead of ~15 torch reductions
            v = self._lv(j)
            with_gc = cond_mode != 'none'
            check(lib.pwv_range_stats_f32(_ptr(v['filter']), _ptr(v['gate']), _ptr(v['dense']), _ptr(v.get('dense_bias')), _ptr(v['skip']),
                                          _ptr(v.get('skip_bias')), _ptr(v['gc_filter']) if with_gc else None,
                                          _ptr(v['gc_gate']) if with_gc else None, net.condition_channels if with_gc else 0,
                                          _ptr(stats[j]), _stream()), 'pwv_range_stats_f32')
        hv = self._hv
        extra = torch.stack([hv['postprocess1'].abs().max(), self.causal_filter.abs().sum(dim=(0, 1)).max()])
        st, (post1_max, c_causal) = stats.cpu().numpy(), extra.cpu().tolist()
        w_max = max(float((st[:, [0, 4]].max()) * kf), float(st[:, [1, 5]].max() * kg), float(st[:, 2:4].max()), post1_max)
        res_bound = float(st[:L - 1, 6].sum())
        skip_bound = float(st[:, 7].sum() if use_skip else st[L - 1, 7])
        # normalize='bn': the causal layer is followed by a folded batch norm, h = a0 * conv(x) + c0 -- the shift is part of |h|
        c0_max = float(self.causal_bias.abs().max()) if self.causal_bias is not None else 0.0
        budget = F16_LIMIT - res_bound - c0_max
        self.f16x3_ok = w_max < F16_LIMIT and skip_bound < F16_LIMIT and res_bound < F16_LIMIT and budget > 0
        self.x_limit = budget / c_causal if c_causal > 0 else 3.0e38
        # what the guard knows at pack time (range_report / tools/precision_report.py: limit vs observed per operand class)
        self.range_bounds = {'w_max': w_max, 'res_bound': res_bound, 'skip_bound': skip_bound, 'c_causal': c_causal, 'c0_max': c0_max}


_plan_cache: Dict[Tuple, Tuple[int, NetPlan]] = {}
_cond_cache = None      # (weakref(condition tensor), its version, precision, converted copy, stream it was made on)


def get_plan(net, cond_mode: str, precision: int) -> NetPlan:
    # the architecture is part of the key: the same store + scope can be re-used with another dilation list or with
    # use_skip_connection toggled (no variable is created then, so the store version alone does not change)
    key = (net.store.uid, net.full_scope, cond_mode, precision, tuple(int(d) for d in net.dilations),
           bool(net.use_skip_connection), bool(net.use_biases), net.in_channels, net.out_channels,
           net.condition_channels, net.filter_width, net.residual_channels, net.dilation_channels, net.skip_channels,
           net.normalize or '', bool(FOLD_FIRST))
    hit = _plan_cache.get(key)
    if hit is not None and hit[0] == net.store.version:
        return hit[1]
    plan = NetPlan(net, cond_mode, precision)
    _plan_cache[key] = (net.store.version, plan)   # read AFTER planning: creating variables bumps it
    return plan


def clear_plan_cache() -> None:
    _plan_cache.clear()


def _same_structure(a, b) -> bool:
    return (list(a.dilations) == list(b.dilations) and a.use_skip_connection == b.use_skip_connection
            and a.in_channels == b.in_channels and a.out_channels == b.out_channels
            and a.condition_channels == b.condition_channels and a.filter_width == b.filter_width)


def tail_fusable(prec: int) -> bool:
    """Does the persistent launch of this arithmetic run the net's last layer + head (+ affine) as its tail?"""
    return bool(FUSE_TAIL and FUSE_HEAD and prec in (_lib.PREC_F16X3, _lib.PREC_F32))      # (round 6: the exact-fp32 kernel has the tail too)


def head_fusable(prec: int) -> bool:
    """Persistent launches without the tail: does the head run inside the last layer's launch (else in a launch of its own)?"""
    return prec == _lib.PREC_F16X3 or (prec == _lib.PREC_F32 and FUSE_HEAD)


class _Path(NamedTuple):
    """Which launches one forward enqueues (_choose_path): decided once, read by the launch helpers."""
    runs: Optional[List[Tuple[int, _lib.PersistArgs]]]    # the persistent launches (_persist_launches); None: per-layer launches
    tail: bool              # layer L-1 + head (+ the flow's affine) run inside the last persistent launch
    first_fused: bool       # layer 0 rebuilds the causal layer from the scalar input (x_first): no causal-layer launch
    two: bool               # per-layer launches of G = 2 nets: each net's chain on a side stream of its own (TWO_STREAMS)

    persist = property(lambda self: self.runs is not None)     # (else per-layer launches)
    # the WHOLE flow inside the persistent launches -- layer 0 and the tail included: the only form the packed and the streaming launches have
    whole_flow = property(lambda self: self.runs is not None and self.tail and self.first_fused)


def _choose_path(net0, plans, mode: str, n: int, t: int, max_workgroups: int, cond_geom) -> _Path:
    """The launch path of a forward of the nets behind `plans` (one structure, one arithmetic, conditioning `mode`) on N x T rows."""
    G, prec = len(plans), plans[0].precision
    use_skip = bool(net0.use_skip_connection)
    first_fused = bool(FUSE_FIRST and prec in (_lib.PREC_F16X3, _lib.PREC_F32, _lib.PREC_F16) and net0.in_channels == 1
                       and net0.filter_width == 2 and net0.residual_channels == 64 and not use_skip and plans[0].causal_bias is None)
    runs, tail = None, False
    if (prec == _lib.PREC_F32 or (prec == _lib.PREC_F16X3 and FUSE_HEAD)) and mode != 'samples' and not use_skip and max_workgroups == 0:
        def launches(tail_q):
            return _persist_launches(G, n, t, net0.dilations, 0 if first_fused else 1, tail_q, prec, plans[0].layer_floats, cond_geom)
        # the tail (last layer + head inside the launch) has a look-back of its own -- the stack's LAST dilation: ask for the launch
        # that will be made, and keep the persistent layers with the tail as a launch of its own where only the tail does not fit
        tail = tail_fusable(prec)
        runs = launches(net0.out_channels if tail else 0)
        if runs is None and tail:
            tail, runs = False, launches(0)
    two = G == 2 and TWO_STREAMS and max_workgroups == 0 and runs is None
    return _Path(runs, tail, first_fused, two)


def _set_x_first(a, plans, x: torch.Tensor, x_limit: float) -> None:
    """pwv_stack_args / pwv_persist_args: layer 0 rebuilds the causal layer from the scalar input x (range-checked against x_limit)."""
    a.x_first, a.x_limit, a.range_flag = _ptr(x), x_limit, range_flag_ptr()
    for g, p in enumerate(plans):
        a.causal_filter[g] = p.causal_filter.data_ptr()
    if FOLD_FIRST and all(p.first_fold is not None for p in plans):
        for g, p in enumerate(plans):
            a.first_fold[g] = p.first_fold.data_ptr()


def _layer_args(net0, plans, projs, row_stride: int, cond_geom, bufs, j: int, src: int, dst: int, x: torch.Tensor) -> _lib.LayerArgs:
    """pwv_layer_args of layer j of the nets behind `plans`: reads bufs[g][src], writes bufs[g][dst]."""
    la = _lib.LayerArgs()
    la.G, la.precision, la.skip_init = len(plans), plans[0].precision, 1
    for g, p in enumerate(plans):
        la.x_in[g], la.x_out[g] = bufs[g][src].data_ptr(), bufs[g][dst].data_ptr()
        la.packed[g] = p.packed_layers.data_ptr() + 4 * p.layer_floats * j
        la.proj[g] = projs[g].data_ptr() + 4 * 128 * j
    la.proj_row_stride = row_stride
    la.N, la.T, la.dilation = x.shape[0], x.shape[1], int(net0.dilations[j])
    la.cond_hop, la.cond_offset, la.cond_frames = cond_geom
    return la


def _run_stack_persist(path: _Path, nets, plans, projs, bufs, outs, x, x_limit, row_stride, cond_geom, affine=None, geom=None, stream_hist=None):
    """Layers 0 .. L-2 as the persistent launches of `path` (layer 0 a launch of its own when it cannot rebuild the causal layer
    itself), with layer L-1 + the head behind them -- and, given `affine` = (x, out), the flow's affine out = x*s + b -- INSIDE the
    last launch where `path.tail` (otherwise one more launch for them); all nets of the flow in every launch, all on the current
    stream.  `bufs[g]` holds THREE tile32 buffers: the persistent launch rotates through them (include/pwv_hip.h,
    pwv_persist_args.x_ring).  With `geom` (a VarlenGeometry; x is then its [1, R, 1]) every launch carries the packed batch's
    fields.  With `stream_hist` = (pwv_stream_args, row_off[g][layer]) the launches are the STREAMING ones: every
    run is told where its own layers' row histories -- and the tail's -- lie in a block.  Returns True when the affine was evaluated
    by the launch."""
    lib, s = _lib.lib(), _stream()
    G, L, prec = len(nets), plans[0].n_layers, plans[0].precision
    net0 = nets[0]
    stride = plans[0].layer_floats

    if not path.first_fused:                # layer 0 on the causal layer's buffer (bufs[g][0]) as a launch of its own
        la = _layer_args(net0, plans, projs, row_stride, cond_geom, bufs, 0, 0, 2, x)
        la.out_mode = _lib.OUT_RESIDUAL
        check(lib.pwv_wavenet_layer_f32(ctypes.byref(la), s), 'pwv_wavenet_layer_f32')

    # the residual layers (0 or) 1 .. L-2 as persistent launches of at most PERSIST_MAX_LAYERS layers each, handing the ring on
    Q = net0.out_channels
    affine_fused = bool(path.tail and affine is not None and ((G == 2 and Q == 1) or (G == 1 and Q == 2)))
    for j0, pa in path.runs:
        for g in range(G):
            pa.x_ring[g] = bufs[g][0].data_ptr()
            pa.packed_layers[g] = plans[g].packed_layers.data_ptr() + 4 * stride * j0
            pa.proj[g] = projs[g].data_ptr() + 4 * 128 * j0
        pa.ring_stride, pa.proj_row_stride = bufs[0][0].numel(), row_stride
        if j0 == 0:
            _set_x_first(pa, plans, x, x_limit)
        if geom is not None:
            geom.set_args(pa)
        tail_here = path.tail and pa is path.runs[-1][1]
        if stream_hist is not None:
            sa, row_off = stream_hist
            layers = list(range(j0, j0 + pa.n_layers)) + ([L - 1] if tail_here else [])
            hist_offs = [(ctypes.c_size_t * len(layers))(*[max(int(row_off[g][j]), 0) for j in layers]) for g in range(G)]      # (layer 0: unused)
            pa.hist = ctypes.addressof(sa)
            for g in range(G):
                pa.hist_row_off[g] = hist_offs[g]
        # one zero-initialised workspace per (device, stream), kept: a launch leaves it clean, so none needs a zeroing kernel
        wkey = (bufs[0][0].device, torch.cuda.current_stream().cuda_stream)
        ws = _persist_ws.get(wkey)
        if ws is None or ws.numel() < pa.workspace_bytes:
            ws = _persist_ws[wkey] = torch.zeros((max(pa.workspace_bytes, 1 << 16),), dtype=torch.uint8, device=bufs[0][0].device)
        pa.workspace, pa.workspace_clean = ws.data_ptr(), 1
        pa.status = persist_status_ptr()
        if tail_here:                        # layer L-1 + head (+ affine) behind this run's layers, inside the launch
            for g in range(G):
                pa.tail_layer[g] = plans[g].packed_layers.data_ptr() + 4 * stride * (L - 1)
                pa.tail_head[g] = plans[g].packed_head.data_ptr()
                pa.tail_out[g] = outs[g].data_ptr()
            if affine_fused:
                pa.affine_x, pa.affine_out = affine[0].data_ptr(), affine[1].data_ptr()
        ev = None
        if EVENT_LOG is not None:
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
        if PERSIST_ARGS_HOOK is not None:
            PERSIST_ARGS_HOOK(pa)
        check(lib.pwv_wavenet_stack_persist_f32(ctypes.byref(pa), s), 'pwv_wavenet_stack_persist_f32')
        if ev is not None:
            ev[1].record()
            EVENT_LOG.append(('persist', ev[0], ev[1], G, pa.n_layers, 1 if j0 == 0 else 0, 1 if tail_here else 0,
                              int(lib.pwv_persist_short_input(ctypes.byref(pa))),      # [7]: the short-input instantiation (round 6)
                              1 if stream_hist is not None else 0))                    # [8]: a STREAMING launch (pwv_persist_args.hist)
    if path.tail:
        return affine_fused
    last = path.runs[-1][1]
    out_slot = (last.n_layers - 1 + last.ring_rotation) % 3      # where the last run left layer L-2
    spare = (out_slot + 1) % 3

    la = _layer_args(net0, plans, projs, row_stride, cond_geom, bufs, L - 1, out_slot, spare, x)
    la.out_mode = _lib.OUT_GATED
    fuse_head = head_fusable(prec)
    if fuse_head:                        # the head runs inside the last layer's launch
        for g in range(G):
            la.head_packed[g] = plans[g].packed_head.data_ptr()
            la.head_out[g] = outs[g].data_ptr()
        la.head_q = Q
    check(lib.pwv_wavenet_layer_f32(ctypes.byref(la), s), 'pwv_wavenet_layer_f32')
    if not fuse_head:
        ha = _lib.HeadArgs()
        ha.G, ha.N, ha.T, ha.Q = G, x.shape[0], x.shape[1], Q
        for g in range(G):
            ha.in_[g], ha.packed[g], ha.out[g] = bufs[g][spare].data_ptr(), plans[g].packed_head.data_ptr(), outs[g].data_ptr()
        ha.in_mode, ha.precision = _lib.HEAD_IN_GATED, prec
        check(lib.pwv_wavenet_head_f32(ctypes.byref(ha), s), 'pwv_wavenet_head_f32')
    return False


_bank_cache = {}      # tuple of plan ids -> (plans (kept alive), concatenated proj_w [K, total], proj_b [total], column offsets)


FUSE_PROLOGUE = os.environ.get('PWV_FUSE_PROLOGUE', '1') != '0'      # 'repeat' conditioning: mel range check + dense/relu + the projection GEMM as ONE launch (pwv_cond_project_f32)
# ... where it pays.  The fused launch recomputes the condition per 128-column block of the bank and holds 113 KB of LDS (one
# workgroup per CU): same box, fused vs three launches (profiles/r05_ab_experiments.md): C1 (201 frames x 2048 columns) -5 %,
# default model at 16000 samples (201 x 15360) level, C3 (2001 x 15360) +1.3 %, C4 +1 %.  Bit-identical either way, so the choice may
# depend on the size: frames x columns up to this many outputs take the one launch.
FUSE_PROLOGUE_MAX_OUTPUTS = 1 << 21


def _projection_bank(nets: Sequence, channels: int, prec: int):
    """(plans, [C, total] weights, [total] biases, column offsets) of the one projection GEMM of a forward, or None when fewer than
    two nets can share it (not fused-capable, another arithmetic after the range fallback)."""
    for _ in range(2):
        # (a first forward creates its variables while the plans are built, and every new variable outdates the plans
        # made before it: plan again once the store has stopped changing, so that run_nets finds these very plans)
        versions = [net.store.version for net in nets]
        plans = []
        for net in nets:
            if not getattr(net, 'fused_supported', None) or channels != net.condition_channels:
                continue
            if not net.fused_supported(_FrameShape(channels)):
                continue
            p = get_plan(net, 'frames', prec)
            if prec == _lib.PREC_F16X3 and not (p.f16x3_ok and p.x_limit > 0):
                continue
            if all(p is not q for q in plans):
                plans.append(p)
        if versions == [net.store.version for net in nets]:
            break
    if len(plans) < 2:
        return None
    key = tuple(id(p) for p in plans)
    hit = _bank_cache.get(key)
    if hit is None:
        if len(_bank_cache) >= 8:
            _bank_cache.clear()
        offs, total = [], 0
        for p in plans:
            offs.append(total)
            total += p.proj_w.shape[1]
        hit = (plans, torch.cat([p.proj_w for p in plans], dim=1).contiguous(), torch.cat([p.proj_b for p in plans]).contiguous(), offs)
        _bank_cache[key] = hit
    return hit


class _FrameShape(RepeatedCondition):
    """(what WaveNet.fused_supported looks at: a frame-rate condition with this many channels)"""

    def __init__(self, channels):
        self.frames = torch.empty((0, 1, channels))
        self.hop = self.offset = self.length = 0


def project_all(nets: Sequence, cond, precision: Optional[str] = None) -> None:
    """The frame-rate projections P of EVERY net of a forward (all flows) as one GEMM: P depends on the mel frames only,
    not on a flow's input, so none of it has to sit between two flows (per flow that was two small launches plus their
    cross-stream dependencies on the critical path).  The result is attached to the RepeatedCondition; run_nets picks its
    nets' column blocks out of it (row stride = all columns).  Nets that cannot use it (not fused-capable, a different
    arithmetic after the range fallback) simply project for themselves as before."""
    if not HOIST_P or not isinstance(cond, RepeatedCondition) or not nets or getattr(cond, 'proj_bank', None) is not None:
        return
    prec = PRECISIONS[precision or DEFAULT_PRECISION]
    bank = _projection_bank(nets, cond.frames.shape[2], prec)
    if bank is None:
        return
    plans, w_all, b_all, offs = bank
    n, frames, c = cond.frames.shape
    f2d = _require_cuda_f32(cond.frames, 'frames').reshape(n * frames, c)
    p_all = linear_op(f2d, w_all, b_all, relu=False, precision=precision or DEFAULT_PRECISION)
    cond.proj_bank = {id(p): p_all[:, o:o + p.proj_w.shape[1]] for p, o in zip(plans, offs)}


def repeat_condition_with_projections(nets: Sequence, melspec: torch.Tensor, dense: torch.Tensor, hop: int, length: int,
                                      precision: Optional[str], mel_limit: Optional[float]):
    """The prologue of a 'repeat'-conditioned forward as ONE launch (pwv_cond_project_f32): the range check of the mel, the
    frame-rate condition relu(mel @ dense) (models.py:128-130) and the projections of every net (project_all) -- bit-identical to
    the three launches it replaces.  Returns the RepeatedCondition with its projection bank attached, or None when the shape is
    outside the fused kernel's (the caller then takes the separate launches)."""
    name = precision or DEFAULT_PRECISION
    if not (FUSE_PROLOGUE and HOIST_P) or name == 'f32' or not nets:
        return None
    n, t_mel, n_mels = melspec.shape
    c = dense.shape[1]
    if n_mels % 8 or c % 8 or n_mels > 80 or c > 80:
        return None
    bank = _projection_bank(nets, c, PRECISIONS[name])
    if bank is None:
        return None
    plans, w_all, b_all, offs = bank
    m = n * t_mel
    if m * w_all.shape[1] > FUSE_PROLOGUE_MAX_OUTPUTS:
        return None
    frames = torch.empty((n, t_mel, c), dtype=torch.float32, device=melspec.device)
    p_all = torch.empty((m, w_all.shape[1]), dtype=torch.float32, device=melspec.device)
    flag = range_flag_ptr() if (name == 'f16x3' and mel_limit is not None) else None
    if flag is not None:
        _log_range('mel', melspec, mel_limit)
    check(_lib.lib().pwv_cond_project_f32(_ptr(melspec), _ptr(dense), n_mels, _ptr(w_all), _ptr(b_all), _ptr(frames), _ptr(p_all), m, c,
                                          w_all.shape[1], float(mel_limit or 0.0), flag, _stream()), 'pwv_cond_project_f32')
    cond = RepeatedCondition(frames, hop, hop // 2, length)
    cond.proj_bank = {id(p): p_all[:, o:o + p.proj_w.shape[1]] for p, o in zip(plans, offs)}
    return cond


def run_nets(nets: Sequence, x: torch.Tensor, cond, precision: Optional[str] = None,
             max_workgroups: int = 0) -> List[torch.Tensor]:
    """Evaluate 1 or 2 structurally identical fused-capable WaveNets on the same input/condition.
    Returns one [N, T, Q] tensor per net."""
    return _run_nets(nets, x, cond, precision, max_workgroups, None)[0]


def run_flow(nets: Sequence, x: torch.Tensor, cond, precision: Optional[str] = None) -> torch.Tensor:
    """One IAF flow (modules.py:53-60): out = x * scale + shift with (scale, shift) = the outputs of two scalar-input nets, or
    the two outputs of one shared net (route 1 of DESIGN.md section 9 "Routes", which lists all four).  On the default path the
    whole flow is ONE persistent launch (the affine is evaluated inside it, pwv_persist_args.affine_x); otherwise the nets' launches
    are followed by the affine kernel."""
    x = _require_cuda_f32(x, 'input')
    out = torch.empty_like(x)
    outs, done = _run_nets(nets, x, cond, precision, 0, out)
    return out if done else _flow_affine(x, outs)


def _flow_affine(x: torch.Tensor, outs: List[torch.Tensor]) -> torch.Tensor:
    """The flow's affine x * scale + shift as a launch of its own (where the persistent launch did not evaluate it): (scale, shift) =
    the outputs of the flow's two nets, or the two interleaved outputs of its one shared net."""
    if len(outs) == 2:
        return iaf_affine_op(x, outs[0], outs[1], 1)
    flat = outs[0].reshape(-1)
    return iaf_affine_op(x, flat, flat[1:], 2)


# ---- packed ("varlen") batches: utterances of different lengths in one forward (include/pwv_hip.h, pwv_persist_args.cu_rows) ------------
VARLEN_PADDED = 0        # flows of packed batches that took the padded fallback (tests / tools read it)
VARLEN_PADDED_WHY = None  # ... and why the last of them did (graph.GraphedPackedVocoder refuses with it)


def _remap_bank(bank: dict, total_frames: int, remap) -> dict:
    """A projection bank (RepeatedCondition.proj_bank) over other frame rows: the bank's column blocks are views of ONE [F, cols] GEMM
    output, so `remap` (rows in, rows out: a padding, a gather) is applied to that once and the blocks keep their column offsets.  The
    prologue is per frame: a remapped row holds the bits a prologue over the remapped frames would compute.  (The GEMM output starts at
    its first block, not necessarily at offset 0 of its storage: it may itself be a view into a larger allocation.)"""
    base = min(bank.values(), key=lambda v: v.storage_offset())
    full = base.as_strided((total_frames, base.stride(0)), (base.stride(0), 1), base.storage_offset())
    rows = remap(full)
    return {k: rows[:, v.storage_offset() - full.storage_offset():][:, :v.shape[1]] for k, v in bank.items()}


class PackedLayout:
    """The host side of a packed batch's layout: utterance i has lengths[i] samples, rows cu_rows_host[i] ..
    cu_rows_host[i+1]-1 of every [R, C] tensor, and t_mel_i = lengths[i] / hop + 1 condition frames, rows cu_frames_host[i] .. of every
    [F, C] tensor.  Plain integers: no device."""

    def __init__(self, lengths: Sequence[int], hop: int):
        self.lengths = [int(v) for v in lengths]
        self.hop = int(hop)
        if not self.lengths:
            raise ValueError('a packed batch needs at least one utterance')
        for v in self.lengths:
            if v <= 0 or v % self.hop:
                raise ValueError('utterance lengths must be positive multiples of hop_length (%d), got %d' % (self.hop, v))
        self.frames = [v // self.hop + 1 for v in self.lengths]
        self.cu_rows_host, self.cu_frames_host = [0], [0]
        for v, f in zip(self.lengths, self.frames):
            self.cu_rows_host.append(self.cu_rows_host[-1] + v)
            self.cu_frames_host.append(self.cu_frames_host[-1] + f)
        self.n, self.rows, self.total_frames = len(self.lengths), self.cu_rows_host[-1], self.cu_frames_host[-1]
        self.max_len, self.max_frames = max(self.lengths), max(self.frames)


class VarlenGeometry(PackedLayout):
    """A PackedLayout on a device.  Sample t of utterance i is conditioned on frame cu_frames[i] + (t + hop/2) // hop and looks back
    at zeros for t < d.  Holds the host prefix sums (the launches are sized on the host), their device copies and, made on first
    use, the per-unit records of the persistent launches and the index maps of the padded fallback."""

    def __init__(self, lengths: Sequence[int], hop: int, device, tables=None):
        """`tables` (optional): caller-owned device buffers (cu_rows int32 [N+1], cu_frames int32 [N+1], unit map int32
        [ceil(R/32) * VARLEN_REC_INTS]) that the caller keeps filled; nothing is uploaded, and unit_map() hands out the buffer as it is
        (the caller rebuilds it, build_unit_map(), ahead of every forward: graph.GraphedPackedVocoder rewrites the tables between
        replays of one capture)."""
        super().__init__(lengths, hop)
        self.device = device
        if tables is None:
            both = self._upload([self.cu_rows_host, self.cu_frames_host], torch.int32)
            self.cu_rows, self.cu_frames = both[0], both[1]
            self._unit_map = None
        else:
            self.cu_rows, self.cu_frames, self._unit_map = tables
            if self._unit_map.numel() != (self.rows + 31) // 32 * _lib.VARLEN_REC_INTS or self.cu_rows.numel() != self.n + 1:
                raise ValueError('tables do not match %d utterances of %d rows' % (self.n, self.rows))
        self._pad_rows = self._pad_frames = None
        self._cond_cache = None

    def _upload(self, table, dtype) -> torch.Tensor:
        """A small host table on the device WITHOUT a synchronisation: a copy from pageable memory makes the host wait until the stream
        has drained (the previous forward), which leaves the GPU idle while this forward's launches are enqueued.  Staged in pinned
        memory instead (torch keeps the staging buffer alive until the copy has run)."""
        t = torch.tensor(table, dtype=dtype)
        if torch.device(self.device).type != 'cuda':
            return t
        return t.pin_memory().to(self.device, non_blocking=True)

    def stream_table(self, streams: Sequence[Tuple[int, int]]) -> torch.Tensor:
        """The int64 [N, 2] table {seed_i, offset_i} (uint64 bits) of logistic_noise_packed_op on the device, staged like the prefix sums."""
        return self._upload([[as_int64_bits(a), as_int64_bits(b)] for a, b in streams], torch.int64)

    def persistent_ok(self) -> bool:
        """Every utterance long enough for the persistent launch's packed form (a unit spans at most two utterances)."""
        return min(self.lengths) >= _lib.VARLEN_MIN_ROWS

    def unit_map(self) -> torch.Tensor:
        if self._unit_map is None:
            units = (self.rows + 31) // 32
            self._unit_map = torch.empty((units * _lib.VARLEN_REC_INTS,), dtype=torch.int32, device=self.device)
            self.build_unit_map()
        return self._unit_map

    def build_unit_map(self) -> None:
        """Enqueue pwv_varlen_unit_map: the unit records from the device tables, into the unit map's buffer."""
        check(_lib.lib().pwv_varlen_unit_map(_ptr(self.cu_rows), _ptr(self.cu_frames), self.n, (self.rows + 31) // 32, _ptr(self._unit_map),
                                             _stream()), 'pwv_varlen_unit_map')

    def set_args(self, pa) -> None:
        """The packed-batch fields of one pwv_persist_args (the plan was made on N = 1, T = R: the same rows and units)."""
        pa.N, pa.T = self.n, 0
        pa.cu_rows, pa.cu_frames = _ptr(self.cu_rows), _ptr(self.cu_frames)
        pa.unit_map, pa.varlen_rows = _ptr(self.unit_map()), self.rows

    # -- the padded fallback: [R, C] <-> zero-padded [N, max_len, C] (rows past an utterance's end are zero, and by causality they
    #    influence nothing before them: the padded batch computes every real row exactly as the packed one)
    def _index(self, cu, counts, stride):
        """The padded position i * stride + t of packed row cu[i] + t, for every row, made on the device: row r of utterance i moves
        by i * stride - cu[i], so the map is arange(size) plus that shift repeated counts[i] times -- per utterance, not per row, on
        the host (one copy of 2N ints, no synchronisation)."""
        per_utt = self._upload([counts, [i * stride - c for i, c in enumerate(cu[:-1])]], torch.int64)
        size = cu[-1]
        return torch.arange(size, dtype=torch.int64, device=self.device) + torch.repeat_interleave(per_utt[1], per_utt[0], output_size=size)

    def pad_rows(self, x: torch.Tensor) -> torch.Tensor:
        if self._pad_rows is None:
            self._pad_rows = self._index(self.cu_rows_host, self.lengths, self.max_len)
        c = x.shape[-1]
        out = torch.zeros((self.n * self.max_len, c), dtype=x.dtype, device=x.device)
        out.index_copy_(0, self._pad_rows, x.reshape(self.rows, c))
        return out.reshape(self.n, self.max_len, c)

    def unpad_rows(self, y: torch.Tensor) -> torch.Tensor:
        c = y.shape[-1]
        return y.reshape(self.n * self.max_len, c).index_select(0, self._pad_rows)

    def pad_frames(self, f: torch.Tensor) -> torch.Tensor:
        if self._pad_frames is None:
            self._pad_frames = self._index(self.cu_frames_host, self.frames, self.max_frames)
        c = f.shape[-1]
        out = torch.zeros((self.n * self.max_frames, c), dtype=f.dtype, device=f.device)
        out.index_copy_(0, self._pad_frames, f.reshape(self.total_frames, c))
        return out.reshape(self.n, self.max_frames, c)

    def pad_condition(self, cond):
        """The packed condition (a RepeatedCondition over [1, F, C] frames with its projection bank, a per-sample [1, R, C] tensor, or
        None) in the padded batch's form; made once per condition object (every flow of a forward shares it)."""
        if cond is None:
            return None
        hit = self._cond_cache
        if hit is not None and hit[0]() is cond:
            return hit[1]
        if isinstance(cond, RepeatedCondition):
            padded = RepeatedCondition(self.pad_frames(cond.frames), cond.hop, cond.offset, self.max_len)
            bank = getattr(cond, 'proj_bank', None)
            if bank is not None:
                padded.proj_bank = _remap_bank(bank, self.total_frames, lambda full: self.pad_frames(full).reshape(self.n * self.max_frames, -1))
        else:
            padded = self.pad_rows(cond)
        self._cond_cache = (weakref.ref(cond), padded)
        return padded


def _instance_norm(nets) -> bool:
    """Instance normalisation ('in') inside a net: its statistics span the whole time axis, so neither a packed or padded batch nor a
    chunk of a stream computes them (run_flow_varlen and stream_refusal refuse it)."""
    return any(getattr(n, 'normalize', None) == 'in' for n in nets)


def _flow_structure(nets, cond, precision: Optional[str] = None, per_sample: bool = False, skip: bool = False) -> Optional[str]:
    """Which structural property keeps a flow (its nets) off the forms that run it whole inside the fused launches -- the packed batch's
    and the streaming ones -- as a key, or None: 'samples' (per-sample conditioning), 'skip' (skip accumulation), 'f16' (the fp16
    storage mode), 'shape' (not two scalar-in / scalar-out nets or one shared net of two outputs, all fused-capable, of one structure
    and one precision).  varlen_fallback_reason and stream_refusal word them.  per_sample=True asks about the per-layer streaming route
    with a per-sample condition (run_flow_stream): 'samples' is then no obstacle, and a condition that is NOT per sample is 'frames'.
    skip=True asks about the per-layer streaming route with skip accumulation: 'skip' is then no obstacle, and nets WITHOUT
    use_skip_connection are 'noskip'."""
    net0 = nets[0]
    if per_sample:
        if cond is None or isinstance(cond, RepeatedCondition):
            return 'frames'
    elif cond is not None and not isinstance(cond, RepeatedCondition):
        return 'samples'
    if skip:
        if not net0.use_skip_connection:
            return 'noskip'
    elif net0.use_skip_connection:
        return 'skip'
    if (precision or net0.precision or DEFAULT_PRECISION) == 'f16':
        return 'f16'
    if not (all(n.fused_supported(cond) for n in nets) and all(_same_structure(net0, n) for n in nets)
            and all(n.precision == net0.precision for n in nets) and net0.in_channels == 1
            and ((len(nets) == 2 and net0.out_channels == 1) or (len(nets) == 1 and net0.out_channels == 2))):
        return 'shape'
    return None


_VARLEN_STRUCTURE_WHY = {'samples': 'per-sample conditioning', 'skip': 'skip accumulation', 'f16': "precision 'f16'",
                         'shape': 'the flow has no fused form'}


def varlen_fallback_reason(nets, cond, geom: VarlenGeometry, precision: Optional[str] = None) -> Optional[str]:
    """Why a flow (its nets) of a packed batch takes the padded fallback -- or None: the persistent launches of the packed form, where
    the library plans the R rows persistently with layer 0 and the tail inside the launches (what a uniform batch of R rows would take)."""
    if not geom.persistent_ok():
        return 'an utterance shorter than %d samples' % _lib.VARLEN_MIN_ROWS
    if PERSIST is False:
        return 'PWV_PERSIST=0'
    if persist_suspended():
        return 'persistent launches suspended after a give-up'
    if PERSIST == 'auto' and geom.rows > PERSIST_AUTO_MAX_ROWS:
        return 'more than PERSIST_AUTO_MAX_ROWS rows'
    return _VARLEN_STRUCTURE_WHY.get(_flow_structure(nets, cond, precision))


def run_flow_varlen(flow, x: torch.Tensor, cond, geom: VarlenGeometry, precision: Optional[str] = None) -> torch.Tensor:
    """One IAF flow (LinearIAFLayer / SharedIAFLayer) over a packed batch: x [R, 1] -> [R, 1], `cond` over the packed frames [1, F, C]
    (length R) or None (route 2 of DESIGN.md section 9 "Routes").  The path is chosen once: the persistent launches of the packed
    form (pwv_persist_args.cu_rows) wherever a uniform batch of R rows would run the flow whole inside its persistent launches; otherwise
    (varlen_fallback_reason) the PADDED fallback: the flow's ordinary path on the zero-padded [N, max_len, 1] batch, gathered back.
    Both give the same bits: every stage of such a flow is causal and row-local in the batch, so the zero rows behind an utterance
    change nothing in front of them.  Instance normalisation ('in') is not row-local -- its statistics span the time axis, padding
    included -- so nets that use it are refused here (IAFVocoder.generate_varlen runs them utterance by utterance).  Only enqueues,
    like run_flow."""
    global VARLEN_PADDED, VARLEN_PADDED_WHY
    nets = list(flow.nets())
    if _instance_norm(nets):
        raise _lib.PwvError("run_flow_varlen: nets with instance normalisation ('in') have no packed or padded form (its statistics "
                            "span the time axis); run the utterances one by one")
    x = _require_cuda_f32(x, 'input')
    if x.dim() != 2 or tuple(x.shape) != (geom.rows, 1):
        raise ValueError('input must be the packed batch [%d, 1], got %s' % (geom.rows, tuple(x.shape)))
    why = varlen_fallback_reason(nets, cond, geom, precision)
    if why is None:
        x3 = x.reshape(1, geom.rows, 1)
        out = torch.empty_like(x3)
        res = _run_nets(nets, x3, cond, precision or nets[0].precision, 0, out, geom)
        if res is not None:
            outs, done = res
            return (out if done else _flow_affine(x3, outs)).reshape(geom.rows, 1)
        why = 'the library plans this stack at %d rows per layer' % geom.rows
    VARLEN_PADDED += 1
    VARLEN_PADDED_WHY = why
    y = flow(geom.pad_rows(x), geom.pad_condition(cond))        # (nested in the caller's verified_call: only enqueues)
    return geom.unpad_rows(y)


class _FlowPrep(NamedTuple):
    """What every route of a flow ("Routes") settles before it enqueues (_prepare_flow)."""
    precision: str          # the arithmetic's name AFTER the pack-time demotion ('f16x3' whose weights leave fp16's range runs as 'f32')
    mode: str               # conditioning: 'none' | 'frames' | 'samples'
    cond_geom: tuple        # (hop, offset, frames per utterance) of a frame-rate condition
    cond_t: Optional[torch.Tensor]      # the per-sample condition in the form the kernels of this precision read (_cond_operand)
    plans: List[NetPlan]
    x_limit: float          # the run-time bound on the flow's input (the smallest of the plans')
    path: _Path


def _prepare_flow(nets: Sequence, x: torch.Tensor, cond, precision: Optional[str], max_workgroups: int = 0) -> _FlowPrep:
    """The preparation of a forward of `nets` (one structure) on x [N, T, C], N * T > 0: the condition checked, the plans fetched --
    in exact fp32 instead where the split-fp16 plans' pack-time bounds fail --, the launch path chosen.  Enqueues at most the
    conversion of a per-sample condition."""
    name = precision or DEFAULT_PRECISION
    prec = PRECISIONS[name]
    net0 = nets[0]
    mode, cond_geom, cond_t = _check_condition(net0, cond, x)
    if prec == _lib.PREC_F16 and (x.shape[2] != 1 or net0.use_skip_connection):
        raise _lib.PwvError("precision 'f16' supports scalar-input nets without skip accumulation only")
    plans = [get_plan(net, mode, prec) for net in nets]
    if prec == _lib.PREC_F16X3 and not all(p.f16x3_ok and p.x_limit > 0 for p in plans):
        # some weight / bound leaves fp16's exponent range: this net runs in the exact fp32 arithmetic instead
        key = tuple(net.full_scope for net in nets)
        if key not in _range_warned:
            _range_warned.add(key)
            import warnings
            warnings.warn("pwv: weights of %s exceed the range of the split-fp16 arithmetic; using precision 'f32' for it" % (key,))
        return _prepare_flow(nets, x, cond, 'f32', max_workgroups)
    x_limit = min(p.x_limit for p in plans)
    if prec == _lib.PREC_F16X3:
        _log_range('flow_input', x, x_limit, [p.range_bounds for p in plans])
    for net, plan in zip(nets, plans):
        assert plan.n_layers == len(net.dilations) and plan.with_skip == bool(net.use_skip_connection)
    if cond_t is not None:
        cond_t = _cond_operand(cond_t, prec)
    path = _choose_path(net0, plans, mode, x.shape[0], x.shape[1], max_workgroups, cond_geom)
    return _FlowPrep(name, mode, cond_geom, cond_t, plans, x_limit, path)


def _run_flow_persist(prep: _FlowPrep, nets, x: torch.Tensor, cond, affine_out: Optional[torch.Tensor], geom=None, stream_hist=None):
    """The whole stack of `nets` as the persistent launches of prep.path on the current stream: ([one [N, T, Q] tensor per net], whether
    `affine_out` = x*s + b was written by the launches).  `geom` and `stream_hist` as _run_stack_persist takes them."""
    plans, path = prep.plans, prep.path
    projs = _projections(cond, prep.mode, plans, prep.precision, None)
    row_stride = projs[0].stride(0)      # (all nets' columns where project_all's one GEMM made them, else 128 * L)
    bufs = _causal_front(x, nets[0], plans, path, prep.x_limit)
    outs = [torch.empty((x.shape[0], x.shape[1], nets[0].out_channels), dtype=torch.float32, device=x.device) for _ in nets]
    aff = (x, affine_out) if (affine_out is not None and x.shape[2] == 1) else None
    return outs, _run_stack_persist(path, nets, plans, projs, bufs, outs, x, prep.x_limit, row_stride, prep.cond_geom, aff, geom, stream_hist)


def _run_nets(nets: Sequence, x: torch.Tensor, cond, precision: Optional[str], max_workgroups: int, affine_out: Optional[torch.Tensor],
              geom=None):
    """run_nets / run_flow: ([one [N, T, Q] tensor per net], whether `affine_out` = x*s + b was written by the launches).
    With `geom` (run_flow_varlen: x = the packed batch as [1, R, 1]) only the persistent path with layer 0 and the tail inside its
    launches is taken; where that path is not the one a uniform batch of R rows would take, nothing is enqueued and None returned."""
    x = _require_cuda_f32(x, 'input_batch')
    if x.dim() != 3:
        raise ValueError('input_batch must be [N, T, C], got %s' % (tuple(x.shape),))
    n, t, qin = x.shape
    assert 1 <= len(nets) <= _lib.PWV_MAX_NETS
    net0 = nets[0]
    for other in nets[1:]:
        assert _same_structure(net0, other)
    if qin != net0.in_channels:
        raise ValueError('input has %d channels, net expects %d' % (qin, net0.in_channels))
    if n * t == 0:
        return [torch.empty((n, t, net0.out_channels), dtype=torch.float32, device=x.device) for _ in nets], False
    prep = _prepare_flow(nets, x, cond, precision, max_workgroups)
    path, plans = prep.path, prep.plans
    if geom is not None and not path.whole_flow:
        return None         # (the per-layer kernels and the causal-layer launch have no packed form)
    if path.persist:
        return _run_flow_persist(prep, nets, x, cond, affine_out, geom)
    side = _net_streams(x.device) if path.two else None
    projs = _projections(cond, prep.mode, plans, prep.precision, side)
    bufs = _causal_front(x, net0, plans, path, prep.x_limit)
    outs = [torch.empty((n, t, net0.out_channels), dtype=torch.float32, device=x.device) for _ in nets]
    _run_stack_layers(path, nets, plans, projs, bufs, outs, x, prep.x_limit, prep.cond_t, projs[0].stride(0), prep.cond_geom, max_workgroups, side)
    return outs, False


def _check_condition(net0, cond, x: torch.Tensor):
    """(conditioning mode, (hop, offset, frames per utterance) of a frame-rate condition, the per-sample condition or None)."""
    n, t = x.shape[0], x.shape[1]
    if cond is None:
        return 'none', (0, 0, 0), None
    if isinstance(cond, RepeatedCondition):
        if cond.length != t or cond.frames.shape[0] != n:
            raise ValueError('condition %s does not match input %s' % (cond.shape, tuple(x.shape)))
        if cond.frames.shape[2] != net0.condition_channels:
            raise ValueError('condition has %d channels, net expects %d' % (cond.frames.shape[2], net0.condition_channels))
        return 'frames', (cond.hop, cond.offset, cond.frames.shape[1]), None
    cond_t = _require_cuda_f32(cond, 'condition_batch')
    if tuple(cond_t.shape) != (n, t, net0.condition_channels):
        raise ValueError('condition_batch %s does not match input %s / %d channels'
                         % (tuple(cond_t.shape), tuple(x.shape), net0.condition_channels))
    return 'samples', (0, 0, 0), cond_t


def _cond_operand(cond_t: torch.Tensor, prec: int) -> torch.Tensor:
    """The per-sample condition in the form the kernels of this precision read: fp32 tile32 ('f32'), pre-split fp16 hi / lo planes
    ('f16x3': split once per forward instead of once per net-layer), fp16 blocks ('f16').  Every flow of a forward pass is handed the
    same tensor: convert it once (the entry is valid while that very tensor object is alive and has not been written to)."""
    global _cond_cache
    hit = _cond_cache
    if (hit is not None and hit[0]() is cond_t and hit[1] == cond_t._version and hit[2] == prec
            and hit[4] == torch.cuda.current_stream()):
        return hit[3]
    lib, s = _lib.lib(), _stream()
    n, t, cc = cond_t.shape
    floats = lib.pwv_tile32_floats(n * t, cc)
    if prec == _lib.PREC_F32:
        ct = torch.empty((floats,), dtype=torch.float32, device=cond_t.device)
        check(lib.pwv_rows_to_tile32_f32(_ptr(cond_t), _ptr(ct), n * t, cc, s), 'pwv_rows_to_tile32_f32')
    elif prec == _lib.PREC_F16X3:
        ct = torch.empty((2 * floats,), dtype=torch.float16, device=cond_t.device)
        check(lib.pwv_cond_split_f16(_ptr(cond_t), _ptr(ct), n, t, cc, s), 'pwv_cond_split_f16')
    else:
        ct = torch.empty((floats,), dtype=torch.float16, device=cond_t.device)
        check(lib.pwv_cond_to_f16(_ptr(cond_t), _ptr(ct), n, t, cc, s), 'pwv_cond_to_f16')
    _cond_cache = (weakref.ref(cond_t), cond_t._version, prec, ct, torch.cuda.current_stream())
    return ct


def _projections(cond, mode: str, plans, precision: Optional[str], side) -> List[torch.Tensor]:
    """P of each net: its column block of the forward's one projection GEMM (project_all), else a frame-rate GEMM of its own, or
    the bias-only row without a frame-rate condition."""
    if mode != 'frames':
        return [p.proj_b.reshape(1, -1) for p in plans]
    bank = getattr(cond, 'proj_bank', None)
    if bank is not None and all(id(p) in bank for p in plans):
        return [bank[id(p)] for p in plans]
    pname = precision or DEFAULT_PRECISION
    n, frames, _ = cond.frames.shape
    f2d = _require_cuda_f32(cond.frames, 'frames').reshape(n * frames, -1)
    if side is None:
        return [linear_op(f2d, p.proj_w, p.proj_b, relu=False, precision=pname) for p in plans]
    # two streams: net 0's P on the main stream, net 1's on its own stream: its chain then starts one small GEMM later than
    # net 0's, which keeps the two chains out of phase (they would otherwise run in lockstep and hit their launch gaps / tails together)
    projs = [linear_op(f2d, plans[0].proj_w, plans[0].proj_b, relu=False, precision=pname), None]
    side[1].wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side[1]):
        projs[1] = linear_op(f2d, plans[1].proj_w, plans[1].proj_b, relu=False, precision=pname)
    return projs


def _causal_front(x: torch.Tensor, net0, plans, path: _Path, x_limit: float) -> List[List[torch.Tensor]]:
    """Each net's residual buffers -- the persistent launch's ring of three (pwv_persist_args.x_ring) or the per-layer path's
    ping-pong pair -- with the causal layer's output (modules.py:174-183) in buffer 0.  Where layer 0 rebuilds that output from
    the scalar input itself (path.first_fused, pwv_layer_args.x_first) the [rows, 64] front buffer is neither written nor read."""
    lib, s = _lib.lib(), _stream()
    n, t, qin = x.shape
    rows, R, G, prec = n * t, net0.residual_channels, len(plans), plans[0].precision
    half = prec == _lib.PREC_F16
    if path.persist:
        bufs = [list(torch.empty((3, lib.pwv_tile32_floats(rows, R)), dtype=torch.float32, device=x.device).unbind(0)) for _ in plans]
    else:
        bufs = [[torch.empty((lib.pwv_tile32_floats(rows, R),), dtype=torch.float16 if half else torch.float32, device=x.device)
                 for _ in range(2)] for _ in plans]
    if path.first_fused:
        return bufs
    if prec == _lib.PREC_F16X3:
        range_check_op(x, x_limit, kind=None)          # (layer 0 checks its scalar input itself when it rebuilds the causal layer)
    if qin == 1:
        filt = (c_void_p * G)(*[p.causal_filter.data_ptr() for p in plans])
        hout = (c_void_p * G)(*[b[0].data_ptr() for b in bufs])
        front = lib.pwv_iaf_front_f16 if half else lib.pwv_iaf_front_f32
        check(front(_ptr(x), None, None, 1, None, G, filt, hout, n, t, net0.filter_width, R, s), 'pwv_iaf_front')
        for g, p in enumerate(plans):
            if p.causal_bias is not None:      # normalize='bn': the shift of the batch norm behind the causal layer (modules.py:182)
                if half:
                    raise _lib.PwvError("precision 'f16' does not support normalize='bn'")
                channel_affine_op(bufs[g][0], None, p.causal_bias, tile32_rows=rows, channels=R, out=bufs[g][0])
    else:
        for g, p in enumerate(plans):      # multi-channel input: generic causal conv, then into tile32
            hrows = torch.empty((n, t, R), dtype=torch.float32, device=x.device)
            check(lib.pwv_causal_conv_f32(_ptr(x), _ptr(p.causal_filter), _ptr(hrows), n, t, qin, R,
                                          net0.filter_width, 1, s), 'pwv_causal_conv_f32')
            check(lib.pwv_rows_to_tile32_f32(_ptr(hrows), _ptr(bufs[g][0]), rows, R, s), 'pwv_rows_to_tile32_f32')
    return bufs


def _run_stack_layers(path: _Path, nets, plans, projs, bufs, outs, x, x_limit, cond_t, row_stride, cond_geom, max_workgroups, side):
    """The whole stack + head as per-layer launches in ONE C call (pwv_wavenet_stack_f32; over two side streams where path.two)."""
    lib, s = _lib.lib(), _stream()
    G, L, prec = len(nets), plans[0].n_layers, plans[0].precision
    net0 = nets[0]
    n, t = x.shape[0], x.shape[1]
    use_skip = bool(net0.use_skip_connection)
    skips = [torch.empty((lib.pwv_tile32_floats(n * t, net0.skip_channels),), dtype=torch.float32, device=x.device)
             for _ in nets] if use_skip else None
    main = torch.cuda.current_stream()
    if path.two:
        for g in range(2):
            side[g].wait_stream(main)
    sa = StackArgs()
    sa.G, sa.n_layers, sa.Q, sa.N, sa.T = G, L, net0.out_channels, n, t
    sa.dilations = (ctypes.c_int * L)(*[int(d) for d in net0.dilations])
    for g in range(G):
        sa.buf0[g], sa.buf1[g] = bufs[g][0].data_ptr(), bufs[g][1].data_ptr()
        sa.packed_layers[g] = plans[g].packed_layers.data_ptr()
        sa.proj[g] = projs[g].data_ptr()
        sa.skip[g] = skips[g].data_ptr() if use_skip else None
        sa.packed_head[g] = plans[g].packed_head.data_ptr()
        sa.out[g] = outs[g].data_ptr()
    sa.packed_layer_stride, sa.proj_row_stride = plans[0].layer_floats, row_stride
    sa.cond, sa.cond_channels = _ptr(cond_t), (net0.condition_channels if cond_t is not None else 0)
    sa.cond_hop, sa.cond_offset, sa.cond_frames = cond_geom
    sa.precision, sa.max_workgroups, sa.separate_head = prec, max_workgroups, 0 if FUSE_HEAD else 1
    if path.first_fused:
        _set_x_first(sa, plans, x, x_limit)
    streams = (c_void_p * 2)(side[0].cuda_stream if path.two else s.value, side[1].cuda_stream if path.two else None)
    evs = []
    if EVENT_LOG is not None and L > 1:
        # bench.py's live kernel timing: the library records one event pair per chain around its run of residual-layer
        # launches (pwv_stack_args.ev_begin / ev_end) -- the production launch path plus two event records
        for c, so in enumerate(side[:2] if path.two else [main]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(so)       # materialises the hipEvent_t handles; the library re-records them
            e1.record(so)
            sa.ev_begin[c], sa.ev_end[c] = e0.cuda_event, e1.cuda_event
            evs.append((e0, e1))
    check(lib.pwv_wavenet_stack_f32(ctypes.byref(sa), streams), 'pwv_wavenet_stack_f32')
    for e0, e1 in evs:
        EVENT_LOG.append(('layer_residual', e0, e1, 1 if path.two else G, L - 1))
    if path.two:
        for g in range(2):
            main.wait_stream(side[g])


# ---- streaming: a flow on one CHUNK of N sessions (include/pwv_hip.h "STREAMING"; stream.StreamingVocoder owns the sessions) ---------
_STREAM_STRUCTURE_WHY = {'samples': 'per-sample (transposed-conv) conditioning',
                         'frames': 'per_sample=True without a per-sample condition (a [N, T, C] tensor at sample rate)', 'skip': 'skip accumulation (use_skip_connection)',
                         'noskip': 'skip=True does not match these nets: they have no skip accumulation (use_skip_connection is False)',
                         'f16': "precision 'f16' (the fp16 storage mode)",
                         'shape': 'a net outside the fused shape (two scalar-input nets per flow, W = 2, R = D = 64, S = 128, no normaliser, at least 2 layers)'}


def stream_refusal(nets, cond, precision: Optional[str] = None, per_sample: bool = False, skip: bool = False) -> Optional[str]:
    """Why a flow (its nets) has no streaming form -- or None.  The per-layer kernels stream in three forms only: layer 0 folded onto
    its scalar input, a plain residual layer, the last layer with the head fused behind it.  Two flow shapes stream (_flow_structure):
    two nets of one output each, and one shared net of two outputs (its launches carry G = 1 and a head / tail of Q = 2).
    per_sample=True: the same question for the streaming forms with a per-sample condition (pwv_wavenet_layer_stream_cond_f32: layer 0
    folded, a plain residual layer, the last layer gated with the head launch behind it); `cond` is then the [N, T, C] tensor, or the
    PackedSampleCondition of a ragged chunk.
    skip=True: the same question for the streaming forms with skip accumulation (pwv_iaf_front_stream_f32, then
    pwv_wavenet_layer_stream_skip_f32 per layer and the head launch on the skip sum); not together with per_sample."""
    net0 = nets[0]
    if skip and per_sample:
        return 'skip=True together with per_sample=True: skip accumulation with a per-sample condition has no streaming form'
    if _instance_norm(nets):
        return "instance normalisation ('in'): its statistics span the whole time axis"
    key = _flow_structure(nets, cond, precision, per_sample, skip)
    if key is None and (net0.normalize or len(net0.dilations) < 2):       # (_flow_structure has settled the nets: two of one output or one of two)
        key = 'shape'
    if key is not None:
        return _STREAM_STRUCTURE_WHY[key]
    if not skip and not (FOLD_FIRST and FUSE_FIRST and FUSE_HEAD):      # (a skip stream has its front and its head as launches of their own)
        return 'PWV_FOLD_FIRST=0 / FUSE_FIRST / FUSE_HEAD off: layer 0 streams folded and the head fused only'
    return None


def _prepare_flow_stream(nets, x: torch.Tensor, cond, precision: Optional[str], skip: bool = False) -> _FlowPrep:
    """_prepare_flow for a streaming flow: layer 0 streams in its folded form only (skip: behind the streaming front, not folded)."""
    prep = _prepare_flow(nets, x, cond, precision)
    if not skip and any(p.first_fold is None for p in prep.plans):
        raise _lib.PwvError('run_flow_stream: no streaming form: layer 0 has no folded form for these weights')
    return prep


# the exact-fp32 instantiations of the ragged kernel (stack_persist_ragged_kernel<true, MODE>) are built: they are spill-free at 256 VGPRs
# (tests/test_stream_varlen_host.py reads the compiler's remarks); False would route f32 ragged pushes to the grouped route
RAGGED_F32 = True


def ragged_cond_rows(cu_frames_i: int, t: int, hop: int):
    """(host arithmetic of the ragged per-sample route) The rows of the UNCROPPED packed condition -- hop rows per packed frame, frame f
    at rows hop f .. hop f + hop - 1 -- that are the condition of a session whose frames start at packed frame cu_frames_i and whose
    chunk has t samples: sample s reads row hop cu_frames_i + hop / 2 + s, the session's own crop [hop/2 : hop/2 + t] (models.py:124).
    A crop of the packed tensor as a whole would be wrong for every session but the first: each session owns one frame more than t / hop."""
    import numpy as np
    return np.arange(hop * int(cu_frames_i) + hop // 2, hop * int(cu_frames_i) + hop // 2 + int(t))


class PackedSampleCondition(object):
    """The per-sample condition of a RAGGED chunk: `full` [F hop, C], the transposed convolutions' output over the packed frames, uncropped
    (every row depends on its own frame alone, so the stages run once per tick); a group of sessions gathers its rows (ragged_cond_rows)."""

    def __init__(self, full: torch.Tensor, hop: int):
        self.full, self.hop = full, int(hop)

    @property
    def shape(self):
        return tuple(self.full.shape)


class _StreamGroup(object):
    """The sessions of a ragged push that share one chunk length (the grouped route of run_flow_stream): their rows and frames in the
    packed tensors (device index vectors) and their rows of the slot table."""

    def __init__(self, geom, tab: torch.Tensor, t: int, members: Sequence[int]):
        import numpy as np
        fr = t // geom.hop + 1
        self.t, self.n, self.frames = t, len(members), fr
        self.first_frames = [geom.cu_frames_host[i] for i in members]
        self.rows_idx = geom._upload(np.concatenate([np.arange(geom.cu_rows_host[i], geom.cu_rows_host[i] + t) for i in members]), torch.int64)
        self.frames_idx = geom._upload(np.concatenate([np.arange(geom.cu_frames_host[i], geom.cu_frames_host[i] + fr) for i in members]), torch.int64)
        self.tab = tab.index_select(0, geom._upload(list(members), torch.int64)).contiguous()
        self._cond = None

    def condition(self, cond, geom):
        """The group's [n, t / hop + 1, C] frames of the packed condition, with their rows of its projection bank (the prologue is per
        frame: a gathered row holds the bits the group's own prologue would compute); made once per condition object."""
        if cond is None:
            return None
        if self._cond is not None and self._cond[0]() is cond:
            return self._cond[1]
        if isinstance(cond, PackedSampleCondition):      # the members' own crops of the uncropped packed condition: [n, t, C]
            import numpy as np
            idx = geom._upload(np.concatenate([ragged_cond_rows(f0, self.t, cond.hop) for f0 in self.first_frames]), torch.int64)
            out = cond.full.index_select(0, idx).reshape(self.n, self.t, cond.full.shape[1])
            self._cond = (weakref.ref(cond), out)
            return out
        c = cond.frames.shape[2]
        out = RepeatedCondition(cond.frames.reshape(geom.total_frames, c).index_select(0, self.frames_idx).reshape(self.n, self.frames, c),
                                cond.hop, cond.offset, self.t)
        bank = getattr(cond, 'proj_bank', None)
        if bank is not None:
            out.proj_bank = _remap_bank(bank, geom.total_frames, lambda full: full.index_select(0, self.frames_idx))
        self._cond = (weakref.ref(cond), out)
        return out


def stream_groups(geom: 'VarlenGeometry', tab: torch.Tensor) -> List[_StreamGroup]:
    """The groups of equal chunk length of a ragged push (first appearance first), made once per push and kept on its geometry."""
    groups = getattr(geom, '_stream_groups', None)
    if groups is None:
        by_t = {}
        for i, t in enumerate(geom.lengths):
            by_t.setdefault(t, []).append(i)
        groups = geom._stream_groups = [_StreamGroup(geom, tab, t, members) for t, members in by_t.items()]
    return groups


def _run_flow_stream_ragged(nets, x, cond, precision, hist, scalar_off, row_off, geom, slot_tab, per_sample=False, skip=False):
    """run_flow_stream on a ragged chunk (geom: session i has geom.lengths[i] rows of the packed x [R, 1]; route 4 of DESIGN.md section 9
    "Routes").  The launches, chosen once per flow:
      * the PACKED streaming persistent launches (pwv_persist_args.cu_rows with hist->cu_rows, stack_persist_ragged_kernel) where a uniform
        forward of R rows takes persistent runs with the tail and the fused, folded layer 0 and every session has >= 32 rows
        (varlen_fallback_reason);
      * else the GROUPED route: the sessions grouped by chunk length, each group the uniform streaming flow (persistent or per layer, as
        run_flow_stream decides for it) on its own rows of x, its own frames and its own rows of the slot table, scattered back.
    Same bits: a session's rows do not depend on which sessions were advanced with it.  EVENT_LOG gets ('stream_ragged', None, None,
    'packed' | 'grouped', why, groups) ahead of the route's own entries.
    per_sample (cond a PackedSampleCondition): the grouped route only -- the packed route is the persistent kernel, which cannot host a
    per-sample condition.  skip: the grouped route only, for the same reason (the persistent launch has no skip accumulators)."""
    x = _require_cuda_f32(x, 'input')
    if x.dim() != 2 or tuple(x.shape) != (geom.rows, 1):
        raise ValueError('input must be the packed chunk [%d, 1], got %s' % (geom.rows, tuple(x.shape)))
    if skip:
        why = 'skip accumulation (the packed route is the persistent launch)'
    else:
        why = 'per-sample conditioning (the packed route is the persistent launch)' if per_sample else varlen_fallback_reason(nets, cond, geom, precision)
    if why is None:
        x3 = x.reshape(1, geom.rows, 1)
        prep = _prepare_flow_stream(nets, x3, cond, precision)
        if prep.precision == 'f32' and not RAGGED_F32:
            why = "the ragged kernel is not built for precision 'f32'"
        elif prep.path.whole_flow:
            if EVENT_LOG is not None:
                EVENT_LOG.append(('stream_ragged', None, None, 'packed', None, 1))
            out = torch.empty_like(x3)
            hist.scalar_off, hist.cu_rows = scalar_off, _ptr(geom.cu_rows)
            try:
                outs, done = _run_flow_persist(prep, nets, x3, cond, out, geom, (hist, row_off))
            finally:
                hist.cu_rows = None
            return (out if done else _flow_affine(x3, outs)).reshape(geom.rows, 1)
        else:
            why = 'the library plans this stack per layer at %d rows' % geom.rows
    groups = stream_groups(geom, slot_tab)
    if EVENT_LOG is not None:
        EVENT_LOG.append(('stream_ragged', None, None, 'grouped', why, len(groups)))
    out = torch.empty_like(x)
    for grp in groups:
        hg = _lib.StreamArgs()
        ctypes.memmove(ctypes.addressof(hg), ctypes.addressof(hist), ctypes.sizeof(_lib.StreamArgs))
        hg.slot_tab, hg.cu_rows = grp.tab.data_ptr(), None
        yg = run_flow_stream(nets, x.index_select(0, grp.rows_idx).reshape(grp.n, grp.t, 1), grp.condition(cond, geom), precision, hg,
                             scalar_off, row_off, per_sample=per_sample, skip=skip)
        out.index_copy_(0, grp.rows_idx, yg.reshape(grp.n * grp.t, 1))
    return out


def run_flow_stream(nets: Sequence, x: torch.Tensor, cond, precision: Optional[str], hist: _lib.StreamArgs, scalar_off: int,
                    row_off, geom=None, slot_tab: Optional[torch.Tensor] = None, per_sample: bool = False, skip: bool = False) -> torch.Tensor:
    """One IAF flow on a chunk: x [N, T, 1] = the T samples that follow what each of the N sessions has seen, `cond` the chunk's own
    frames (a RepeatedCondition of T / hop + 1 frames per session).  `hist` carries the history blocks and the slot table of the call
    (read / written block per session); `scalar_off` and `row_off[g][j]` (j >= 1) say where this flow's histories lie in a block.
    The launches (route 3 of DESIGN.md section 9 "Routes"), chosen once per flow, all on the current stream:
      * the persistent STREAMING launches (pwv_persist_args.hist; the affine inside the last one: one launch per run of
        _persist_runs, one for a stack of up to PERSIST_MAX_LAYERS + 1 layers) where _choose_path gives an [N, T] forward persistent
        runs with the tail and the fused, folded layer 0 -- PERSIST not False, not suspended, rows <= PERSIST_AUTO_MAX_ROWS, L >= 4;
      * else L streaming layer launches of all the flow's nets (G = 2, or G = 1 with a head of two outputs for a shared net), then the
        affine (PWV_PERSIST=0 keeps this route in use and tested).
    Same bits, same written history rows either way.  Only enqueues, like run_flow; the written blocks become the sessions' state
    when the caller flips their generation -- so a push whose persistent launch gave up is rerun by verified_call on the per-layer
    launches (persist_suspended()) from the same generation.
    With `geom` (a VarlenGeometry) the chunk is RAGGED: session i brings geom.lengths[i] rows, x is the packed [R, 1], `cond` spans the
    packed frames (geom.frames[i] per session) and `slot_tab` is the device int32 [N, 2] table hist.slot_tab points at
    (_run_flow_stream_ragged: packed persistent launches, else the sessions grouped by length on the routes above).
    per_sample=True (a transposed-conv model's stream): `cond` is the chunk's condition at sample rate, [N, T, C] -- a PackedSampleCondition
    for a ragged chunk -- and the flow is L calls of pwv_wavenet_layer_stream_cond_f32, the head launch and the affine
    (_run_flow_stream_cond); the persistent launch cannot host a per-sample condition.
    skip=True (a stream of a model with use_skip_connection): the flow is the streaming front, L calls of
    pwv_wavenet_layer_stream_skip_f32 on a per-chunk skip accumulator, the head launch on the skip sum and the affine
    (_run_flow_stream_skip); `scalar_off` is then the ONE scalar x[-1] of the front and row_off[g][0] layer 0's row history."""
    why = stream_refusal(nets, cond, precision, per_sample=per_sample, skip=skip)
    if why is not None:
        raise _lib.PwvError('run_flow_stream: no streaming form: ' + why)
    if geom is not None:
        return _run_flow_stream_ragged(nets, x, cond, precision, hist, scalar_off, row_off, geom, slot_tab, per_sample, skip)
    x = _require_cuda_f32(x, 'input')
    prep = _prepare_flow_stream(nets, x, cond, precision, skip)
    if skip:
        return _run_flow_stream_skip(prep, nets, x, cond, hist, scalar_off, row_off)
    if per_sample:
        return _run_flow_stream_cond(prep, nets, x, hist, scalar_off, row_off)
    if prep.path.whole_flow:
        hist.scalar_off = scalar_off
        out = torch.empty_like(x)
        outs, done = _run_flow_persist(prep, nets, x, cond, out, None, (hist, row_off))
        return out if done else _flow_affine(x, outs)
    lib, s = _lib.lib(), _stream()
    net0, plans = nets[0], prep.plans
    n, t, _ = x.shape
    G, L = len(plans), plans[0].n_layers
    if EVENT_LOG is not None:
        EVENT_LOG.append(('layer_stream', None, None, G, L))      # L calls of pwv_wavenet_layer_stream_f32 + the affine
    projs = _projections(cond, prep.mode, plans, prep.precision, None)
    outs = [torch.empty((n, t, net0.out_channels), dtype=torch.float32, device=x.device) for _ in plans]
    bufs = [[torch.empty((lib.pwv_tile32_floats(n * t, 64),), dtype=torch.float32, device=x.device) for _ in range(2)] for _ in plans]
    for j in range(L):
        la = _layer_args(net0, plans, projs, projs[0].stride(0), prep.cond_geom, bufs, j, (j + 1) & 1, j & 1, x)
        la.out_mode = _lib.OUT_GATED if j == L - 1 else _lib.OUT_RESIDUAL
        if j == 0:
            _set_x_first(la, plans, x, prep.x_limit)
            hist.scalar_off = scalar_off
        else:
            for g in range(G):
                hist.row_off[g] = row_off[g][j]
        if j == L - 1:
            for g in range(G):
                la.head_packed[g], la.head_out[g] = plans[g].packed_head.data_ptr(), outs[g].data_ptr()
            la.head_q = net0.out_channels
        check(lib.pwv_wavenet_layer_stream_f32(ctypes.byref(la), ctypes.byref(hist), s), 'pwv_wavenet_layer_stream_f32')
    return _flow_affine(x, outs)


def _run_flow_stream_cond(prep: _FlowPrep, nets, x: torch.Tensor, hist: _lib.StreamArgs, scalar_off: int, row_off) -> torch.Tensor:
    """run_flow_stream with a per-sample condition ("Streaming transposed-conv conditioning"): L streaming layer
    launches of all the flow's nets with the condition GEMM inside (pwv_wavenet_layer_stream_cond_f32; prep.cond_t is the chunk's
    condition as the kernels of this arithmetic read it, P the bias-only row, as in the one-shot 'samples' mode), the last one with gated
    output; the head launch on it -- the fused head has no room for the condition weights --; the affine."""
    lib, s = _lib.lib(), _stream()
    net0, plans = nets[0], prep.plans
    n, t, _ = x.shape
    G, L = len(plans), plans[0].n_layers
    assert prep.mode == 'samples' and prep.cond_t is not None
    if EVENT_LOG is not None:
        EVENT_LOG.append(('layer_stream_cond', None, None, G, L))      # L calls of pwv_wavenet_layer_stream_cond_f32 + the head + the affine
    projs = _projections(None, prep.mode, plans, prep.precision, None)
    outs = [torch.empty((n, t, net0.out_channels), dtype=torch.float32, device=x.device) for _ in plans]
    bufs = [[torch.empty((lib.pwv_tile32_floats(n * t, 64),), dtype=torch.float32, device=x.device) for _ in range(2)] for _ in plans]
    for j in range(L):
        la = _layer_args(net0, plans, projs, projs[0].stride(0), prep.cond_geom, bufs, j, (j + 1) & 1, j & 1, x)
        la.cond, la.cond_channels = _ptr(prep.cond_t), net0.condition_channels
        la.out_mode = _lib.OUT_GATED if j == L - 1 else _lib.OUT_RESIDUAL
        if j == 0:
            _set_x_first(la, plans, x, prep.x_limit)
            hist.scalar_off = scalar_off
        else:
            for g in range(G):
                hist.row_off[g] = row_off[g][j]
        check(lib.pwv_wavenet_layer_stream_cond_f32(ctypes.byref(la), ctypes.byref(hist), s), 'pwv_wavenet_layer_stream_cond_f32')
    ha = _lib.HeadArgs()
    ha.G, ha.N, ha.T, ha.Q = G, n, t, net0.out_channels
    ha.in_mode, ha.precision = _lib.HEAD_IN_GATED, plans[0].precision
    for g, p in enumerate(plans):
        ha.in_[g], ha.packed[g], ha.out[g] = bufs[g][(L - 1) & 1].data_ptr(), p.packed_head.data_ptr(), outs[g].data_ptr()
    check(lib.pwv_wavenet_head_f32(ctypes.byref(ha), s), 'pwv_wavenet_head_f32')
    return _flow_affine(x, outs)


def _run_flow_stream_skip(prep: _FlowPrep, nets, x: torch.Tensor, cond, hist: _lib.StreamArgs, scalar_off: int, row_off) -> torch.Tensor:
    """run_flow_stream with skip accumulation ("Streaming the skip-connection architecture"): the launches of the
    one-shot skip forward (_causal_front + pwv_wavenet_stack_f32) with the look-back of a stream.  The streaming front writes the causal
    layer's rows of the chunk (x[-1] from the session's scalar at `scalar_off`); L streaming layer launches of all the flow's nets add
    their skip contributions, in layer order, to the CHUNK's accumulators -- pwv_tile32_floats(n t, 128) floats per net: the skip sum is
    row-local and has no history --, layer 0 on a row history like the others (row_off[g][0]), the last one with gated output; the head
    launch reads the skip sum; the affine."""
    lib, s = _lib.lib(), _stream()
    net0, plans = nets[0], prep.plans
    n, t, _ = x.shape
    G, L = len(plans), plans[0].n_layers
    assert prep.mode != 'samples' and all(p.with_skip for p in plans)
    if EVENT_LOG is not None:
        EVENT_LOG.append(('layer_stream_skip', None, None, G, L))      # the front + L calls of pwv_wavenet_layer_stream_skip_f32 + the head + the affine
    if plans[0].precision == _lib.PREC_F16X3:
        range_check_op(x, prep.x_limit, kind=None)      # (as _causal_front: no layer reads the scalar input itself)
    projs = _projections(cond, prep.mode, plans, prep.precision, None)
    outs = [torch.empty((n, t, net0.out_channels), dtype=torch.float32, device=x.device) for _ in plans]
    bufs = [[torch.empty((lib.pwv_tile32_floats(n * t, 64),), dtype=torch.float32, device=x.device) for _ in range(2)] for _ in plans]
    skips = [torch.empty((lib.pwv_tile32_floats(n * t, net0.skip_channels),), dtype=torch.float32, device=x.device) for _ in plans]
    hist.scalar_off = scalar_off
    filt = (c_void_p * G)(*[p.causal_filter.data_ptr() for p in plans])
    hout = (c_void_p * G)(*[b[0].data_ptr() for b in bufs])
    check(lib.pwv_iaf_front_stream_f32(_ptr(x), G, filt, hout, n, t, ctypes.byref(hist), s), 'pwv_iaf_front_stream_f32')
    for j in range(L):
        la = _layer_args(net0, plans, projs, projs[0].stride(0), prep.cond_geom, bufs, j, j & 1, (j + 1) & 1, x)
        la.out_mode = _lib.OUT_GATED if j == L - 1 else _lib.OUT_RESIDUAL
        la.skip_init = 1 if j == 0 else 0
        for g in range(G):
            la.skip[g] = skips[g].data_ptr()
            hist.row_off[g] = row_off[g][j]
        check(lib.pwv_wavenet_layer_stream_skip_f32(ctypes.byref(la), ctypes.byref(hist), s), 'pwv_wavenet_layer_stream_skip_f32')
    ha = _lib.HeadArgs()
    ha.G, ha.N, ha.T, ha.Q = G, n, t, net0.out_channels
    ha.in_mode, ha.precision = _lib.HEAD_IN_SKIPSUM, plans[0].precision
    for g, p in enumerate(plans):
        ha.in_[g], ha.packed[g], ha.out[g] = skips[g].data_ptr(), p.packed_head.data_ptr(), outs[g].data_ptr()
    check(lib.pwv_wavenet_head_f32(ctypes.byref(ha), s), 'pwv_wavenet_head_f32')
    return _flow_affine(x, outs)
