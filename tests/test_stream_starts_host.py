"""CPU: the host side of STARTS inside a graphed ragged tick (include/pwv_hip.h, "STARTS"; csrc/pwv_stream_tick.hip; graph.GraphedRaggedStream
.tick(starts=)): the grown args struct against its ctypes mirror with everything else of the ABI where it was, the new refusals, the numpy
restatement of the two starts kernels against what reset + push_varlen / _commit do on the host for random mixes of fresh, running and
restarting sessions, the compiler's resource remarks for the two new kernels, and the argument errors of tick()."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests.test_stream_ragged_graph_host import _args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('pwv_stream_tick_ragged_begin', 'pwv_stream_tick_ragged_commit')
OLD_SIZE = 120          # pwv_stream_tick_ragged_args without starts, first and zero_block: the offset of `starts`


def test_grown_struct_and_the_frozen_rest(built_lib, tmp_path):
    """The C compiler's size and offsets of pwv_stream_tick_ragged_args, the three trailing fields included, equal the ctypes mirror's;
    the uniform tick's struct is 112 bytes, the version 301 and the library's symbols 52, as they were."""
    from pwv_amd import _lib
    from tests.util import c_struct_probe
    S = _lib.StreamTickRaggedArgs
    fields = [f[0] for f in S._fields_]
    assert fields[0] == 'struct_size' and fields[-3:] == ['starts', 'first', 'zero_block']
    got = c_struct_probe('pwv_stream_tick_ragged_args', fields, tmp_path, extra=['sizeof(pwv_stream_tick_args)'])
    assert got == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in fields] + [112, 301]
    assert S.starts.offset == OLD_SIZE and ctypes.sizeof(S) == 144 and S().struct_size == 144
    assert ctypes.sizeof(_lib.StreamTickArgs) == 112
    assert built_lib.pwv_version() == _lib.HEADER_VERSION == 301
    assert len(_lib.EXPORTED_SYMBOLS) == len(set(_lib.EXPORTED_SYMBOLS)) == 52
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'pwv_hip.h')).read(), flags=re.S)
    assert len(set(re.findall(r'\b(pwv_\w+)\s*\(', header))) == 52          # no new entry point in the header either


@pytest.mark.parametrize('symbol', SYMBOLS)
def test_refusals_of_starts_name_their_field(built_lib, symbol):
    """starts without first, and a zero block that is a session's block: refused before a device is needed (the addresses are made
    up); so is a struct shorter than the one without the new fields."""
    fn = getattr(built_lib, symbol)
    for fields, named in (({'starts': 0xb0000, 'first': None, 'zero_block': 8}, b'first'),
                          ({'starts': 0xb0000, 'first': 0xc0000, 'zero_block': 7}, b'zero_block'),
                          ({'starts': 0xb0000, 'first': 0xc0000, 'zero_block': 0}, b'zero_block'),
                          ({'starts': 0xb0000, 'first': 0xc0000, 'zero_block': -1}, b'zero_block'),
                          ({'starts': 0xb0000, 'first': 0xc0000, 'zero_block': 8, 'struct_size': 16}, b'struct_size'),
                          ({'struct_size': OLD_SIZE - 8}, b'struct_size')):
        assert fn(ctypes.byref(_args(**fields)), None) == -1, fields
        err = built_lib.pwv_last_error()
        assert named in err and symbol.encode() in err, (fields, err)


@pytest.mark.parametrize('symbol,planted,named', [('pwv_stream_tick_ragged_begin', {'cu_frames': None}, b'cu_frames'),
                                                  ('pwv_stream_tick_ragged_commit', {'in_frames': 1 << 30}, b'2^31')])
def test_the_struct_at_its_old_size_is_accepted(built_lib, symbol, planted, named):
    """A caller compiled against the struct without the three fields: struct_size = 120 passes the size check, as does the grown struct
    and a longer one.  Nothing may be launched on these made-up addresses, so each call carries one planted fault that the library
    looks at only after the size: that is the refusal it names.  (That the fields behind the caller's size are read as zero is shown
    on the device: tests/test_gpu_stream_starts.py.)"""
    fn = getattr(built_lib, symbol)
    for size in (OLD_SIZE, OLD_SIZE + 8, 144, 4096):
        ta = _args(struct_size=size, **planted)
        assert fn(ctypes.byref(ta), None) == -1
        err = built_lib.pwv_last_error()
        assert named in err and b'struct_size' not in err, (size, err)
    # a struct that ends between the fields holds the ones in front of its end: starts (128 bytes) but no first, which reads as NULL
    ta = _args(struct_size=OLD_SIZE + 8, starts=0xb0000, first=0xc0000, zero_block=8)
    assert fn(ctypes.byref(ta), None) == -1 and b'first' in built_lib.pwv_last_error()


# ---- the restatement against reset + push_varlen on the host ---------------------------------------------------------------------------
class _HostStream(object):
    """The host bookkeeping of StreamingVocoder without a device, fresh and running sessions mixed: `reset`, `push_tables` -- what
    push_varlen builds (ragged_plan, the packed mel with a kept frame in front of a RUNNING session's frames only, stream_table, the
    slot table) -- and `commit`, what _commit's closure does."""

    def __init__(self, rng, n_slots, n_mels, hop):
        self.hop = hop
        self.running = [bool(v) for v in rng.integers(0, 2, n_slots)]
        self.gen = [int(v) if r else 0 for v, r in zip(rng.integers(0, 2, n_slots), self.running)]
        self.emitted = [int(v) * hop if r else 0 for v, r in zip(rng.integers(1, 1000, n_slots), self.running)]
        self.seed = [int(v) for v in rng.integers(0, 1 << 63, n_slots)]
        self.kept = rng.uniform(-1, 1, (n_slots, n_mels)).astype(np.float32)

    def sess(self):
        from pwv_amd import engine
        return np.array([[g, e, engine.as_int64_bits(sd), 0] for g, e, sd in zip(self.gen, self.emitted, self.seed)], np.int64)

    def reset(self, s, seed):
        self.gen[s], self.running[s], self.emitted[s], self.seed[s] = 0, False, 0, seed

    def push_tables(self, slots, mels):
        from pwv_amd import engine, stream
        fresh = [not self.running[s] for s in slots]
        plan = stream.ragged_plan([m.shape[0] for m in mels], fresh, self.hop)
        assert plan.launch == list(range(len(slots)))
        geom = engine.VarlenGeometry(plan.samples, self.hop, 'cpu')
        table = geom.stream_table([(self.seed[s], self.emitted[s]) for s in slots]).numpy()
        tab = np.array([[2 * s + self.gen[s], 2 * s + 1 - self.gen[s]] for s in slots], np.int32)
        mel = np.concatenate([p for s, m, fr in zip(slots, mels, fresh) for p in (([] if fr else [self.kept[s:s + 1]]) + [m])])
        return plan.samples, tab, table, np.asarray(plan.cu_rows, np.int32), np.asarray(plan.cu_frames, np.int32), mel

    def commit(self, slots, samples, last):
        for i, s in enumerate(slots):
            self.gen[s] ^= 1
            self.running[s] = True
            self.emitted[s] += samples[i]
        self.kept[slots] = last


@pytest.mark.parametrize('hop', [80, 16, 96])
def test_restatement_equals_reset_and_push_varlen(hop):
    """Random mixes of fresh sessions that start, running sessions that go on and running sessions that are cut off and start again:
    ragged_tick_begin_tables with starts gives the cu_rows, cu_frames, stream table and packed mel that reset + push_varlen build on the
    host, and their slot table except that a starting entry READS the zero block (and writes 2 s + 1 - g of the generation the device
    table holds, which is the host's block wherever that generation is 0, as after a reset); ragged_tick_commit gives the effect of
    _commit -- the generation apart, for the same reason -- and nothing with a word raised.  Without starts both are what they were."""
    from pwv_amd import engine, graph, stream
    n_mels = 8
    min_frames = graph.packed_filler_rows(hop) // hop
    rng = np.random.default_rng(1000 + hop)
    kinds = set()
    for n_slots in (1, 2, 5, 9):
        for _ in range(8):
            host = _HostStream(rng, n_slots, n_mels, hop)
            zero_block = 2 * n_slots + int(rng.integers(0, 3))
            k = int(rng.integers(1, n_slots + 1))
            slots = [int(s) for s in rng.permutation(n_slots)[:k]]
            # a fresh slot has to start; a running one restarts now and then
            restart = [host.running[s] and bool(rng.integers(0, 2)) for s in slots]
            starting = [not host.running[s] or r for s, r in zip(slots, restart)]
            kinds.update(('fresh' if not host.running[s] else 'restart' if r else 'running') for s, r in zip(slots, restart))
            counts = [int(f) for f in rng.integers(min_frames, min_frames + 9, k)]          # the frames that bring samples
            mels = [rng.uniform(-1, 1, (f + (1 if st else 0), n_mels)).astype(np.float32) for f, st in zip(counts, starting)]
            seeds = [int(v) for v in rng.integers(0, 1 << 63, k)]
            seeds[0] = (1 << 63) + 11          # the top bit set: carried as the int64 with the same bits
            sess0, kept0 = host.sess(), host.kept.copy()
            gen0 = list(host.gen)
            entries = [[s, 1, f, 0] for s, f in zip(slots, counts)]
            starts = np.array([[int(rng.integers(1, 9)) if st else 0, engine.as_int64_bits(sd) if st else int(rng.integers(-99, 99))]
                               for st, sd in zip(starting, seeds)], np.int64)
            first = np.stack([m[0] if st else rng.uniform(5, 6, n_mels).astype(np.float32) for m, st in zip(mels, starting)])
            mel = np.concatenate([m[1:] if st else m for m, st in zip(mels, starting)])
            got = stream.ragged_tick_begin_tables(sess0, kept0, entries, mel, hop, min_frames, starts=starts, first=first, zero_block=zero_block)
            # the host: reset + push_varlen
            for s, st, sd in zip(slots, starting, seeds):
                if st:
                    host.reset(s, sd)
            samples, tab, table, cu_rows, cu_frames, packed = host.push_tables(slots, mels)
            assert samples == [f * hop for f in counts]
            for name, g, w in zip(('streams', 'cu_rows', 'cu_frames', 'chunk'), got[1:], (table, cu_rows, cu_frames, packed)):
                assert g.dtype == w.dtype and np.array_equal(g, w), name
            for i, (s, st) in enumerate(zip(slots, starting)):
                assert got[0][i, 0] == (zero_block if st else tab[i, 0])
                assert got[0][i, 1] == 2 * s + 1 - gen0[s] and (gen0[s] != 0 or got[0][i, 1] == tab[i, 1])
            # a raised word: nothing changes, for a starting entry either
            for words in ((4, 0), (0, 1), (1, 1)):
                s2, k2, done = stream.ragged_tick_commit(sess0, kept0, entries, mel, hop, min_frames, words, starts=starts)
                assert not done and np.array_equal(s2, sess0) and np.array_equal(k2, kept0)
            sess1, kept1, done = stream.ragged_tick_commit(sess0, kept0, entries, mel, hop, min_frames, (0, 0), starts=starts,
                                                           first=first, zero_block=zero_block)
            host.commit(slots, samples, np.stack([m[-1] for m in mels]))
            want = host.sess()
            assert done and np.array_equal(sess1[:, 1:], want[:, 1:]) and np.array_equal(kept1, host.kept)
            for s in range(n_slots):
                assert sess1[s, 0] == (sess0[s, 0] ^ 1 if s in slots else sess0[s, 0])
                if s in slots and gen0[s] == 0:
                    assert sess1[s, 0] == want[s, 0]
            # a filler never starts, whatever its flag says; and the defaults are today's outputs
            dead = [[s, 0, f, 0] for s, f in zip(slots, counts)]
            plain = stream.ragged_tick_begin_tables(sess0, kept0, dead, mel, hop, min_frames)
            flagged = stream.ragged_tick_begin_tables(sess0, kept0, dead, mel, hop, min_frames, starts=starts, first=first, zero_block=zero_block)
            none = stream.ragged_tick_begin_tables(sess0, kept0, dead, mel, hop, min_frames, starts=np.zeros_like(starts), first=first,
                                                   zero_block=zero_block)
            assert all(np.array_equal(a, b) and np.array_equal(a, c) for a, b, c in zip(plain, flagged, none))
            s4, k4, _ = stream.ragged_tick_commit(sess0, kept0, entries, mel, hop, min_frames, (0, 0), starts=np.zeros_like(starts))
            s5, k5, _ = stream.ragged_tick_commit(sess0, kept0, entries, mel, hop, min_frames, (0, 0))
            assert np.array_equal(s4, s5) and np.array_equal(k4, k5)
    assert kinds == {'fresh', 'restart', 'running'}
    with pytest.raises(ValueError, match='zero_block'):
        stream.ragged_tick_begin_tables(sess0, kept0, entries, mel, hop, min_frames, starts=starts, first=first, zero_block=2 * n_slots - 1)


def test_garbage_in_the_starts_table_moves_no_access():
    """Garbage entries (the clamp's cases, slots out of range) with garbage starts words: every index the restatement of the two starts
    kernels touches lies inside its array, `first` included, and the slot table holds session blocks and the zero block only."""
    from pwv_amd import stream
    rng = np.random.default_rng(77)
    n_mels = 3
    for case in range(300):
        n = int(rng.integers(1, 12))
        min_frames = int(rng.integers(1, 4))
        in_frames = n * min_frames + int(rng.integers(0, 40))
        n_slots = int(rng.integers(1, 9))
        counts = np.where(rng.integers(0, 2, n) == 0, rng.integers(-2 ** 31, 2 ** 31, n), rng.integers(-5, in_frames + 3, n))
        slots = np.where(rng.integers(0, 3, n) == 0, rng.integers(-2 ** 31, 2 ** 31, n), rng.integers(0, n_slots, n))
        entries = np.stack([slots, rng.integers(-1, 3, n), counts, rng.integers(-9, 9, n)], axis=1).astype(np.int32)
        starts = np.where(rng.integers(0, 3, (n, 2)) == 0, 0, rng.integers(-2 ** 63, 2 ** 63, (n, 2))).astype(np.int64)
        sess = rng.integers(0, 1 << 40, (n_slots, 4)).astype(np.int64)
        kept = rng.uniform(-1, 1, (n_slots, n_mels)).astype(np.float32)
        mel = rng.uniform(-1, 1, (in_frames, n_mels)).astype(np.float32)
        first = rng.uniform(-1, 1, (n, n_mels)).astype(np.float32)
        touched = {}
        tab = stream.ragged_tick_begin_tables(sess, kept, entries, mel, 80, min_frames, touched=touched, starts=starts, first=first,
                                              zero_block=2 * n_slots)[0]
        stream.ragged_tick_commit(sess, kept, entries, mel, 80, min_frames, (0, 0), touched=touched, starts=starts)
        sizes = {'sess': n_slots, 'kept': n_slots, 'mel': in_frames, 'chunk': in_frames + n, 'first': n}
        for name, idx in touched.items():
            assert not idx or (min(idx) >= 0 and max(idx) < sizes[name]), (case, name, min(idx), max(idx), sizes[name])
        assert tab.min() >= 0 and tab.max() <= 2 * n_slots and bool((tab[:, 1] < 2 * n_slots).all())


def test_the_two_starts_kernels_use_no_scratch():
    """The compiler's resource remarks for pwv_stream_tick.hip (gfx950 device code, no GPU needed): the two starts kernels with 0 bytes
    of scratch, nothing spilled and the LDS tables of the ragged kernels they instantiate; the two ragged kernels keep their figures."""
    from tests.util import kernel_resources
    names = ('stream_tick_ragged_begin_kernel', 'stream_tick_ragged_commit_kernel', 'stream_tick_starts_begin_kernel',
             'stream_tick_starts_commit_kernel')
    seen = {}
    for name, r in kernel_resources('pwv_stream_tick.hip').items():
        for kernel in names:
            if kernel in name:
                assert kernel not in seen, (kernel, name)
                seen[kernel] = r
    print({k: (r['scratch'], r['vgpr_spills'], r['sgpr_spills'], r['vgprs'], r['lds']) for k, r in seen.items()})
    assert sorted(seen) == sorted(names), sorted(seen)
    for kernel, r in seen.items():
        assert r['scratch'] == 0 and r['vgpr_spills'] == 0 and r['sgpr_spills'] == 0, (kernel, r)
    assert seen['stream_tick_ragged_begin_kernel']['lds'] == 8208 and seen['stream_tick_ragged_commit_kernel']['lds'] == 12304
    # cu [1025] and slot [1024], and live [1024] and the decision word for the commit: nothing beyond RAGGED_MAX_N-sized tables
    assert seen['stream_tick_starts_begin_kernel']['lds'] == 8208 and seen['stream_tick_starts_commit_kernel']['lds'] == 12304


# ---- tick(starts=): what is refused before anything is enqueued ------------------------------------------------------------------------
class _Stream(object):
    """What _TickGraph._tick reads of a StreamingVocoder up to its argument checks."""

    def __init__(self, n_slots, running, hop=80, n_mels=4):
        self.n_slots, self.hop, self.n_mels, self._running = n_slots, hop, n_mels, list(running)
        self._seed = [None] * n_slots
        self._pending = self._ticker = None

    def _slot(self, slot):
        from pwv_amd.stream import StreamingVocoder
        return StreamingVocoder._slot(self, slot)

    @staticmethod
    def _check_seed(v):
        from pwv_amd.stream import StreamingVocoder
        return StreamingVocoder._check_seed(v)


def _ticker(monkeypatch, running, hop=80, min_frames=1):
    """A GraphedRaggedStream without a device: the checks of tick() run on mels the device check is made to wave through."""
    from pwv_amd import engine, graph
    monkeypatch.setattr(engine, '_require_cuda_f32', lambda t, name: t)
    g = object.__new__(graph.GraphedRaggedStream)
    g.stream = _Stream(len(running), running, hop)
    g.sample, g.hop, g.min_frames, g._started = True, hop, min_frames, set()
    g._starts = object()          # (the stream has a zero block)
    return g


def test_tick_argument_errors(monkeypatch):
    import torch
    g = _ticker(monkeypatch, [True, False, True])
    m = lambda f: torch.zeros((f, 4))      # noqa: E731
    with pytest.raises(ValueError, match='starts names slot 2, which is not among the slots of this tick'):
        g.tick([m(3)], [1], starts={1: 5, 2: 7})
    with pytest.raises(ValueError, match='starts names slot 0'):          # a seed on a slot the tick does not hold at all
        g.tick([m(3)], [1], starts={0: 7})
    with pytest.raises(ValueError, match='slot 1 starts an utterance with 1 frames: it needs its first frame and at least 1 more'):
        g.tick([m(2), m(1)], [0, 1], starts={1: None})
    with pytest.raises(ValueError, match='seed'):
        g.tick([m(3)], [1], starts={1: -1})
    with pytest.raises(ValueError, match='seed'):
        g.tick([m(3)], [1], starts={1: 1 << 64})
    with pytest.raises(ValueError, match='out of range'):
        g.tick([m(3)], [1], starts={9: 1})
    with pytest.raises(ValueError, match='starts must be a dict'):
        g.tick([m(3)], [1], starts=[1])
    # a fresh slot that starts does not name is refused with the text it always had, with and without starts for others
    old = 'slot 1 is fresh: a session starts with the eager one-frame push \\(push_varlen\\(\\[mel\\[:1\\]\\], slots=\\[1\\]\\) keeps the frame'
    with pytest.raises(ValueError, match=old):
        g.tick([m(3)], [1])
    with pytest.raises(ValueError, match=old):
        g.tick([m(3), m(3)], [1, 2], starts={2: 4})
    with pytest.raises(ValueError, match=old):
        g.tick([m(3)], [1], starts={})
    # hop 16: min_frames = 2, a start needs three frames
    h = _ticker(monkeypatch, [False], hop=16, min_frames=2)
    with pytest.raises(ValueError, match='at least 2 more \\(3 in all'):
        h.tick([m(2)], [0], starts={0: 1})
    # a stream whose histories are a caller's allocation has no zero block
    from pwv_amd._lib import PwvError
    g._starts = None
    with pytest.raises(PwvError, match='no zero block'):
        g.tick([m(3)], [1], starts={1: 5})
