"""CPU: the host side of the graphed RAGGED streaming tick (csrc/pwv_stream_tick.hip, graph.GraphedRaggedStream): the two entry points of
the C ABI and their ctypes mirror, their refusals (each names its field, none needs a device), the numpy restatement of the two kernels
against what StreamingVocoder.push_varlen / _commit do on the host, the clamp that keeps every address inside its array whatever the
entries hold, the layout and filler rule, and the compiler's resource remarks for the two kernels."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('pwv_stream_tick_ragged_begin', 'pwv_stream_tick_ragged_commit')


def test_abi_symbols_struct_and_version(built_lib, tmp_path):
    """Both symbols are declared in the header, listed in EXPORTED_SYMBOLS and exported by the built library; the C compiler's size and
    offsets of pwv_stream_tick_ragged_args equal the ctypes mirror's; pwv_stream_tick_args is what it was and the version is still 301."""
    from pwv_amd import _lib
    from tests.util import c_struct_probe
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'pwv_hip.h')).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r'\bint %s\s*\(const pwv_stream_tick_ragged_args\*' % name, header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(raw, name), name
    assert len(_lib.EXPORTED_SYMBOLS) == len(set(_lib.EXPORTED_SYMBOLS)) == 52
    fields = [f[0] for f in _lib.StreamTickRaggedArgs._fields_]
    assert fields[0] == 'struct_size'
    got = c_struct_probe('pwv_stream_tick_ragged_args', fields, tmp_path, extra=['sizeof(pwv_stream_tick_args)'])
    S = _lib.StreamTickRaggedArgs
    assert got == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in fields] + [ctypes.sizeof(_lib.StreamTickArgs), 301]
    assert ctypes.sizeof(_lib.StreamTickArgs) == 112          # (the size word, 4 pointers, 5 int32 padded to 24 bytes, 6 pointers: as it was)
    assert S().struct_size == ctypes.sizeof(S)
    assert built_lib.pwv_version() == _lib.HEADER_VERSION == 301


def _args(**kw):
    """A complete pwv_stream_tick_ragged_args on made-up addresses: nothing may be launched or dereferenced on the refused paths."""
    from pwv_amd import _lib
    ta = _lib.StreamTickRaggedArgs()
    ta.sess, ta.kept, ta.entries, ta.mel = 0x10000, 0x20000, 0x30000, 0x40000
    ta.n_slots, ta.N, ta.in_frames, ta.n_mels, ta.hop, ta.min_frames = 4, 3, 10, 80, 80, 1
    ta.slot_tab, ta.streams, ta.cu_rows, ta.cu_frames, ta.chunk = 0x50000, 0x60000, 0x70000, 0x78000, 0x80000
    ta.words, ta.counters = 0x90000, 0xa0000
    for k, v in kw.items():
        setattr(ta, k, v)
    return ta


_BOTH = [({'sess': None}, b'sess'), ({'kept': None}, b'kept'), ({'entries': None}, b'entries'), ({'mel': None}, b'mel'),
         ({'N': 0}, b'N must'), ({'N': 1025, 'in_frames': 4096}, b'N must'), ({'in_frames': 2}, b'in_frames'),
         ({'in_frames': 5, 'min_frames': 2}, b'in_frames'), ({'min_frames': 0}, b'min_frames'), ({'hop': 0}, b'hop'),
         ({'n_mels': 0}, b'n_mels'), ({'n_slots': 0}, b'n_slots'), ({'struct_size': 0}, b'struct_size'), ({'struct_size': 16}, b'struct_size'),
         ({'in_frames': 1 << 30, 'hop': 80}, b'2^31')]


@pytest.mark.parametrize('symbol', SYMBOLS)
@pytest.mark.parametrize('fields,named', _BOTH, ids=[','.join('%s=%r' % kv for kv in f.items()) for f, _ in _BOTH])
def test_refusals_name_the_field(built_lib, symbol, fields, named):
    fn = getattr(built_lib, symbol)
    assert fn(ctypes.byref(_args(**fields)), None) == -1
    err = built_lib.pwv_last_error()
    assert named in err and symbol.encode() in err, err


def test_refusals_of_each_entry_point(built_lib):
    """The pointers each entry point alone needs.  `streams` is the one pointer that may be NULL (the caller's noise); cu_rows is
    required with or without it: the layout of the launches, not only of the sampler."""
    lib = built_lib
    assert lib.pwv_stream_tick_ragged_begin(None, None) == -1 and b'args is NULL' in lib.pwv_last_error()
    assert lib.pwv_stream_tick_ragged_commit(None, None) == -1 and b'args is NULL' in lib.pwv_last_error()
    for field in ('slot_tab', 'chunk', 'cu_rows', 'cu_frames'):
        assert lib.pwv_stream_tick_ragged_begin(ctypes.byref(_args(**{field: None})), None) == -1
        assert field.encode() in lib.pwv_last_error(), lib.pwv_last_error()
    assert lib.pwv_stream_tick_ragged_begin(ctypes.byref(_args(streams=None, cu_rows=None)), None) == -1
    assert b'cu_rows' in lib.pwv_last_error(), lib.pwv_last_error()
    for field in ('words', 'counters'):
        assert lib.pwv_stream_tick_ragged_commit(ctypes.byref(_args(**{field: None})), None) == -1
        assert field.encode() in lib.pwv_last_error(), lib.pwv_last_error()


# ---- the restatement against the host code of push_varlen ----------------------------------------------------------------------------
class _HostStream(object):
    """The host bookkeeping of StreamingVocoder for RUNNING sessions, without a device: `push_tables` is what push_varlen() builds
    (stream.py: ragged_plan, the packed mel with the kept frames in front, VarlenGeometry.stream_table, the slot table), `commit` what
    _commit's closure does."""

    def __init__(self, rng, n_slots, n_mels, hop):
        self.hop = hop
        self.gen = [int(v) for v in rng.integers(0, 2, n_slots)]
        self.emitted = [int(v) * hop for v in rng.integers(0, 1000, n_slots)]
        self.seed = [int(v) for v in rng.integers(0, 1 << 63, n_slots)]
        self.seed[0] = (1 << 63) + 9          # a seed whose top bit is set: carried as the int64 with the same bits
        self.kept = rng.uniform(-1, 1, (n_slots, n_mels)).astype(np.float32)

    def sess(self):
        from pwv_amd import engine
        return np.array([[g, e, engine.as_int64_bits(sd), 0] for g, e, sd in zip(self.gen, self.emitted, self.seed)], np.int64)

    def push_tables(self, slots, mels):
        from pwv_amd import engine, stream
        plan = stream.ragged_plan([m.shape[0] for m in mels], [False] * len(slots), self.hop)
        assert plan.launch == list(range(len(slots)))
        geom = engine.VarlenGeometry(plan.samples, self.hop, 'cpu')
        table = geom.stream_table([(self.seed[s], self.emitted[s]) for s in slots]).numpy()
        tab = np.array([[2 * s + self.gen[s], 2 * s + 1 - self.gen[s]] for s in slots], np.int32)
        mel = np.concatenate([p for s, m in zip(slots, mels) for p in (self.kept[s:s + 1], m)])
        return tab, table, np.asarray(plan.cu_rows, np.int32), np.asarray(plan.cu_frames, np.int32), mel

    def commit(self, slots, samples, last):
        for i, s in enumerate(slots):
            self.gen[s] ^= 1
            self.emitted[s] += samples[i]
        self.kept[slots] = last


def _random_tick(rng, n_slots, min_frames, n_mels):
    k = int(rng.integers(1, n_slots + 1))
    slots = [int(s) for s in rng.permutation(n_slots)[:k]]
    frames = [int(f) for f in rng.integers(min_frames, min_frames + 9, k)]
    mels = [rng.uniform(-1, 1, (f, n_mels)).astype(np.float32) for f in frames]
    return slots, frames, mels


@pytest.mark.parametrize('hop', [80, 16, 96])
def test_restatement_equals_what_push_varlen_builds(hop):
    """Random sets of running sessions and frame counts: the tables of ragged_tick_begin_tables are ragged_plan's cu_rows / cu_frames, the
    slot table, stream_table and the packed mel of push_varlen; ragged_tick_commit is _commit's effect, and nothing with a word raised."""
    from pwv_amd import graph, stream
    n_mels = 8
    min_frames = graph.packed_filler_rows(hop) // hop
    assert min_frames == {80: 1, 16: 2, 96: 1}[hop]
    rng = np.random.default_rng(hop)
    for n_slots in (1, 2, 5, 9):
        for _ in range(6):
            host = _HostStream(rng, n_slots, n_mels, hop)
            slots, frames, mels = _random_tick(rng, n_slots, min_frames, n_mels)
            entries = [[s, 1, f, 0] for s, f in zip(slots, frames)]
            mel = np.concatenate(mels)
            got = stream.ragged_tick_begin_tables(host.sess(), host.kept, entries, mel, hop, min_frames)
            want = host.push_tables(slots, mels)
            for g, w in zip(got, want):
                assert g.dtype == w.dtype and np.array_equal(g, w)
            # `live` plays no part in the tables
            again = stream.ragged_tick_begin_tables(host.sess(), host.kept, [[s, 0, f, 0] for s, f in zip(slots, frames)], mel, hop, min_frames)
            assert all(np.array_equal(a, b) for a, b in zip(again, got))
            sess0, kept0 = host.sess(), host.kept.copy()
            for words in ((4, 0), (0, 1), (1, 1)):
                s2, k2, done = stream.ragged_tick_commit(sess0, kept0, entries, mel, hop, min_frames, words)
                assert not done and np.array_equal(s2, sess0) and np.array_equal(k2, kept0)
            # a filler never changes the table or the kept frames; a live entry does what _commit does
            mixed = [[s, 1 if i % 2 == 0 else 0, f, 0] for i, (s, f) in enumerate(zip(slots, frames))]
            s3, k3, done = stream.ragged_tick_commit(sess0, kept0, mixed, mel, hop, min_frames, (0, 0))
            assert done
            for i, s in enumerate(slots):
                if i % 2:
                    assert np.array_equal(s3[s], sess0[s]) and np.array_equal(k3[s], kept0[s])
            sess1, kept1, done = stream.ragged_tick_commit(sess0, kept0, entries, mel, hop, min_frames, (0, 0))
            host.commit(slots, [f * hop for f in frames], np.stack([m[-1] for m in mels]))
            assert done and np.array_equal(sess1, host.sess()) and np.array_equal(kept1, host.kept)
            assert np.array_equal(sess0[:, 2:], sess1[:, 2:])          # the seeds do not move


def test_ticks_chain_like_pushes():
    """Three ragged ticks through the restatement (the begin tables of tick j from the table tick j - 1 committed) against three host
    pushes, with a filler entry behind the sessions: the device table alone carries generation, counter and kept frame."""
    from pwv_amd import stream
    rng = np.random.default_rng(3)
    hop, n_mels = 80, 8
    host = _HostStream(rng, 4, n_mels, hop)
    sess, kept = host.sess(), host.kept.copy()
    slots, in_frames = [2, 0], 12
    for frames in ([3, 5], [1, 1], [7, 2]):
        mels = [rng.uniform(-1, 1, (f, n_mels)).astype(np.float32) for f in frames]
        real = sum(frames)
        mel = np.concatenate(mels + [np.zeros((in_frames - real, n_mels), np.float32)])
        entries = [[s, 1, f, 0] for s, f in zip(slots, frames)] + [[3, 0, in_frames - real, 0]]
        tab, streams, cu_rows, cu_frames, chunk = stream.ragged_tick_begin_tables(sess, kept, entries, mel, hop, 1)
        w = host.push_tables(slots, mels)
        assert np.array_equal(tab[:2], w[0]) and np.array_equal(streams[:2], w[1])
        assert np.array_equal(cu_rows[:3], w[2]) and np.array_equal(cu_frames[:3], w[3]) and np.array_equal(chunk[:real + 2], w[4])
        assert cu_rows[3] == in_frames * hop and cu_frames[3] == in_frames + 3
        assert np.array_equal(chunk[real + 2], kept[3]) and not chunk[real + 3:].any()      # the filler: its kept frame, then zeros
        sess, kept, _ = stream.ragged_tick_commit(sess, kept, entries, mel, hop, 1, (0, 0))
        host.commit(slots, [f * hop for f in frames], np.stack([m[-1] for m in mels]))
    assert np.array_equal(sess, host.sess()) and np.array_equal(kept, host.kept)


def test_clamp_keeps_every_address_inside_its_array():
    """1000 seeded tables of garbage -- negative counts, huge counts, zeros, slots out of range --: the counts the device reads rise by
    at least min_frames per entry and end at in_frames, and every index the restatement of the two kernels touches lies inside its
    array (the chunk is tiled exactly: ragged_tick_begin_tables asserts it)."""
    from pwv_amd import stream
    rng = np.random.default_rng(2024)
    n_mels = 3
    for case in range(1000):
        n = int(rng.integers(1, 12))
        min_frames = int(rng.integers(1, 4))
        in_frames = n * min_frames + int(rng.integers(0, 40))
        n_slots = int(rng.integers(1, 9))
        kind = rng.integers(0, 5, (n,))
        counts = np.select([kind == 0, kind == 1, kind == 2, kind == 3],
                           [rng.integers(-2 ** 31, 0, n), rng.integers(2 ** 20, 2 ** 31, n), np.zeros(n, np.int64), rng.integers(0, in_frames + 3, n)],
                           rng.integers(-5, 5, n))
        slots = np.where(rng.integers(0, 3, n) == 0, rng.integers(-2 ** 31, 2 ** 31, n), rng.integers(0, n_slots, n))
        entries = np.stack([slots, rng.integers(-1, 3, n), counts, rng.integers(-9, 9, n)], axis=1).astype(np.int32)
        cu = stream.ragged_tick_counts(entries, in_frames, min_frames)
        assert cu[0] == 0 and cu[-1] == in_frames and bool((np.diff(cu) >= min_frames).all()), (case, cu)
        sess = rng.integers(0, 1 << 40, (n_slots, 4)).astype(np.int64)
        kept = rng.uniform(-1, 1, (n_slots, n_mels)).astype(np.float32)
        mel = rng.uniform(-1, 1, (in_frames, n_mels)).astype(np.float32)
        touched = {}
        tab, streams, cu_rows, cu_frames, chunk = stream.ragged_tick_begin_tables(sess, kept, entries, mel, 80, min_frames, touched=touched)
        stream.ragged_tick_commit(sess, kept, entries, mel, 80, min_frames, (0, 0), touched=touched)
        sizes = {'sess': n_slots, 'kept': n_slots, 'mel': in_frames, 'chunk': in_frames + n}
        for name, idx in touched.items():
            assert idx and min(idx) >= 0 and max(idx) < sizes[name], (case, name, min(idx), max(idx), sizes[name])
        assert np.array_equal(cu_rows, 80 * cu) and np.array_equal(cu_frames, cu + np.arange(n + 1))
        assert tab.min() >= 0 and tab.max() < 2 * n_slots


class _Capacity(object):
    """GraphedRaggedStream's layout arithmetic on a capacity, without a device (the methods read these four attributes only)."""

    def __init__(self, slots, rows, hop):
        from pwv_amd import graph
        self.slots, self.rows, self.hop = slots, rows, hop
        self.filler = graph.packed_filler_rows(hop)
        self.min_frames, self.in_frames = self.filler // hop, rows // hop
        self._layout = graph.GraphedRaggedStream._layout.__get__(self)
        self.fits = graph.GraphedRaggedStream.fits.__get__(self)


def test_layout_and_fits():
    c = _Capacity(3, 400, 80)
    assert c.min_frames == 1 and c.in_frames == 5
    assert c._layout([1, 3, 1]) == [1, 3, 1]                      # an exact fill at k = slots
    assert not c.fits([1, 2, 1]) and not c.fits([2, 3, 1])        # k = slots must fill exactly
    assert c._layout([2, 1]) == [2, 1, 2]                         # the remainder filler
    assert c._layout([1]) == [1, 1, 3]                            # a min_frames filler, then the remainder
    assert c.fits([3]) and not c.fits([4])                        # 4 frames + 2 fillers of 1 = 6 > 5: k * min_frames too many
    assert c.fits([2, 2]) and not c.fits([3, 2])
    assert not c.fits([]) and not c.fits([1, 1, 1, 2]) and not c.fits([0, 2])
    with pytest.raises(ValueError, match='exceed'):
        c._layout([4])
    h = _Capacity(3, 16 * 20, 16)                                 # hop 16: a session needs 32 rows = 2 frames
    assert h.min_frames == 2 and h.in_frames == 20
    assert h._layout([5]) == [5, 2, 13] and h._layout([2, 2]) == [2, 2, 16] and h._layout([16]) == [16, 2, 2]
    assert not h.fits([17])
    with pytest.raises(ValueError, match='at least 2 frames'):
        h._layout([1, 5])                                         # a count below min_frames
    one = _Capacity(1, 800, 80)
    assert one._layout([10]) == [10] and not one.fits([9])


class _StubStream(object):
    def __init__(self, n_slots):
        self.n_slots, self._running, self._scratch_dirty = n_slots, [True] * n_slots, [False] * n_slots


def _entry_writer(cls, count, ints, **attrs):
    """A graph class's _write_entries on host tensors, without a device: the staging buffers and the 'device' table are CPU tensors."""
    import torch
    g = object.__new__(cls)
    g.stream = _StubStream(count)
    g._entries = torch.full((count, ints), -7, dtype=torch.int32)
    g._entries_host = [torch.zeros((count, ints), dtype=torch.int32)]
    g._entries_dev = None
    for k, v in attrs.items():
        setattr(g, k, v)
    return g


def test_the_entries_upload_is_skipped_only_for_the_same_table():
    """The upload of a tick's entries is skipped when the device table holds them already -- and the LIVE flags are part of what is
    compared: the same slots and frames with another number of called sessions is another table.  (A session that sits out a tick
    becomes a filler on its own slot with the frames it had; one that rejoins takes over a filler's slot and frames.)"""
    from pwv_amd import graph
    g = _entry_writer(graph.GraphedRaggedStream, 3, 4, slots=3)
    cap = _Capacity(3, 720, 80)
    for called, frames, want in [([0, 1, 2], [3, 3, 3], [[0, 1, 3, 0], [1, 1, 3, 0], [2, 1, 3, 0]]),
                                 ([0, 1], [3, 3], [[0, 1, 3, 0], [1, 1, 3, 0], [2, 0, 3, 0]]),          # session 2 sits out: same slots, same frames
                                 ([0, 1], [3, 3], [[0, 1, 3, 0], [1, 1, 3, 0], [2, 0, 3, 0]]),
                                 ([0], [3], [[0, 1, 3, 0], [1, 0, 1, 0], [2, 0, 5, 0]]),
                                 ([0, 1], [3, 1], [[0, 1, 3, 0], [1, 1, 1, 0], [2, 0, 5, 0]]),          # session 1 rejoins on the filler's frames
                                 ([0, 1, 2], [3, 1, 5], [[0, 1, 3, 0], [1, 1, 1, 0], [2, 1, 5, 0]])]:
        before = g._entries.clone()
        others = g._write_entries(0, called, cap._layout(frames))
        assert others == [s for s in range(3) if s not in called]
        assert g._entries.tolist() == want, (called, frames, g._entries.tolist())
        if before.tolist() == want:
            g._entries_host[0].fill_(-9)          # (an identical table: nothing is staged again)
            g._write_entries(0, called, cap._layout(frames))
            assert g._entries.tolist() == want
    u = _entry_writer(graph.GraphedStream, 3, 2, n=3)
    for called, want in [([0, 1, 2], [[0, 1], [1, 1], [2, 1]]), ([0, 1], [[0, 1], [1, 1], [2, 0]]), ([0], [[0, 1], [1, 0], [2, 0]]),
                         ([0, 1], [[0, 1], [1, 1], [2, 0]]), ([0, 1, 2], [[0, 1], [1, 1], [2, 1]])]:
        u._write_entries(0, called)
        assert u._entries.tolist() == want, (called, u._entries.tolist())


def test_the_two_ragged_tick_kernels_use_no_scratch():
    """The compiler's resource remarks for pwv_stream_tick.hip (gfx950 device code, no GPU needed): both ragged kernels with 0 bytes of
    scratch and nothing spilled."""
    from tests.util import kernel_resources
    seen, lds = {}, {}
    for name, r in kernel_resources('pwv_stream_tick.hip').items():
        for kernel in ('stream_tick_ragged_begin_kernel', 'stream_tick_ragged_commit_kernel'):
            if kernel in name:
                seen[kernel] = (r['scratch'], r['vgpr_spills'], r['sgpr_spills'], r['vgprs'])
                lds[kernel] = r['lds']
    print('ragged tick kernels (scratch, spilled VGPRs, spilled SGPRs, VGPRs):', seen, 'LDS bytes:', lds)
    # cu [1025] and slot [1024] (begin), and live [1024] and the decision word besides (commit): what the kernels held before the merge
    assert lds == {'stream_tick_ragged_begin_kernel': 8208, 'stream_tick_ragged_commit_kernel': 12304}, lds
    assert sorted(seen) == ['stream_tick_ragged_begin_kernel', 'stream_tick_ragged_commit_kernel'], seen
    for kernel, (sc, vs, ss, vg) in seen.items():
        assert sc == 0 and vs == 0 and ss == 0, (kernel, sc, vs, ss)
