"""-m gpu: the four entry points of csrc/pwv_stream_tick.hip called directly through _lib on tiny, well-formed tables inside poisoned,
guard-banded buffers (tests/guarded.py): every array a kernel writes equals the numpy restatement of stream.py exactly (integer tables and
copied floats: no tolerance), no band is touched and no poison is left where a store is due.  The shapes are the smallest at which a
stride, a loop bound or the cap can go wrong: one entry and three, n_mels = 3 and 2, more entries than the 256 threads of a workgroup,
and -- the uniform tick alone -- more than the 1024 entries the ragged tick's LDS tables hold.  Only tables the contract calls well
formed: slots in range, counts that need no clamp (the clamp: tests/test_stream_ragged_graph_host.py)."""
import ctypes

import numpy as np
import pytest
import torch

from tests.guarded import guarded

pytestmark = pytest.mark.gpu

# (ragged, n_slots, N, n_mels, frame counts, hop, min_frames, sampler)
CASES = [(False, 5, 1, 3, [2], 16, None, True), (False, 5, 1, 3, [2], 16, None, False),
         (False, 5, 3, 3, [2] * 3, 16, None, True), (False, 5, 3, 3, [2] * 3, 16, None, False),
         (False, 1030, 1025, 2, [1] * 1025, 2, None, True),          # distinct slots; past 256 threads and past the ragged cap
         (True, 5, 3, 3, [2, 5, 3], 16, 2, True), (True, 5, 3, 3, [2, 5, 3], 16, 2, False),
         (True, 1030, 1024, 2, [1] * 1024, 2, 1, True)]
IDS = ['%s-%dof%d-%s' % ('ragged' if c[0] else 'uniform', c[2], c[1], 'sampler' if c[7] else 'own_noise') for c in CASES]


@pytest.mark.parametrize('ragged,n_slots,n,n_mels,counts,hop,min_frames,sample', CASES, ids=IDS)
def test_tick_kernels_equal_the_restatement(gpu, ragged, n_slots, n, n_mels, counts, hop, min_frames, sample):
    from pwv_amd import _lib, engine, stream
    lib = _lib.lib()
    rng = np.random.default_rng(n_slots + n)
    in_frames = sum(counts)
    sess = np.stack([rng.integers(0, 2, n_slots), rng.integers(0, 1000, n_slots) * hop, rng.integers(-2 ** 63, 2 ** 63, n_slots),
                     np.zeros(n_slots, np.int64)], axis=1).astype(np.int64)
    kept = rng.uniform(-1, 1, (n_slots, n_mels)).astype(np.float32)
    mel = rng.uniform(-1, 1, (in_frames, n_mels)).astype(np.float32)
    slots, live = rng.permutation(n_slots)[:n], rng.integers(0, 2, n)
    live[0] = 1
    if ragged:
        entries = np.stack([slots, live, counts, np.zeros(n)], axis=1).astype(np.int32)
        begin, commit = lib.pwv_stream_tick_ragged_begin, lib.pwv_stream_tick_ragged_commit
        tab, streams, cu_rows, cu_frames, chunk = stream.ragged_tick_begin_tables(sess, kept, entries, mel, hop, min_frames, sample=sample)
        restated_commit = lambda s, k, words: stream.ragged_tick_commit(s, k, entries, mel, hop, min_frames, words)      # noqa: E731
    else:
        f = counts[0]
        entries = np.stack([slots, live], axis=1).astype(np.int32)
        begin, commit = lib.pwv_stream_tick_begin, lib.pwv_stream_tick_commit
        tab, streams, cu_rows, chunk = stream.tick_begin_tables(sess, kept, entries, mel.reshape(n, f, n_mels), hop, sample=sample)
        cu_frames = None
        restated_commit = lambda s, k, words: stream.tick_commit(s, k, entries, mel.reshape(n, f, n_mels), f * hop, words)      # noqa: E731
    words = engine.StatusWords()          # the test's own pair of sticky words
    with guarded(engine) as g:
        T = engine.torch

        def dev(a):
            t = T.empty(a.shape, dtype=torch.from_numpy(a).dtype, device=gpu)
            t.copy_(torch.from_numpy(a))
            return t

        def table(want, dtype):          # what a kernel has to write: -1 / NaN wherever no store lands
            if want is None:
                return None
            return T.full(want.shape, -1, dtype=dtype, device=gpu) if dtype != torch.float32 else T.empty(want.shape, dtype=dtype, device=gpu)

        d_sess, d_kept, d_entries, d_mel = dev(sess), dev(kept), dev(entries), dev(mel)
        d_tab, d_streams, d_cu_rows = table(tab, torch.int32), table(streams, torch.int64), table(cu_rows, torch.int32)
        d_cu_frames, d_chunk = table(cu_frames, torch.int32), table(chunk, torch.float32)
        d_counters = T.zeros((2,), dtype=torch.int64, device=gpu)
        ta = (_lib.StreamTickRaggedArgs if ragged else _lib.StreamTickArgs)()
        ta.sess, ta.kept, ta.entries, ta.mel = d_sess.data_ptr(), d_kept.data_ptr(), d_entries.data_ptr(), d_mel.data_ptr()
        ta.n_slots, ta.N, ta.n_mels = n_slots, n, n_mels
        if ragged:
            ta.in_frames, ta.hop, ta.min_frames = in_frames, hop, min_frames
        else:
            ta.frames, ta.T = counts[0], counts[0] * hop
        ta.slot_tab, ta.chunk = d_tab.data_ptr(), d_chunk.data_ptr()
        for name, t in (('streams', d_streams), ('cu_rows', d_cu_rows), ('cu_frames', d_cu_frames)):
            if t is not None:
                setattr(ta, name, t.data_ptr())
        ta.words, ta.counters = words.addr, d_counters.data_ptr()

        def same(t, want):
            assert g.holds(t)
            return torch.equal(t.cpu(), torch.from_numpy(want))

        _lib.check(begin(ctypes.byref(ta), engine._stream()), 'begin')
        torch.cuda.synchronize()
        for name, t, want in (('slot_tab', d_tab, tab), ('streams', d_streams, streams), ('cu_rows', d_cu_rows, cu_rows),
                              ('cu_frames', d_cu_frames, cu_frames), ('chunk', d_chunk, chunk)):
            assert (t is None) == (want is None), name
            if t is not None:
                assert same(t, want), name
        assert not torch.isnan(d_chunk).any()
        assert same(d_sess, sess) and same(d_kept, kept)          # the begin kernel only reads the state
        # the commit, once with clean words and once with the range word raised
        sess1, kept1, done = restated_commit(sess, kept, (0, 0))
        assert done and not np.array_equal(sess1, sess)
        _lib.check(commit(ctypes.byref(ta), engine._stream()), 'commit')
        torch.cuda.synchronize()
        assert same(d_sess, sess1) and same(d_kept, kept1) and d_counters.tolist() == [1, 0]
        try:
            words.range = 1
            sess2, kept2, done = restated_commit(sess1, kept1, (0, 1))
            assert not done and np.array_equal(sess2, sess1) and np.array_equal(kept2, kept1)
            _lib.check(commit(ctypes.byref(ta), engine._stream()), 'commit')
            torch.cuda.synchronize()
        finally:
            words.range = 0
        assert same(d_sess, sess2) and same(d_kept, kept2) and d_counters.tolist() == [1, 1]
        assert same(d_entries, entries) and same(d_mel, mel)
        g.check()
