"""GPU: sessions that START (or are cut off and start again) inside a graphed ragged tick -- graph.GraphedRaggedStream.tick(starts=),
stream_tick_starts_begin_kernel / stream_tick_starts_commit_kernel in csrc/pwv_stream_tick.hip (include/pwv_hip.h, "STARTS").  The
contract is reset + push_varlen's: a started session gives the bits of the eager calls, its pieces concatenate to its one-shot forward,
the ticks stay pipelined (no eager push after the capture), and a refused tick leaves a fresh slot fresh and a running one on its old
utterance."""
import ctypes

import numpy as np
import pytest
import torch

from tests.guarded import guarded
from tests.test_gpu_stream import _inputs, _model, _one_shot, _small
from tests.test_gpu_stream_graph import _same_session
from tests.test_gpu_stream_persist import _Log, knobs      # noqa: F401  (knobs: the fixture)
from tests.test_gpu_stream_ragged_graph import _graphed, hop_80_afterwards      # noqa: F401  (hop_80_afterwards: the fixture)
from tests.util import hop_cfg

pytestmark = pytest.mark.gpu
HOP = 80


# ---- the two kernels against the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sample', [True, False], ids=['sampler', 'own_noise'])
@pytest.mark.parametrize('flags', ['random', 'all', 'none', 'old_size'])
@pytest.mark.parametrize('n', [1, 3, 1024])
def test_starts_kernels_equal_the_restatement(gpu, n, flags, sample):
    """The two entry points with a starts table, inside poisoned, guard-banded buffers: garbage entries (slots out of range, counts
    that need the clamp, any live word) and garbage starts words (any non-zero flag, any seed; a flag on a filler).  Every table, sess,
    kept and the counters equal the restatement, with clean words and with the range word raised, and no band is touched.  `old_size`:
    the same struct with struct_size = 120 -- the three fields are not read, the plain kernels run."""
    from pwv_amd import _lib, engine, stream
    lib = _lib.lib()
    rng = np.random.default_rng(10 * n + len(flags))
    n_slots, n_mels, hop, min_frames = n + 6, 3 if n < 1024 else 2, 16, 2
    zero_block = 2 * n_slots + 3
    counts = rng.integers(min_frames, min_frames + 4, n)
    in_frames = int(counts.sum()) + 5
    counts = np.where(rng.integers(0, 4, n) == 0, rng.integers(-2 ** 31, 2 ** 31, n), counts)          # garbage: the clamp's
    slots = rng.permutation(n_slots)[:n]
    wild = rng.integers(0, 5, n) == 0
    wild[0] = False          # entry 0 is a session: the clean commit has something to do
    slots = np.where(wild, rng.choice([-1, -2 ** 31, n_slots, 2 ** 31 - 1], n), slots)      # (in range: distinct)
    live = rng.integers(-1, 3, n)
    live[0] = 1
    entries = np.stack([slots, live, counts, rng.integers(-9, 9, n)], axis=1).astype(np.int32)
    word = rng.integers(-2 ** 63, 2 ** 63, (n, 2))
    flag = {'random': rng.integers(0, 2, n), 'all': np.ones(n, np.int64), 'none': np.zeros(n, np.int64), 'old_size': np.ones(n, np.int64)}[flags]
    starts = np.stack([np.where(flag != 0, np.where(word[:, 0] == 0, 1, word[:, 0]), 0), word[:, 1]], axis=1).astype(np.int64)
    sess = np.stack([rng.integers(0, 2, n_slots), rng.integers(0, 1000, n_slots) * hop, rng.integers(-2 ** 63, 2 ** 63, n_slots),
                     np.zeros(n_slots, np.int64)], axis=1).astype(np.int64)
    kept = rng.uniform(-1, 1, (n_slots, n_mels)).astype(np.float32)
    mel = rng.uniform(-1, 1, (in_frames, n_mels)).astype(np.float32)
    seen = None if flags == 'old_size' else starts
    starting = stream.ragged_tick_starting(entries, seen, n_slots)
    assert flags not in ('all', 'random') or n == 1 or starting.any()
    first = rng.uniform(-1, 1, (n, n_mels)).astype(np.float32)
    first[~starting] = np.nan          # read for starting entries only
    tab, streams, cu_rows, cu_frames, chunk = stream.ragged_tick_begin_tables(sess, kept, entries, mel, hop, min_frames, sample=sample,
                                                                              starts=seen, first=first, zero_block=zero_block)
    assert not np.isnan(chunk).any() and bool((tab[starting, 0] == zero_block).all()) and bool((tab[~starting] < 2 * n_slots).all())
    words = engine.StatusWords()
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

        d_sess, d_kept, d_entries, d_mel, d_starts, d_first = dev(sess), dev(kept), dev(entries), dev(mel), dev(starts), dev(first)
        d_tab, d_streams, d_cu_rows = table(tab, torch.int32), table(streams, torch.int64), table(cu_rows, torch.int32)
        d_cu_frames, d_chunk = table(cu_frames, torch.int32), table(chunk, torch.float32)
        d_counters = T.zeros((2,), dtype=torch.int64, device=gpu)
        ta = _lib.StreamTickRaggedArgs()
        ta.sess, ta.kept, ta.entries, ta.mel = d_sess.data_ptr(), d_kept.data_ptr(), d_entries.data_ptr(), d_mel.data_ptr()
        ta.n_slots, ta.N, ta.n_mels, ta.in_frames, ta.hop, ta.min_frames = n_slots, n, n_mels, in_frames, hop, min_frames
        ta.slot_tab, ta.chunk, ta.cu_rows, ta.cu_frames = d_tab.data_ptr(), d_chunk.data_ptr(), d_cu_rows.data_ptr(), d_cu_frames.data_ptr()
        if sample:
            ta.streams = d_streams.data_ptr()
        ta.words, ta.counters = words.addr, d_counters.data_ptr()
        ta.starts, ta.first, ta.zero_block = d_starts.data_ptr(), d_first.data_ptr(), zero_block
        if flags == 'old_size':
            ta.struct_size = _lib.StreamTickRaggedArgs.starts.offset

        def same(t, want):
            assert g.holds(t)
            return torch.equal(t.cpu(), torch.from_numpy(want))

        _lib.check(lib.pwv_stream_tick_ragged_begin(ctypes.byref(ta), engine._stream()), 'begin')
        torch.cuda.synchronize()
        for name, t, want in (('slot_tab', d_tab, tab), ('streams', d_streams, streams), ('cu_rows', d_cu_rows, cu_rows),
                              ('cu_frames', d_cu_frames, cu_frames), ('chunk', d_chunk, chunk)):
            assert (t is None) == (want is None), name
            if t is not None:
                assert same(t, want), name
        assert same(d_sess, sess) and same(d_kept, kept)          # the begin kernel only reads the state
        sess1, kept1, done = stream.ragged_tick_commit(sess, kept, entries, mel, hop, min_frames, (0, 0), starts=seen)
        assert done and not np.array_equal(sess1, sess)
        _lib.check(lib.pwv_stream_tick_ragged_commit(ctypes.byref(ta), engine._stream()), 'commit')
        torch.cuda.synchronize()
        assert same(d_sess, sess1) and same(d_kept, kept1) and d_counters.tolist() == [1, 0]
        try:
            words.range = 1
            sess2, kept2, done = stream.ragged_tick_commit(sess1, kept1, entries, mel, hop, min_frames, (0, 1), starts=seen)
            assert not done and np.array_equal(sess2, sess1) and np.array_equal(kept2, kept1)
            _lib.check(lib.pwv_stream_tick_ragged_commit(ctypes.byref(ta), engine._stream()), 'commit')
            torch.cuda.synchronize()
        finally:
            words.range = 0
        assert same(d_sess, sess1) and same(d_kept, kept1) and d_counters.tolist() == [1, 1]
        assert same(d_entries, entries) and same(d_mel, mel) and same(d_starts, starts)
        g.check()


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
class _Utterance(object):
    """An utterance and how far a session has got with it: chunk(c, start) = the frames and the noise of its next c frames of samples."""

    def __init__(self, cfg, frames, gpu, seed, hop=HOP):
        self.hop, self.done = hop, 0
        _, _, self.mel, self.z = _inputs(cfg, frames * hop, gpu, seed=seed)

    def chunk(self, c, start):
        assert not start or self.done == 0
        lo = self.done
        self.done += c
        return self.mel[0 if start else lo + 1:lo + 1 + c], self.z[lo * self.hop:(lo + c) * self.hop]


def _drive(g, ref, tick, sample):
    """One tick -- [(slot, utterance, frames of samples, None or ('start', seed, reset the reference?))] -- on the graphed stream and as
    reset + push_varlen on the reference stream: (graphed pieces, reference pieces)."""
    slots = [t[0] for t in tick]
    parts = [t[1].chunk(t[2], t[3]) for t in tick]
    mels, zs = [p[0] for p in parts], [p[1] for p in parts]
    starts = {t[0]: t[3][1] for t in tick if t[3]}
    got = [o.clone() for o in g.tick(mels, slots, z=None if sample else zs, starts=starts or None)]
    for t in tick:
        if t[3] and t[3][2]:
            ref.reset(t[0], t[3][1])
    want = ref.push_varlen(mels, slots=slots, z=None if sample else zs)
    return got, list(want)


@pytest.mark.parametrize('sample', [False, True], ids=['own_noise', 'sampler'])
def test_starts_inside_pipelined_ticks(gpu, knobs, sample):
    """Five ticks on a (4, 1600) capture of a 5-slot stream, enqueued with no verify() in between: running sessions alone; a start on a
    fresh slot that has served as a filler; a restart of a running slot together with a start on a fresh slot that keeps the seed of its
    reset (seed None); then two plain ticks, one of which fills the capture exactly.  Every piece equals the piece of a second stream
    driven by reset + push_varlen, the host's view after verify() equals that stream's, the pieces of every started session
    concatenate to its one-shot forward, and nothing ran eagerly after the capture."""
    cfg = _small()
    model, _ = _model(gpu, cfg)
    engine = knobs
    u = [_Utterance(cfg, f, gpu, 60 + i) for i, f in enumerate((5, 12, 11, 9, 12))]
    seeds = [3, 4, 11, (1 << 63) + 5, 77]
    s, ref = model.open_stream(slots=5), model.open_stream(slots=5)
    for st in (s, ref):
        st.reset(4, seeds[4])
        st.push_varlen([u[0].mel[:1], u[1].mel[:1]], slots=[0, 1], **({'seeds': seeds[:2]} if sample else {'z': [u[0].z[:0], u[1].z[:0]]}))
    g = _graphed(engine, s, cfg, gpu, 4, 1600, sample=sample)
    assert s._scratch_dirty[2] and not s._scratch_dirty[4]          # the capture's fillers ran on slots 0 .. 3
    ticks = [[(0, u[0], 3, None), (1, u[1], 2, None)],
             [(0, u[0], 2, None), (2, u[2], 4, ('start', seeds[2], True)), (1, u[1], 3, None)],
             [(1, u[1], 1, None), (0, u[3], 3, ('start', seeds[3], True)), (4, u[4], 5, ('start', None, False))],
             [(0, u[3], 5, None), (1, u[1], 6, None), (2, u[2], 4, None), (4, u[4], 5, None)],
             [(4, u[4], 2, None), (2, u[2], 3, None), (0, u[3], 1, None)]]
    pieces = {id(x): [] for x in u}
    with _Log(engine) as lg:
        graphed = []
        for t in ticks:
            slots = [e[0] for e in t]
            parts = [e[1].chunk(e[2], e[3]) for e in t]
            starts = {e[0]: e[3][1] for e in t if e[3]}
            got = g.tick([p[0] for p in parts], slots, z=None if sample else [p[1] for p in parts], starts=starts or None)
            graphed.append(([o.clone() for o in got], parts))
        assert [s.emitted(i) for i in range(5)] == [0] * 5 and not s._running[2] and not s._running[4]      # nothing has come back yet
        assert g.verify() == 5
        assert lg.log == [] and g.eager_calls == 0 and g.captures == 1          # no eager push, no launch outside the graph
    for t, (got, parts) in zip(ticks, graphed):
        for e in t:
            if e[3] and e[3][2]:
                ref.reset(e[0], e[3][1])
        want = ref.push_varlen([p[0] for p in parts], slots=[e[0] for e in t], z=None if sample else [p[1] for p in parts])
        for e, a, b in zip(t, got, want):
            assert tuple(a.shape) == (e[2] * HOP, 1) and bool(torch.isfinite(a).all()) and torch.equal(a, b), (e[0], e[2])
            pieces[id(e[1])].append(a)
    assert [s.emitted(i) for i in range(5)] == [ref.emitted(i) for i in range(5)] == [720, 960, 880, 0, 960]
    assert s._seed == ref._seed and s._running == ref._running == [True, True, True, False, True]
    assert torch.equal(s._kept, ref._kept)
    if sample:
        assert s._seed == [seeds[3], seeds[1], seeds[2], None, seeds[4]]
    for k in (2, 3, 4):
        got = torch.cat(pieces[id(u[k])])
        want = _one_shot(model, u[k].mel, seed=seeds[k]) if sample else _one_shot(model, u[k].mel, u[k].z)
        assert torch.equal(got, want), (k, float((got - want).abs().max()))


def test_four_starts_behind_one_verify(gpu, knobs):
    """Four ticks, each with a start (tick j starts slot j with three frames of samples and gives the sessions started before it their
    next frames; the last one fills the capture exactly), enqueued behind ONE verify(): it returns 4, and every session is its one-shot
    forward."""
    cfg = _small()
    model, _ = _model(gpu, cfg)
    counts = [[3], [2, 3], [2, 2, 3], [6, 6, 5, 3]]
    total = [sum(c[j] for c in counts if len(c) > j) for j in range(4)]
    assert total == [13, 11, 8, 3] and sum(counts[3]) * HOP == 1600
    u = [_Utterance(cfg, f, gpu, 70 + j) for j, f in enumerate(total)]
    s = model.open_stream(slots=4)
    g = _graphed(knobs, s, cfg, gpu, 4, 1600, sample=False)
    outs = [[] for _ in u]
    for j in range(4):
        slots = list(range(j + 1))
        parts = [u[i].chunk(counts[j][i], i == j) for i in slots]
        got = g.tick([p[0] for p in parts], slots, z=[p[1] for p in parts], starts={j: None})
        for i in slots:
            outs[i].append(got[i].clone())
    assert s._running == [False] * 4 and s._pending is not None
    assert g.verify() == 4 and g.eager_calls == 0 and g.captures == 1
    assert s._running == [True] * 4 and [s.emitted(j) for j in range(4)] == [f * HOP for f in total]
    for j in range(4):
        assert torch.equal(torch.cat(outs[j]), _one_shot(model, u[j].mel, u[j].z)), j


def test_a_refused_tick_starts_nothing(gpu, knobs):
    """The range word is raised as in test_prefix_rule_range_word (frames * 1e5).  The tick restarts running slot 0 and starts fresh
    slot 1 on the hot mel: it does not commit (.committed == 0).  Slot 1 is still fresh, its current block untouched and its other
    generation marked as scratch; slot 0 stands on its old utterance; and the eager pushes that follow -- a one-frame start on slot 1,
    which counts on zeros in that generation, and slot 0's next frames -- give the one-shot forwards."""
    from pwv_amd._lib import PwvRangeError
    cfg = _small()
    model, _ = _model(gpu, cfg)
    old, new, hot = _Utterance(cfg, 6, gpu, 80), _Utterance(cfg, 4, gpu, 81), _Utterance(cfg, 4, gpu, 82)
    cold = hot.mel.clone()
    hot.mel = hot.mel.clone()
    hot.mel[1:3] *= 1e5
    s = model.open_stream(slots=3)
    g = _graphed(knobs, s, cfg, gpu, 3, 800, sample=False)
    s.reset(1, 9)
    s.push_varlen([old.mel[:1]], slots=[0], z=[old.z[:0]])
    a = old.chunk(2, False)
    first = g.tick([a[0]], [0], z=[a[1]])[0].clone()
    assert g.verify() == 1
    before = s.state(0)
    gen1, block1 = s._gen[1], s._hist[2 + s._gen[1]].clone()
    b, c = new.chunk(3, True), hot.chunk(3, True)
    g.tick([b[0], c[0]], [0, 1], z=[b[1], c[1]], starts={0: 5, 1: None})
    with pytest.raises(PwvRangeError) as ei:
        g.verify()
    assert ei.value.committed == 0 and s._pending is None
    assert not s._running[1] and s._gen[1] == gen1 and s.emitted(1) == 0 and s._seed[1] == 9 and s._scratch_dirty[1]
    assert torch.equal(s._hist[2 + gen1], block1) and not bool(block1.any())
    assert s._running[0] and s.emitted(0) == 2 * HOP and _same_session(s.state(0), before)
    # the next eager pushes: slot 1 starts with one frame and goes on, slot 0 goes on with its old utterance
    hot.mel, hot.done = cold, 0
    s.push_varlen([hot.mel[:1]], slots=[1], z=[hot.z[:0]])
    d, e = old.chunk(4, False), (hot.mel[1:], hot.z)
    rest = s.push_varlen([d[0], e[0]], slots=[0, 1], z=[d[1], e[1]])
    assert torch.equal(torch.cat([first, rest[0]]), _one_shot(model, old.mel, old.z))
    assert torch.equal(rest[1], _one_shot(model, hot.mel, hot.z))


def test_a_start_that_does_not_fit_runs_eagerly(gpu, knobs):
    """12 frames of samples in a start on a (3, 800) capture (10 frames): the tick settles what is in flight, runs reset + push_varlen
    (eager_calls) and gives the bits of the reference stream; the session goes on in graphed ticks."""
    cfg = _small()
    model, _ = _model(gpu, cfg)
    s, ref = model.open_stream(slots=3), model.open_stream(slots=3)
    g = _graphed(knobs, s, cfg, gpu, 3, 800, sample=False)
    u, v = _Utterance(cfg, 15, gpu, 85), _Utterance(cfg, 15, gpu, 86)
    assert not g.fits([12])
    (got_a, want_a) = _drive(g, ref, [(1, u, 3, ('start', 6, True))], False)          # in flight when the next one arrives
    assert g.eager_calls == 0
    (got_b, want_b) = _drive(g, ref, [(2, v, 12, ('start', 7, True))], False)
    assert g.eager_calls == 1 and s._ticker is None and s._pending is not None
    assert g.verify() == 2 and s.emitted(2) == 12 * HOP == ref.emitted(2) and s._seed[2] == ref._seed[2] == 7
    (got_c, want_c) = _drive(g, ref, [(2, v, 3, None), (1, u, 4, None)], False)
    assert g.verify() == 1 and g.eager_calls == 1
    for got, want in ((got_a, want_a), (got_b, want_b), (got_c, want_c)):
        assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert torch.equal(torch.cat([got_b[0], got_c[0]]), _one_shot(model, v.mel, v.z))


def test_hop_16_a_start_of_min_frames_plus_one(gpu, knobs, hop_80_afterwards):      # noqa: F811
    """hop 16, min_frames = 2: a start with exactly three frames (32 samples) next to a running session, then a plain tick of both."""
    from pwv_amd import graph
    cfg = hop_cfg(16)
    model, _ = _model(gpu, cfg)
    assert graph.packed_filler_rows(16) // 16 == 2
    s, ref = model.open_stream(slots=3), model.open_stream(slots=3)
    u, v = _Utterance(cfg, 12, gpu, 90, hop=16), _Utterance(cfg, 7, gpu, 91, hop=16)
    for st in (s, ref):
        st.push_varlen([u.mel[:1]], slots=[0], z=[u.z[:0]])
    g = s.graphed_varlen(3, 320, sample=False)
    assert g.min_frames == 2
    with pytest.raises(ValueError, match='at least 2 more'):
        g.tick([v.mel[:2]], [2], z=[v.z[:16]], starts={2: 1})
    one = _drive(g, ref, [(0, u, 5, None), (2, v, 2, ('start', 8, True))], False)
    two = _drive(g, ref, [(2, v, 5, None), (0, u, 7, None)], False)
    assert g.verify() == 2 and g.eager_calls == 0
    for got, want in (one, two):
        assert all(torch.equal(a, b) and bool(torch.isfinite(a).all()) for a, b in zip(got, want))
    assert [s.emitted(i) for i in range(3)] == [ref.emitted(i) for i in range(3)] == [192, 0, 112]
    assert torch.equal(s._kept, ref._kept) and s._running == ref._running


def test_generate_cli_stream_graph_starts_the_files(gpu, tmp_path, monkeypatch):
    """`generate default --stream=5 --graph` on three .npy mels writes the files `--stream=5` writes, bit for bit, and begins all three
    inside its first graphed tick: no eager push at all."""
    from pwv_amd import engine, graph
    from pwv_amd.generate import _fire, generate
    from pwv_amd.hparam import hparam as hp
    from pwv_amd.stream import StreamingVocoder
    rng = np.random.default_rng(8)
    frames = [11, 16, 6]
    for i, f in enumerate(frames):
        np.save(str(tmp_path / ('m%d.npy' % i)), rng.uniform(-1, 1, (f, 80)).astype(np.float32))
    orig = type(hp).set_hparam_yaml

    def patched(self, case, *a, **k):          # what a user's hparams.yaml case would override
        r = orig(self, case, *a, **k)
        self.data_path = str(tmp_path / '*.npy')
        self.train.dataset_ratio, self.generate.batch_size = 0.0, 3
        self.model.n_iaf, self.model.dilations = 1, [[1, 2, 4, 8]]
        return r

    monkeypatch.setattr(type(hp), 'set_hparam_yaml', patched)
    calls, pushes = [], []
    real_tick, real_push = graph.GraphedRaggedStream.tick, StreamingVocoder.push_varlen

    def counting(self, mels, slots, z=None, starts=None):
        calls.append((sorted(starts or {}), self.eager_calls))
        return real_tick(self, mels, slots, z=z, starts=starts)

    def pushing(self, *a, **k):
        pushes.append(1)
        return real_push(self, *a, **k)

    monkeypatch.setattr(graph.GraphedRaggedStream, 'tick', counting)
    files = {}
    for how, argv in (('eager', ['default', '--stream=5']), ('graph', ['default', '--stream=5', '--graph'])):
        drawn = iter(range(1000, 2000))
        monkeypatch.setattr(engine, 'os_seed', lambda: next(drawn))
        if how == 'graph':
            monkeypatch.setattr(StreamingVocoder, 'push_varlen', pushing)
        logdir = tmp_path / how
        monkeypatch.setenv('PWV_LOGDIR', str(logdir))
        pred = _fire(generate, argv)
        assert [p.shape for p in pred] == [((f - 1) * 80, 1) for f in frames]
        files[how] = [(logdir / ('pred_%d.wav' % i)).read_bytes() for i in range(3)]
        with np.load(str(logdir / 'pred_wav_varlen.npz')) as npz:
            files[how] += [npz['pred_%d' % i].tobytes() for i in range(3)]
    assert calls == [([0, 1, 2], 0), ([], 0), ([], 0)] and pushes == []          # [5, 5, 5], [5, 5] + a filler, [5] + fillers: all replays
    assert files['graph'] == files['eager']
