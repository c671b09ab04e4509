"""GPU: a RAGGED streaming tick replayed as ONE graph with the frame counts read and the commit made on the device
(graph.GraphedRaggedStream, StreamingVocoder.graphed_varlen; stream_tick_ragged_begin_kernel / stream_tick_ragged_commit_kernel in
csrc/pwv_stream_tick.hip).  The contract is push_varlen's: a tick gives the bits of the eager push_varlen from the same state, the ticks
of a session concatenate to its one-shot forward, a session does not depend on its companions (filler sessions included), and a tick
is a transaction that the device commits or refuses.  Every case first shows, from engine.EVENT_LOG during the warm-up of the capture,
that each flow is one PACKED streaming persistent launch."""
import numpy as np
import pytest
import torch

from oracle import iaf_oracle as O
from tests.test_gpu_stream import _inputs, _model, _one_shot, _small, _small_wide
from tests.test_gpu_stream_graph import _same_session
from tests.test_gpu_stream_persist import _Log, _random_state, _short_expected, knobs      # noqa: F401  (knobs: the fixture)
from tests.test_gpu_stream_varlen import _check_packed
from tests.util import HOP_CASES, hop_cfg, set_hparams, small_cfg

pytestmark = pytest.mark.gpu
HOP = 80


def _graphed(engine, s, cfg, gpu, slots, rows, **kw):
    """s.graphed_varlen(slots, rows) with the route of its warm-up ticks checked: per flow one ('stream_ragged', 'packed') entry and
    one streaming persistent launch (layer 0 folded, the tail inside, the instantiation the plan predicts), nothing else."""
    with _Log(engine) as lg:
        g = s.graphed_varlen(slots, rows, **kw)
    _check_packed(lg.log, cfg, [rows] * kw.get('warmup', 2), gpu)
    assert g.captures == 1 and g.eager_calls == 0
    return g


def _mid_utterance(s, rng, gpu, hop=HOP, slots=None):
    """The slots of `s` (default: all) running, as load_state leaves them: a random kept frame, some samples emitted."""
    for sl in (range(s.n_slots) if slots is None else slots):
        st = s.state(sl)
        st['kept'] = torch.from_numpy(rng.uniform(-1, 1, (s.n_mels,)).astype(np.float32)).to(gpu)
        st['running'], st['emitted'] = True, hop * (3 + sl)
        s.load_state(sl, st)


def _tick_inputs(cfg, frames, gpu, seed, hop=HOP):
    rng = np.random.default_rng(seed)
    mels = [torch.from_numpy(rng.uniform(-1, 1, (f, cfg.n_mels)).astype(np.float32)).to(gpu) for f in frames]
    zs = [torch.from_numpy(np.clip(rng.logistic(0, 1, (f * hop, 1)), -20, 20).astype(np.float32)).to(gpu) for f in frames]
    return mels, zs


def _tick_against_push_varlen(engine, model, cfg, gpu, n_slots, capacity, slots, frames, hop=HOP):
    """One graphed tick and one eager push_varlen from the same random non-zero state (both generations, random kept frames), explicit
    z: torch.equal outputs, both generations of the called sessions, the current generation of every other slot, kept frames, emitted
    counts and generation bits.  (A filler writes the generation its slot does not stand on: scratch until a flip.)"""
    mels, zs = _tick_inputs(cfg, frames, gpu, 17 * n_slots + sum(frames), hop)
    res = []
    for graphed in (True, False):
        s = model.open_stream(slots=n_slots)
        g = _graphed(engine, s, cfg, gpu, capacity[0], capacity[1], sample=False) if graphed else None
        _mid_utterance(s, np.random.default_rng(5), gpu, hop)
        _random_state(s, 100 + sum(frames))
        if graphed:
            assert g.fits(frames)
            out = g.tick(mels, slots, z=zs)
            out = [o.clone() for o in out]
            assert s._pending is not None
            assert g.verify() == 1 and s._pending is None and g.eager_calls == 0 and g.captures == 1
        else:
            out = list(s.push_varlen(mels, slots=slots, z=zs))
        res.append((out, s._hist.clone(), s._kept.clone(), [s.emitted(sl) for sl in range(n_slots)], list(s._gen)))
    (out_g, hist_g, kept_g, em_g, gen_g), (out_p, hist_p, kept_p, em_p, gen_p) = res
    assert [tuple(o.shape) for o in out_g] == [(f * hop, 1) for f in frames]
    for a, b in zip(out_g, out_p):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b), float((a - b).abs().max())
    called = [blk for sl in slots for blk in (2 * sl, 2 * sl + 1)]
    assert torch.equal(hist_g[called], hist_p[called]), int((hist_g[called] != hist_p[called]).sum())
    current = [2 * sl + gen_p[sl] for sl in range(n_slots) if sl not in slots]
    assert torch.equal(hist_g[current], hist_p[current])
    assert torch.equal(kept_g, kept_p) and em_g == em_p and gen_g == gen_p
    assert em_g == [hop * (3 + sl) + (frames[slots.index(sl)] * hop if sl in slots else 0) for sl in range(n_slots)]


_TICKS = [('small_wide', 4, (3, 400), [0, 1, 2], [1, 3, 1]), ('small_wide', 4, (3, 400), [0, 1], [2, 1]), ('small_wide', 4, (3, 400), [2], [1]),
          ('default', 6, (4, 1280), [4, 1, 5], [7, 1, 5])]


@pytest.mark.parametrize('shape', _TICKS, ids=['wide_exact_fill', 'wide_remainder_filler', 'wide_hop_filler_and_remainder', 'default_permuted'])
@pytest.mark.parametrize('precision', ['f16x3', 'f32'])
def test_tick_against_push_varlen(gpu, knobs, precision, shape):
    config, n_slots, capacity, slots, frames = shape
    cfg = _small_wide() if config == 'small_wide' else O.ModelConfig()
    model, _ = _model(gpu, cfg, precision)
    _tick_against_push_varlen(knobs, model, cfg, gpu, n_slots, capacity, slots, frames)


@pytest.mark.parametrize('precision', ['f16x3', 'f32'])
def test_tick_on_the_general_instantiation(gpu, knobs, precision):
    """Default model, 8 sessions in all 8 slots filling 32000 rows exactly (one of them a single frame next to 78): the packed launch
    of the graph is the general instantiation."""
    cfg = O.ModelConfig()
    model, _ = _model(gpu, cfg, precision)
    assert _short_expected(32000, 512, gpu) == 0
    _tick_against_push_varlen(knobs, model, cfg, gpu, 8, (8, 32000), list(range(8)), [51, 52, 53, 54, 55, 56, 78, 1])


@pytest.mark.parametrize('config', ['small', 'default'])
def test_pipelined_ragged_ticks_equal_the_one_shot_forward(gpu, knobs, config):
    """Three sessions of 2400, 1600 and 880 samples: each starts with the eager one-frame push, then EVERY tick is enqueued with no
    verify() in between, the frame counts changing from tick to tick; a session leaves the tick when its utterance ends, on a short
    last chunk.  One verify() at the end returns the tick count; until then nothing has come back to the host."""
    cfg = _small() if config == 'small' else O.ModelConfig()
    model, _ = _model(gpu, cfg)
    lengths = [2400, 1600, 880]
    ins = [_inputs(cfg, L, gpu, seed=3 + i) for i, L in enumerate(lengths)]
    schedule = {0: [7, 3, 9, 5, 6], 1: [5, 8, 1, 6], 2: [2, 6, 3]}
    assert [sum(v) * HOP for v in schedule.values()] == lengths
    s = model.open_stream(slots=4)
    g = _graphed(knobs, s, cfg, gpu, 4, 1600, sample=False)      # (its fillers ran on the fresh slots: the starts below must not see them)
    first = s.push_varlen([ins[i][2][:1] for i in range(3)], slots=[0, 1, 2], z=[ins[i][3][:0] for i in range(3)])
    assert [tuple(p.shape) for p in first] == [(0, 1)] * 3
    outs, fpos = [[], [], []], [1, 1, 1]
    for j in range(5):
        slots = [i for i in range(3) if j < len(schedule[i])]
        counts = [schedule[i][j] for i in slots]
        got = g.tick([ins[i][2][fpos[i]:fpos[i] + f] for i, f in zip(slots, counts)], slots,
                     z=[ins[i][3][(fpos[i] - 1) * HOP:(fpos[i] - 1 + f) * HOP] for i, f in zip(slots, counts)])
        for k, (i, f) in enumerate(zip(slots, counts)):
            outs[i].append(got[k].clone())
            fpos[i] += f
    assert [s.emitted(i) for i in range(3)] == [0, 0, 0]          # nothing has come back to the host yet
    assert g.verify() == 5
    assert [s.emitted(i) for i in range(4)] == lengths + [0] and g.captures == 1 and g.eager_calls == 0
    for i in range(3):
        got, want = torch.cat(outs[i]), _one_shot(model, ins[i][2], ins[i][3])
        assert torch.equal(got, want), (i, float((got - want).abs().max()))


def test_seeds(gpu, knobs):
    """sample=True, two sessions with seeds (one above 2**63) and frame counts of their own: the pieces of slot i concatenate to
    IAFVocoder(1, L_i) drawing from noise_seed = seeds[i], noise_offset = 0 -- the sampler inside the graph reads cu_rows and {seed,
    emitted} from the tables the begin kernel wrote."""
    cfg = _small()
    model, _ = _model(gpu, cfg)
    lengths = [640, 480]
    ins = [_inputs(cfg, L, gpu, seed=30 + i) for i, L in enumerate(lengths)]
    seeds = [5, (1 << 63) + 9]
    s = model.open_stream(slots=3)
    g = _graphed(knobs, s, cfg, gpu, 3, 800, sample=True)
    s.push_varlen([ins[0][2][:1], ins[1][2][:1]], slots=[0, 1], seeds=seeds)
    outs, fpos = [[], []], [1, 1]
    for counts in ([3, 1], [1, 4], [4, 1]):
        got = g.tick([ins[i][2][fpos[i]:fpos[i] + f] for i, f in enumerate(counts)], [0, 1])
        for i, f in enumerate(counts):
            outs[i].append(got[i].clone())
            fpos[i] += f
    assert g.verify() == 3 and g.eager_calls == 0
    assert [s.emitted(i) for i in range(2)] == lengths and s._seed[:2] == seeds
    with pytest.raises(ValueError, match='z is not taken'):
        g.tick([ins[0][2][:1]], [0], z=[ins[0][3][:HOP]])
    for i in range(2):
        assert torch.equal(torch.cat(outs[i]), _one_shot(model, ins[i][2], seed=seeds[i])), i


def test_fillers_and_independence(gpu, knobs):
    """A (4, 1600) capture on a 6-slot stream called with 2 permuted slots (two fillers per tick, one of them on a FRESH slot) against a
    (2, exact) capture: the called sessions give the same bits; the bystanders' current generation, kept frame and emitted count are
    untouched; the warm-up and the capture -- all fillers -- changed no session; and the fresh slot a filler ran on still starts an
    utterance that equals the one-shot forward."""
    cfg = _small()
    model, _ = _model(gpu, cfg)
    called, frames, running = [4, 1], [3, 5], [4, 1, 3]
    ticks = [_tick_inputs(cfg, frames, gpu, 40 + j) for j in range(3)]
    a = model.open_stream(slots=6)
    _mid_utterance(a, np.random.default_rng(6), gpu, slots=running)
    before = [a.state(sl) for sl in range(6)]
    ga = _graphed(knobs, a, cfg, gpu, 4, 1600, sample=False)
    assert all(_same_session(a.state(sl), before[sl]) for sl in range(6))          # warm-up and capture: fillers only
    b = model.open_stream(slots=6)
    for sl in range(6):
        b.load_state(sl, before[sl])
    gb = _graphed(knobs, b, cfg, gpu, 2, sum(frames) * HOP, sample=False)
    outs = []
    for g in (ga, gb):
        got = []
        for mels, zs in ticks:
            got.append(torch.cat([o.clone() for o in g.tick(mels, called, z=zs)]))
        assert g.verify() == 3 and g.eager_calls == 0
        outs.append(torch.cat(got))
    assert torch.equal(outs[0], outs[1])
    assert a._scratch_dirty[0] and not a._running[0]                               # slot 0: fresh, and a filler of `ga` ran on it
    for sl in range(6):
        if sl in called:
            assert _same_session(a.state(sl), b.state(sl))
            assert a.emitted(sl) == before[sl]['emitted'] + 3 * frames[called.index(sl)] * HOP
        else:
            assert _same_session(a.state(sl), before[sl]), sl
    L = 480
    _, _, mel_t, z_t = _inputs(cfg, L, gpu, seed=77)
    start = a.push_varlen([mel_t[:1]], slots=[0], z=[z_t[:0]])
    piece = ga.tick([mel_t[1:]], [0], z=[z_t])[0].clone()
    assert ga.verify() == 1 and a.emitted(0) == L and tuple(start[0].shape) == (0, 1)
    assert torch.equal(piece, _one_shot(model, mel_t, z_t))


def test_a_session_sits_out_a_tick_and_rejoins_on_the_same_layout(gpu, knobs):
    """Consecutive ticks whose slots and frame layout coincide while the set of called sessions differs: session 2 sits out a tick (its
    slot is the filler, with the frames it had), session 1 rejoins on the frames a filler of its slot had.  The live flags reach the
    device with every such tick: a session that sat out is untouched, one that rejoined is committed.  Every session equals the same
    push_varlen calls on an eager stream (history, kept frame, emitted, generation) and its own one-shot forward."""
    cfg = _small()
    model, _ = _model(gpu, cfg)
    ticks = [([0, 1, 2], [3, 3, 3]), ([0, 1], [3, 3]), ([0], [3]), ([0, 1], [3, 1]), ([0, 1, 2], [3, 3, 3])]
    frames = [sum(f for sl, fr in ticks for s_, f in zip(sl, fr) if s_ == i) for i in range(3)]
    assert frames == [15, 10, 6]
    ins = [_inputs(cfg, f * HOP, gpu, seed=90 + i) for i, f in enumerate(frames)]
    s, ref = model.open_stream(slots=3), model.open_stream(slots=3)
    g = _graphed(knobs, s, cfg, gpu, 3, 720, sample=False)
    for st in (s, ref):
        st.push_varlen([ins[i][2][:1] for i in range(3)], z=[ins[i][3][:0] for i in range(3)])
    outs, fpos = [[], [], []], [1, 1, 1]
    layouts = []
    for slots, counts in ticks:
        mels = [ins[i][2][fpos[i]:fpos[i] + f] for i, f in zip(slots, counts)]
        zs = [ins[i][3][(fpos[i] - 1) * HOP:(fpos[i] - 1 + f) * HOP] for i, f in zip(slots, counts)]
        layouts.append(g._layout(counts))
        got = g.tick(mels, slots, z=zs)
        ref.push_varlen(mels, slots=slots, z=zs)
        for k, (i, f) in enumerate(zip(slots, counts)):
            outs[i].append(got[k].clone())
            fpos[i] += f
    assert layouts[0] == layouts[1] == [3, 3, 3] and layouts[2] == layouts[3] == [3, 1, 5]       # the coinciding layouts
    assert g.verify() == 5 and g.eager_calls == 0 and g.captures == 1
    assert [s.emitted(i) for i in range(3)] == [f * HOP for f in frames] and s._gen == ref._gen
    for i in range(3):
        assert _same_session(s.state(i), ref.state(i)), i
        got, want = torch.cat(outs[i]), _one_shot(model, ins[i][2], ins[i][3])
        assert torch.equal(got, want), (i, float((got - want).abs().max()))


def test_a_session_sits_out_a_uniform_tick(gpu, knobs):
    """The same for the uniform GraphedStream: ticks of slots [0, 1, 2], [0, 1] (slot 2 the filler), [0, 1, 2] keep the slot order, so
    only the live flags tell them apart."""
    cfg = _small()
    model, _ = _model(gpu, cfg)
    f = 2
    ticks = [[0, 1, 2], [0, 1], [0], [0, 1], [0, 1, 2]]
    frames = [f * sum(i in t for t in ticks) for i in range(3)]
    ins = [_inputs(cfg, n * HOP, gpu, seed=95 + i) for i, n in enumerate(frames)]
    s = model.open_stream(slots=3)
    g = s.graphed(3, f, sample=False)
    s.push(torch.stack([ins[i][2][:1] for i in range(3)]), z=torch.stack([ins[i][3][:0] for i in range(3)]))
    outs, fpos = [[], [], []], [1, 1, 1]
    for slots in ticks:
        got = g.tick(torch.stack([ins[i][2][fpos[i]:fpos[i] + f] for i in slots]), slots,
                     z=torch.stack([ins[i][3][(fpos[i] - 1) * HOP:(fpos[i] - 1 + f) * HOP] for i in slots]))
        for k, i in enumerate(slots):
            outs[i].append(got[k].clone())
            fpos[i] += f
    assert g.verify() == 5 and g.eager_calls == 0
    assert [s.emitted(i) for i in range(3)] == [n * HOP for n in frames]
    for i in range(3):
        assert torch.equal(torch.cat(outs[i]), _one_shot(model, ins[i][2], ins[i][3])), i


def test_prefix_rule_range_word(gpu, knobs):
    """Three ragged ticks of two sessions in flight, the second with session 0's mel * 1e5 (its last frame, the one kept, excepted):
    verify() raises PwvRangeError with .committed == 1 and both sessions stand where a stream that ran tick 1 only stands; the eager
    push_varlen of tick 2 (rerun in fp32, with its warning) and of tick 3 continue the bits of an all-eager stream."""
    from pwv_amd._lib import PwvRangeError
    cfg = _small()
    model, _ = _model(gpu, cfg)
    ins = [_inputs(cfg, L, gpu, seed=40 + i) for i, L in enumerate((720, 480))]
    hot = ins[0][2].clone()
    hot[4:6] *= 1e5                        # frames 4, 5 of the tick that brings session 0 its frames 4, 5, 6
    mel = [hot, ins[1][2]]
    z = [ins[0][3], ins[1][3]]
    counts = [[3, 2], [3, 1], [3, 3]]
    fpos, chunks = [1, 1], []
    for c in counts:
        chunks.append(([mel[i][fpos[i]:fpos[i] + f] for i, f in enumerate(c)],
                       [z[i][(fpos[i] - 1) * HOP:(fpos[i] - 1 + f) * HOP] for i, f in enumerate(c)]))
        fpos = [p + f for p, f in zip(fpos, c)]
    s, ref = model.open_stream(slots=3), model.open_stream(slots=2)
    g = _graphed(knobs, s, cfg, gpu, 3, 800, sample=False)
    for st in (s, ref):
        st.push_varlen([mel[0][:1], mel[1][:1]], slots=[0, 1], z=[z[0][:0], z[1][:0]])
    first = [o.clone() for o in g.tick(chunks[0][0], [0, 1], z=chunks[0][1])]
    g.tick(chunks[1][0], [0, 1], z=chunks[1][1])
    g.tick(chunks[2][0], [0, 1], z=chunks[2][1])
    with pytest.raises(PwvRangeError) as ei:
        g.verify()
    assert ei.value.committed == 1 and s._pending is None
    want = ref.push_varlen(chunks[0][0], slots=[0, 1], z=chunks[0][1])
    assert torch.equal(first[0], want[0]) and torch.equal(first[1], want[1])
    assert [s.emitted(0), s.emitted(1)] == [240, 160]
    assert all(_same_session(s.state(i), ref.state(i)) for i in range(2))
    for j in (1, 2):
        if j == 1:
            with pytest.warns(UserWarning, match='rerun in exact fp32'):
                got = s.push_varlen(chunks[j][0], slots=[0, 1], z=chunks[j][1])
            with pytest.warns(UserWarning, match='rerun in exact fp32'):
                want = ref.push_varlen(chunks[j][0], slots=[0, 1], z=chunks[j][1])
        else:
            got = s.push_varlen(chunks[j][0], slots=[0, 1], z=chunks[j][1])
            want = ref.push_varlen(chunks[j][0], slots=[0, 1], z=chunks[j][1])
        assert torch.equal(got.packed, want.packed) and bool(torch.isfinite(got.packed).all())
    assert [s.emitted(0), s.emitted(1)] == [720, 480]


def test_give_up_word(gpu, knobs):
    """Nothing on the GPU is made to fail: the give-up word is set by a host write, as a launch that gave up would leave it.  The ticks
    behind it are refused on the device (.committed == 0, the sessions unchanged); the graph is dropped and the next tick runs
    eagerly (the persistent launches are suspended) with the same bits; after the suspension a tick captures again and the sessions
    continue bit-identically."""
    from pwv_amd._lib import PwvPersistError
    engine = knobs
    cfg = _small()
    model, _ = _model(gpu, cfg)
    lengths = [960, 640]
    ins = [_inputs(cfg, L, gpu, seed=81 + i) for i, L in enumerate(lengths)]
    counts = [[3, 2], [4, 1], [2, 3], [3, 2]]
    fpos, chunks = [1, 1], []
    for c in counts:
        chunks.append(([ins[i][2][fpos[i]:fpos[i] + f] for i, f in enumerate(c)],
                       [ins[i][3][(fpos[i] - 1) * HOP:(fpos[i] - 1 + f) * HOP] for i, f in enumerate(c)]))
        fpos = [p + f for p, f in zip(fpos, c)]
    s = model.open_stream(slots=3)
    g = _graphed(engine, s, cfg, gpu, 3, 800, sample=False)
    s.push_varlen([ins[0][2][:1], ins[1][2][:1]], slots=[0, 1], z=[ins[0][3][:0], ins[1][3][:0]])
    outs = [[], []]

    def tick(j):
        got = g.tick(chunks[j][0], [0, 1], z=chunks[j][1])
        return [o.clone() for o in got]

    def keep(pieces):
        for i in range(2):
            outs[i].append(pieces[i])

    keep(tick(0))
    assert g.verify() == 1
    before = [s.state(0), s.state(1)]
    torch.cuda.synchronize()
    engine.poke_persist_status(4)
    tick(1)
    tick(2)                                        # refused too: the word is sticky
    with pytest.raises(PwvPersistError) as ei:
        g.verify()
    assert ei.value.committed == 0 and [s.emitted(0), s.emitted(1)] == [240, 160] and s._pending is None
    assert all(_same_session(s.state(i), before[i]) for i in range(2))
    assert engine.persist_suspended() and g.graph is None
    keep(tick(1))                                  # eager: push_varlen(verify=False) on the grouped route
    assert g.eager_calls == 1 and g.captures == 1
    assert g.verify() == 1 and [s.emitted(0), s.emitted(1)] == [560, 240]
    engine.resume_persist()
    with _Log(engine) as lg:
        keep(tick(2))
        _check_packed(lg.log, cfg, [800] * 2, gpu)                  # the warm-up of the new capture
    assert g.captures == 2 and g.eager_calls == 1
    keep(tick(3))
    assert g.verify() == 2 and [s.emitted(0), s.emitted(1)] == lengths
    for i in range(2):
        assert torch.equal(torch.cat(outs[i]), _one_shot(model, ins[i][2], ins[i][3])), i


def test_interleaving_with_push_push_varlen_and_a_uniform_graph(gpu, knobs):
    """One session advanced alternately by ragged ticks, push, push_varlen and the ticks of a uniform GraphedStream on the same stream:
    whoever finds ticks of another in flight settles them first (_ticker), the device table is rewritten from the host's view after
    every eager push and the host's view from the table at every verify() -- the concatenation is the one-shot forward."""
    cfg = _small()
    model, _ = _model(gpu, cfg)
    how = [('ragged', 3), ('uniform', 2), ('ragged', 1), ('push', 2), ('ragged', 4), ('varlen', 1), ('uniform', 2), ('ragged', 2)]
    L = sum(f for _, f in how) * HOP
    _, _, mel_t, z_t = _inputs(cfg, L, gpu, seed=12)
    s = model.open_stream(slots=3)
    r = _graphed(knobs, s, cfg, gpu, 2, 800, sample=False)
    u = s.graphed(1, 2, sample=False)
    s.push(mel_t[None, :1], slots=[1], z=z_t[None, :0])
    outs, fpos, committed = [], 1, 0
    for j, (kind, f) in enumerate(how):
        mel, z = mel_t[fpos:fpos + f], z_t[(fpos - 1) * HOP:(fpos - 1 + f) * HOP]
        fpos += f
        if kind == 'ragged':
            outs.append(r.tick([mel], [1], z=[z])[0].clone())          # (no verify(): the next caller settles it)
            assert s._ticker is r
            with pytest.raises(Exception, match='verify'):
                s.push_varlen([mel], slots=[1], z=[z])                 # pending: the eager calls refuse until verify()
        elif kind == 'uniform':
            outs.append(u.tick(mel[None], [1], z=z[None])[0].clone())
            assert s._ticker is u
        else:
            committed += s.verify() or 0
            assert s._ticker is None and s.emitted(1) == (fpos - 1 - f) * HOP
            outs.append(s.push(mel[None], slots=[1], z=z[None])[0] if kind == 'push' else s.push_varlen([mel], slots=[1], z=[z])[0])
    committed += r.verify()
    assert committed == 6 and s.emitted(1) == L and s.emitted(0) == 0
    assert r.captures == 1 and r.eager_calls == 0 and u.captures == 1 and u.eager_calls == 0
    assert torch.equal(torch.cat(outs), _one_shot(model, mel_t, z_t))


def test_recapture_and_refusals(gpu, knobs, monkeypatch):
    from pwv_amd._lib import PwvError
    engine = knobs
    cfg = _small()
    model, _ = _model(gpu, cfg)
    _, _, mel_t, z_t = _inputs(cfg, 800, gpu, seed=13)
    s = model.open_stream(slots=2)
    g = _graphed(engine, s, cfg, gpu, 2, 480, sample=False)
    with pytest.raises(ValueError, match='fresh.*eager one-frame push'):
        g.tick([mel_t[1:3]], [0], z=[z_t[:160]])
    s.push_varlen([mel_t[:1]], slots=[0], z=[z_t[:0]])
    with pytest.raises(ValueError, match='z.* is required'):
        g.tick([mel_t[1:3]], [0])
    first = g.tick([mel_t[1:3]], [0], z=[z_t[:160]])[0].clone()
    assert g.verify() == 1 and g.eager_calls == 0
    # a tick that does not fit the capture (7 frames + a filler > 6) runs the eager push_varlen
    assert not g.fits([7]) and g.fits([5])
    big = g.tick([mel_t[3:10]], [0], z=[z_t[160:720]])
    assert g.eager_calls == 1 and s._pending is not None and s._ticker is None
    assert g.verify() == 1 and s.emitted(0) == 720
    assert torch.equal(torch.cat([first, big[0]]), _one_shot(model, mel_t[:10], z_t[:720]))
    # new weights in the store: the captured launches point at stale packs -> captured again; the session keeps its history
    model.store.load_dict(O.init_weights(cfg, seed=9))
    twin = model.open_stream(slots=1)
    twin.load_state(0, s.state(0))
    second = g.tick([mel_t[10:11]], [0], z=[z_t[720:]])[0].clone()
    assert g.captures == 2 and g.verify() == 1
    assert torch.equal(second, twin.push_varlen([mel_t[10:11]], z=[z_t[720:]])[0])
    # refusals at construction
    with pytest.raises(PwvError, match='at least 3 slots'):
        s.graphed_varlen(3, 800)
    with pytest.raises(PwvError, match='multiple of hop_length'):
        s.graphed_varlen(2, 500)
    with pytest.raises(PwvError, match='at least 160'):
        s.graphed_varlen(2, 80)
    monkeypatch.setattr(engine, 'PERSIST_AUTO_MAX_ROWS', 400)
    with pytest.raises(PwvError, match='PERSIST_AUTO_MAX_ROWS'):
        s.graphed_varlen(2, 480)
    monkeypatch.undo()
    engine.PERSIST = False
    with pytest.raises(PwvError, match='PWV_PERSIST=0'):
        s.graphed_varlen(2, 480)


@pytest.fixture()
def hop_80_afterwards():
    """The hparams are a process-wide singleton: leave the reference's hop behind for whatever runs next."""
    yield
    set_hparams(small_cfg())


@pytest.mark.parametrize('hop,capacity,frames', [(16, (3, 320), [5, 2]), (96, (3, 768), [3, 1])], ids=['hop16', 'hop96'])
@pytest.mark.parametrize('precision', ['f16x3', 'f32'])
def test_hops_16_and_96(gpu, knobs, hop_80_afterwards, precision, hop, capacity, frames):
    """At hop 16 a session needs two frames (32 rows): min_frames = 2, and the fillers have two frames; at hop 96 one."""
    from pwv_amd import graph
    assert hop in HOP_CASES and graph.packed_filler_rows(hop) // hop == (2 if hop == 16 else 1)
    cfg = hop_cfg(hop)
    model, _ = _model(gpu, cfg, precision)
    _tick_against_push_varlen(knobs, model, cfg, gpu, 3, capacity, [2, 0], frames, hop=hop)


def test_generate_cli_stream_graph_writes_the_files_of_stream(gpu, tmp_path, monkeypatch):
    """`generate default --stream=3 --graph` on the tiny case of test_generate_cli_stream_pushes_once_per_tick writes the files
    `--stream=3` writes, bit for bit (the OS seeds the CLI draws are made the same for both runs), through graphed ticks."""
    from pwv_amd import engine, graph
    from pwv_amd.generate import _fire, generate
    from pwv_amd.hparam import hparam as hp
    rng = np.random.default_rng(4)
    frames = [3, 21, 9]
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
    ticks = []
    real_tick = graph.GraphedRaggedStream.tick

    def counting(self, *a, **k):
        ticks.append(self.eager_calls)
        return real_tick(self, *a, **k)

    monkeypatch.setattr(graph.GraphedRaggedStream, 'tick', counting)
    replays = []
    real_replay = graph.GraphedRaggedStream._replay

    def replaying(self, *a, **k):
        replays[:] = [replays[0] + 1 if replays else 1]
        return real_replay(self, *a, **k)

    monkeypatch.setattr(graph.GraphedRaggedStream, '_replay', replaying)
    files = {}
    for how, argv in (('eager', ['default', '--stream=3']), ('graph', ['default', '--stream=3', '--graph'])):
        drawn = iter(range(1000, 2000))
        monkeypatch.setattr(engine, 'os_seed', lambda: next(drawn))
        logdir = tmp_path / how
        monkeypatch.setenv('PWV_LOGDIR', str(logdir))
        pred = _fire(generate, argv)
        assert [p.shape for p in pred] == [((f - 1) * 80, 1) for f in frames]
        files[how] = [(logdir / ('pred_%d.wav' % i)).read_bytes() for i in range(3)]
        with np.load(str(logdir / 'pred_wav_varlen.npz')) as npz:
            files[how] += [npz['pred_%d' % i].tobytes() for i in range(3)]
    # ceil(20 / 3) ticks behind the one-frame push; the first -- short last chunks in all three slots, 8 of 9 frames -- does not fit and
    # runs eagerly, every other one is a graph replay
    assert ticks == [0, 1, 1, 1, 1, 1, 1] and replays == [6]
    assert files['graph'] == files['eager']
    with pytest.raises(ValueError, match='--graph applies to --stream'):
        _fire(generate, ['default', '--graph'])
