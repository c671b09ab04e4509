"""GPU: a streaming tick replayed as ONE graph with the commit on the device (graph.GraphedStream, csrc/pwv_stream_tick.hip).  The
contract of push does not change: a tick gives the bits of the eager push from the same state, the ticks of a session concatenate to
the one-shot forward, a session does not depend on its companions (filler entries included), and a tick is a transaction -- now one
that the device itself commits or refuses, so ticks are enqueued back to back.  Every case first shows, from engine.EVENT_LOG during
the warm-up of the capture, that each flow is one streaming persistent launch."""
import numpy as np
import pytest
import torch

from oracle import iaf_oracle as O
from tests.test_gpu_stream import _inputs, _model, _one_shot, _small, _small_wide
from tests.test_gpu_stream_persist import _Log, _random_state, knobs      # noqa: F401  (knobs: the fixture)

pytestmark = pytest.mark.gpu
HOP = 80


def _graphed(engine, s, cfg, gpu, n, frames, **kw):
    """s.graphed(n, frames) with the route of its warm-up ticks checked: one streaming persistent launch per flow, nothing else."""
    with _Log(engine) as lg:
        g = s.graphed(n, frames, **kw)
    lg.check(cfg, [n * frames * HOP] * kw.get('warmup', 2), gpu)
    assert g.captures == 1 and g.eager_calls == 0
    return g


def _mid_utterance(s, rng, gpu, emitted=None):
    """Every slot of `s` running, as load_state leaves it: a random kept frame, some samples emitted."""
    for sl in range(s.n_slots):
        st = s.state(sl)
        st['kept'] = torch.from_numpy(rng.uniform(-1, 1, (s.n_mels,)).astype(np.float32)).to(gpu)
        st['running'], st['emitted'] = True, HOP * (3 + sl) if emitted is None else emitted
        s.load_state(sl, st)


def _same_session(a, b):
    return (torch.equal(a['hist'], b['hist']) and torch.equal(a['kept'], b['kept']) and a['running'] == b['running']
            and a['emitted'] == b['emitted'])


_TICK_SHAPES = [('small_wide', 1, [0], 1), ('small_wide', 3, [0, 1, 2], 2), ('default', 2, [0, 1], 7), ('default', 8, [5, 2, 7, 0], 1)]


@pytest.mark.parametrize('shape', _TICK_SHAPES, ids=['wide_1x80', 'wide_3x160', 'default_2x560', 'default_subset_permuted'])
@pytest.mark.parametrize('precision', ['f16x3', 'f32'])
def test_tick_against_push(gpu, knobs, precision, shape):
    """One tick and one eager push from the same random non-zero histories (both generations), explicit z: torch.equal outputs, whole
    history arrays (every slot, both generations), kept frames and emitted counts.  On _small_wide T is below most dilations: the
    carry launch sits inside the graph."""
    config, n_slots, slots, f = shape
    cfg = _small_wide() if config == 'small_wide' else O.ModelConfig()
    model, _ = _model(gpu, cfg, precision)
    n, T = len(slots), f * HOP
    rng = np.random.default_rng(17 * n_slots + f)
    mel = torch.from_numpy(rng.uniform(-1, 1, (n, f, cfg.n_mels)).astype(np.float32)).to(gpu)
    z = torch.from_numpy(np.clip(rng.logistic(0, 1, (n, T, 1)), -20, 20).astype(np.float32)).to(gpu)
    res = []
    for graphed in (True, False):
        s = model.open_stream(slots=n_slots)
        g = _graphed(knobs, s, cfg, gpu, n, f, sample=False) if graphed else None
        _mid_utterance(s, np.random.default_rng(5), gpu)
        _random_state(s, 100 + f)
        if graphed:
            out = g.tick(mel, slots, z=z).clone()
            assert s._pending is not None
            assert g.verify() == 1 and s._pending is None
        else:
            out = s.push(mel, slots=slots, z=z)
        res.append((out, s._hist.clone(), s._kept.clone(), [s.emitted(sl) for sl in range(n_slots)], list(s._gen)))
    (out_g, hist_g, kept_g, em_g, gen_g), (out_p, hist_p, kept_p, em_p, gen_p) = res
    assert tuple(out_g.shape) == (n, T, 1) and bool(torch.isfinite(out_g).all())
    assert torch.equal(out_g, out_p), float((out_g - out_p).abs().max())
    assert torch.equal(hist_g, hist_p), int((hist_g != hist_p).sum())
    assert torch.equal(kept_g, kept_p) and em_g == em_p and gen_g == gen_p
    assert em_g == [HOP * (3 + sl) + (T if sl in slots else 0) for sl in range(n_slots)]


@pytest.mark.parametrize('frames', [1, 5])
@pytest.mark.parametrize('config', ['small', 'default'])
def test_pipelined_ticks_equal_the_one_shot_forward(gpu, knobs, config, frames):
    """L = 2400: the session starts with the one-frame eager push, then EVERY tick is enqueued with no verify() in between (each output
    cloned on the stream), one verify() at the end.  The generation flip, the counter and the kept frame move on the device alone."""
    cfg = _small() if config == 'small' else O.ModelConfig()
    L, T = 2400, frames * HOP
    model, _ = _model(gpu, cfg)
    _, _, mel_t, z_t = _inputs(cfg, L, gpu, seed=3)
    s = model.open_stream(slots=1)
    g = _graphed(knobs, s, cfg, gpu, 1, frames, sample=False)      # (its fillers ran on the fresh slot: the start below must not see them)
    assert tuple(s.push(mel_t[None, :1], z=z_t[None, :0]).shape) == (1, 0, 1)
    outs = []
    for j in range(L // T):
        out = g.tick(mel_t[None, 1 + j * frames:1 + (j + 1) * frames], [0], z=z_t[None, j * T:(j + 1) * T])
        outs.append(out[0].clone())
    assert s.emitted(0) == 0                       # nothing has come back to the host yet
    assert g.verify() == L // T
    assert s.emitted(0) == L and g.captures == 1 and g.eager_calls == 0
    got, want = torch.cat(outs), _one_shot(model, mel_t, z_t)
    assert torch.equal(got, want), float((got - want).abs().max())


def test_seeds(gpu, knobs):
    """sample=True, two sessions with seeds (one above 2**63): the ticks of slot i concatenate to IAFVocoder(1, L) drawing from
    noise_seed = seeds[i], noise_offset = 0 -- the sampler inside the graph reads {seed, emitted} from the device table."""
    cfg = _small()
    L, f = 640, 2
    model, _ = _model(gpu, cfg)
    ins = [_inputs(cfg, L, gpu, seed=30 + i) for i in range(2)]
    seeds = [5, (1 << 63) + 9]
    s = model.open_stream(slots=2)
    g = _graphed(knobs, s, cfg, gpu, 2, f, sample=True)
    s.push(torch.stack([ins[0][2][:1], ins[1][2][:1]]), seeds=seeds)
    outs = [[], []]
    for j in range(L // (f * HOP)):
        out = g.tick(torch.stack([ins[i][2][1 + j * f:1 + (j + 1) * f] for i in range(2)]), [0, 1])
        for i in range(2):
            outs[i].append(out[i].clone())
    assert g.verify() == L // (f * HOP)
    assert [s.emitted(i) for i in range(2)] == [L, L] and s._seed == seeds
    for i in range(2):
        assert torch.equal(torch.cat(outs[i]), _one_shot(model, ins[i][2], seed=seeds[i])), i


def test_fillers_and_independence(gpu, knobs):
    """A graph for n = 4 on a 6-slot stream, called with 2 permuted slots (2 filler entries per tick): the called sessions equal the
    same ticks from a 2-session graph; every other slot's current generation, kept frame and emitted count are untouched; and the
    warm-up and the capture -- all fillers -- changed no session."""
    cfg = _small()
    model, _ = _model(gpu, cfg)
    f, called = 2, [4, 1]
    rng = np.random.default_rng(8)
    mels = [torch.from_numpy(rng.uniform(-1, 1, (2, f, cfg.n_mels)).astype(np.float32)).to(gpu) for _ in range(3)]
    zs = [torch.from_numpy(np.clip(rng.logistic(0, 1, (2, f * HOP, 1)), -20, 20).astype(np.float32)).to(gpu) for _ in range(3)]
    a = model.open_stream(slots=6)
    _mid_utterance(a, np.random.default_rng(6), gpu)
    _random_state(a, 9)
    before, hist0 = [a.state(sl) for sl in range(6)], a._hist.clone()
    ga = _graphed(knobs, a, cfg, gpu, 4, f, sample=False)
    assert all(_same_session(a.state(sl), before[sl]) for sl in range(6))          # warm-up and capture: fillers only
    b = model.open_stream(slots=6)
    for sl in range(6):
        b.load_state(sl, before[sl])
    b._hist.copy_(hist0)                        # (both generations as `a` had them: the rows a block pads its histories with included)
    gb = _graphed(knobs, b, cfg, gpu, 2, f, sample=False)
    outs = []
    for g in (ga, gb):
        got = [g.tick(mels[j], called, z=zs[j]).clone() for j in range(3)]
        assert g.verify() == 3
        outs.append(torch.cat(got, dim=1))
    assert torch.equal(outs[0], outs[1])
    for sl in range(6):
        if sl in called:
            assert _same_session(a.state(sl), b.state(sl)) and a.emitted(sl) == before[sl]['emitted'] + 3 * f * HOP
        else:
            assert _same_session(a.state(sl), before[sl]), sl


def test_prefix_rule_range_word(gpu, knobs):
    """Three ticks in flight, the second with mel * 1e5 (its last frame, the one kept, excepted): verify() raises PwvRangeError with
    .committed == 1 and the session stands where a stream that ran tick 1 only stands; the eager push of chunk 2 (rerun in fp32, with
    its warning) and of chunk 3 then give what tests/test_gpu_stream.py::test_range_rerun_is_transactional expects."""
    from pwv_amd._lib import PwvRangeError
    from pwv_amd.models import IAFVocoder
    cfg = _small()
    model, _ = _model(gpu, cfg)
    m32 = IAFVocoder(batch_size=1, length=80, store=model.store, precision='f32')
    L = 720
    _, _, mel_t, z_t = _inputs(cfg, L, gpu, seed=40)
    mel_t = mel_t.clone()
    mel_t[4:6] *= 1e5                      # frames 4, 5 of the chunk that brings frames 4, 5, 6
    chunks = [(mel_t[None, 1 + 3 * j:4 + 3 * j], z_t[None, 240 * j:240 * (j + 1)]) for j in range(3)]
    s = model.open_stream(slots=1)
    g = _graphed(knobs, s, cfg, gpu, 1, 3, sample=False)
    s.push(mel_t[None, :1], z=z_t[None, :0])
    first = g.tick(chunks[0][0], [0], z=chunks[0][1]).clone()
    g.tick(chunks[1][0], [0], z=chunks[1][1])
    g.tick(chunks[2][0], [0], z=chunks[2][1])
    with pytest.raises(PwvRangeError) as ei:
        g.verify()
    assert ei.value.committed == 1
    assert torch.equal(first[0], _one_shot(model, mel_t[:4], z_t[:240]))
    ref = model.open_stream(slots=1)
    ref.push(mel_t[None, :1], z=z_t[None, :0])
    ref.push(chunks[0][0], z=chunks[0][1])
    assert s.emitted(0) == 240 and _same_session(s.state(0), ref.state(0)) and s._pending is None
    before = s.state(0)
    with pytest.warns(UserWarning, match='rerun in exact fp32'):
        tripped = s.push(chunks[1][0], z=chunks[1][1])
    assert s.emitted(0) == 480 and bool(torch.isfinite(tripped).all())
    s32 = m32.open_stream(slots=1)
    s32.load_state(0, before)
    assert torch.equal(tripped, s32.push(chunks[1][0], z=chunks[1][1]))
    s2 = model.open_stream(slots=1)
    s2.load_state(0, s32.state(0))
    after = s.push(chunks[2][0], z=chunks[2][1])
    assert torch.equal(after, s2.push(chunks[2][0], z=chunks[2][1])) and s.emitted(0) == L


def test_give_up_word(gpu, knobs):
    """Nothing on the GPU is made to fail: the give-up word is set by a host write, as a launch that gave up would leave it.  The tick
    behind it is refused on the device (.committed == 0, the session unchanged); the next tick runs eagerly (the persistent launches
    are suspended) with the same bits; after the suspension a tick captures again and the session continues bit-identically."""
    from pwv_amd._lib import PwvPersistError
    engine = knobs
    cfg = _small()
    L, f = 960, 3
    T = f * HOP
    model, _ = _model(gpu, cfg)
    _, _, mel_t, z_t = _inputs(cfg, L, gpu, seed=81)
    chunk = lambda j: (mel_t[None, 1 + f * j:1 + f * (j + 1)], z_t[None, T * j:T * (j + 1)])      # noqa: E731
    s = model.open_stream(slots=1)
    g = _graphed(engine, s, cfg, gpu, 1, f, sample=False)
    s.push(mel_t[None, :1], z=z_t[None, :0])
    outs = [g.tick(chunk(0)[0], [0], z=chunk(0)[1])[0].clone()]
    assert g.verify() == 1
    before = s.state(0)
    torch.cuda.synchronize()
    engine.poke_persist_status(4)
    g.tick(chunk(1)[0], [0], z=chunk(1)[1])
    with pytest.raises(PwvPersistError) as ei:
        g.verify()
    assert ei.value.committed == 0 and s.emitted(0) == T and _same_session(s.state(0), before) and s._pending is None
    assert engine.persist_suspended() and g.graph is None
    with _Log(engine) as lg:
        outs.append(g.tick(chunk(1)[0], [0], z=chunk(1)[1])[0].clone())
        assert [e[0] for e in lg.log] == ['layer_stream'] * cfg.n_iaf
    assert g.eager_calls == 1 and g.captures == 1
    assert g.verify() == 1 and s.emitted(0) == 2 * T
    engine.resume_persist()
    with _Log(engine) as lg:
        outs.append(g.tick(chunk(2)[0], [0], z=chunk(2)[1])[0].clone())
        lg.check(cfg, [T] * 2, gpu)                 # the warm-up of the new capture
    assert g.captures == 2 and g.eager_calls == 1
    outs.append(g.tick(chunk(3)[0], [0], z=chunk(3)[1])[0].clone())
    assert g.verify() == 2 and s.emitted(0) == L
    assert torch.equal(torch.cat(outs), _one_shot(model, mel_t, z_t))


def test_interleaving_with_push_and_push_varlen(gpu, knobs):
    """One session advanced alternately by tick, push and push_varlen: the device table is rewritten from the host's view after every
    eager push, the host's view from the table at every verify() -- the concatenation is the one-shot forward."""
    cfg = _small()
    f = 2
    T = f * HOP
    L = 6 * T
    model, _ = _model(gpu, cfg)
    _, _, mel_t, z_t = _inputs(cfg, L, gpu, seed=12)
    s = model.open_stream(slots=2)
    g = _graphed(knobs, s, cfg, gpu, 1, f, sample=False)
    s.push(mel_t[None, :1], slots=[1], z=z_t[None, :0])
    outs = []
    for j, how in enumerate(['tick', 'push', 'varlen', 'tick', 'tick', 'push']):
        mel, z = mel_t[1 + f * j:1 + f * (j + 1)], z_t[T * j:T * (j + 1)]
        if how == 'tick':
            outs.append(g.tick(mel[None], [1], z=z[None])[0].clone())
            with pytest.raises(Exception, match='verify'):
                s.push(mel[None], slots=[1], z=z[None])          # pending: the eager calls refuse until verify()
            assert g.verify() == 1
        elif how == 'push':
            outs.append(s.push(mel[None], slots=[1], z=z[None])[0])
        else:
            outs.append(s.push_varlen([mel], slots=[1], z=[z])[0])
        assert s.emitted(1) == (j + 1) * T
    assert g.captures == 1 and g.eager_calls == 0 and s.emitted(0) == 0
    assert torch.equal(torch.cat(outs), _one_shot(model, mel_t, z_t))


def test_recapture_and_refusals(gpu, knobs):
    from pwv_amd._lib import PwvError
    engine = knobs
    cfg = _small()
    f = 2
    T = f * HOP
    model, _ = _model(gpu, cfg)
    _, _, mel_t, z_t = _inputs(cfg, 2 * T, gpu, seed=13)
    s = model.open_stream(slots=2)
    g = _graphed(engine, s, cfg, gpu, 1, f, sample=False)
    with pytest.raises(ValueError, match='fresh'):
        g.tick(mel_t[None, 1:1 + f], [0], z=z_t[None, :T])
    s.push(mel_t[None, :1], slots=[0], z=z_t[None, :0])
    with pytest.raises(ValueError, match='z .* is required'):
        g.tick(mel_t[None, 1:1 + f], [0])
    first = g.tick(mel_t[None, 1:1 + f], [0], z=z_t[None, :T]).clone()
    assert g.verify() == 1
    # new weights in the store: the captured launches point at stale packs -> captured again; the session keeps its history
    model.store.load_dict(O.init_weights(cfg, seed=9))
    twin = model.open_stream(slots=1)
    twin.load_state(0, s.state(0))
    second = g.tick(mel_t[None, 1 + f:1 + 2 * f], [0], z=z_t[None, T:]).clone()
    assert g.captures == 2 and g.verify() == 1
    assert torch.equal(second, twin.push(mel_t[None, 1 + f:1 + 2 * f], z=z_t[None, T:])) and not torch.equal(first, second)
    # refusals
    with pytest.raises(ValueError, match='at least 3 slots'):
        s.graphed(3, f)
    gs = s.graphed(1, f, sample=True, warmup=1)
    with pytest.raises(ValueError, match='z is not taken'):
        gs.tick(mel_t[None, 1:1 + f], [0], z=z_t[None, :T])
    engine.PERSIST = False
    with pytest.raises(PwvError, match='PWV_PERSIST=0'):
        s.graphed(1, f)


def test_a_filler_follows_its_slots_eager_pushes(gpu, knobs):
    """Slot 1 is the filler of every tick of slot 0 and is advanced by eager pushes in between: the filler entry must write the
    generation slot 1 does NOT stand on after each of them (its row of the device table is rewritten like a called slot's).  Both
    sessions equal their one-shot forwards."""
    cfg = _small()
    f = 2
    T = f * HOP
    L = 3 * T
    model, _ = _model(gpu, cfg)
    ins = [_inputs(cfg, L, gpu, seed=50 + i) for i in range(2)]
    s = model.open_stream(slots=2)
    g = _graphed(knobs, s, cfg, gpu, 2, f, sample=False)
    s.push(torch.stack([ins[0][2][:1], ins[1][2][:1]]), z=torch.stack([ins[0][3][:0], ins[1][3][:0]]))
    outs = [[], []]
    for j in range(3):
        mel = [ins[i][2][None, 1 + f * j:1 + f * (j + 1)] for i in range(2)]
        z = [ins[i][3][None, T * j:T * (j + 1)] for i in range(2)]
        outs[0].append(g.tick(mel[0], [0], z=z[0])[0].clone())
        assert g.verify() == 1
        outs[1].append(s.push(mel[1], slots=[1], z=z[1])[0])
    assert [s.emitted(i) for i in range(2)] == [L, L] and g.captures == 1
    for i in range(2):
        assert torch.equal(torch.cat(outs[i]), _one_shot(model, ins[i][2], ins[i][3])), i
