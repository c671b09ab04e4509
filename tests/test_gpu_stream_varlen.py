"""GPU: RAGGED streaming pushes (StreamingVocoder.push_varlen): sessions that get different numbers of frames, fresh and running ones
mixed, in ONE packed persistent launch per flow (pwv_persist_args.cu_rows with hist->cu_rows, stack_persist_ragged_kernel<F32, MODE>;
engine.run_flow_stream with a geometry).  The contract is push's: the pieces of a session concatenate to its own one-shot forward bit
for bit, a session does not depend on its companions, a push is a transaction.  Every case that claims the new kernel first shows from
engine.EVENT_LOG / PERSIST_ARGS_HOOK that it RAN (cu_rows, unit_map and hist all set, and in which instantiation).
(Every configuration here runs hop 80, so a session under 32 rows cannot be made: the grouped route is reached with PERSIST = False and
through a suspension.  tests/test_gpu_hop_geometry.py reaches it at hop 16 with PERSIST at its default: a one-frame session of 16 rows.)"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import iaf_oracle as O
from tests.guarded import Guard
from tests.test_gpu_stream import _inputs, _model, _one_shot, _small, _small_wide
from tests.test_gpu_stream_persist import _Log, _random_state, _short_expected, knobs  # noqa: F401  (knobs: a fixture)

pytestmark = pytest.mark.gpu
HOP = 80


class _Ragged:
    """Per slot an utterance (mel, z) and a frame cursor; tick({slot: frames}) gives those slots their next frames in ONE push_varlen."""

    def __init__(self, s):
        self.s, self.utt, self.fpos, self.out = s, {}, {}, {}

    def start(self, slot, mel_t, z_t=None):
        self.utt[slot], self.fpos[slot], self.out[slot] = (mel_t, z_t), 0, []

    def tick(self, counts, **kw):
        from pwv_amd.stream import push_samples
        slots = list(counts)
        mels, zs, want = [], [], []
        for sl in slots:
            mel, z = self.utt[sl]
            f = counts[sl]
            T = push_samples(f, self.fpos[sl] == 0, HOP)
            mels.append(mel[self.fpos[sl]:self.fpos[sl] + f])
            e = self.s.emitted(sl)
            if z is not None:
                zs.append(z[e:e + T])
            want.append(T)
        got = self.s.push_varlen(mels, slots=slots, z=zs if zs else None, **kw)
        assert [tuple(g.shape) for g in got] == [(T, 1) for T in want] and tuple(got.packed.shape) == (sum(want), 1)
        for i, sl in enumerate(slots):
            self.out[sl].append(got[i])
            self.fpos[sl] += counts[sl]
        return got, sum(want)

    def result(self, slot):
        return torch.cat(self.out[slot])


class _Hook:
    """PERSIST_ARGS_HOOK inside the block: per persistent launch (precision, cu_rows set, unit_map set, hist set, hist->cu_rows == cu_rows)."""

    def __init__(self, engine):
        self.engine, self.seen = engine, []

    def __enter__(self):
        from pwv_amd import _lib

        def hook(pa):
            same = False
            if pa.hist:
                sa = ctypes.cast(pa.hist, ctypes.POINTER(_lib.StreamArgs)).contents
                same = bool(sa.cu_rows) and sa.cu_rows == pa.cu_rows
            self.seen.append((int(pa.precision), bool(pa.cu_rows), bool(pa.unit_map), bool(pa.hist), same))
        self.engine.PERSIST_ARGS_HOOK = hook
        return self

    def __exit__(self, *exc):
        self.engine.PERSIST_ARGS_HOOK = None


def _check_packed(log, cfg, rows_per_push, gpu):
    """Every push (of `rows` packed rows, 0: nothing launched) took the PACKED route: per flow one ('stream_ragged', ., ., 'packed') entry and one
    streaming persistent launch with layer 0 folded and the tail inside, in the instantiation the plan predicts.  Returns the
    instantiations ([7]: 1 = short-input)."""
    flows = [list(d) for d in cfg.dilations[:cfg.n_iaf]]
    assert not [e for e in log if e[0] not in ('persist', 'stream_ragged')], [e[0] for e in log]
    assert all(e[3] == 'packed' for e in log if e[0] == 'stream_ragged'), [e for e in log if e[0] == 'stream_ragged']
    per = [e for e in log if e[0] == 'persist']
    launched = [r for r in rows_per_push if r > 0]
    assert len(per) == len(launched) * len(flows) == len([e for e in log if e[0] == 'stream_ragged']), (len(per), launched)
    kinds, k = [], 0
    for rows in launched:
        for dil in flows:
            e = per[k]
            k += 1
            assert e[3] == 2 and e[8] == 1 and e[5] == 1 and e[6] == 1 and e[4] == len(dil) - 1, e
            assert e[7] == _short_expected(rows, max(dil), gpu), (rows, e[7])
            kinds.append(e[7])
    return kinds


# frames per tick and session (None: the session sits the tick out).  Tick 1 pairs session 0 with ONE frame (T = hop = 80, below most
# dilations) with session 1's first 8 frames (T = 560 >= 512, the largest dilation); session 2 starts with one frame (T = 0: committed,
# no launch); the sessions start and end at different ticks, each with a short last chunk; 80-row chunks put unit boundaries inside
# sessions and session boundaries inside units.
_SCHEDULE = {0: [5, 1, 12, 3, 1, None],
             1: [None, 8, 10, 1, 7, 2],
             2: [None, None, 1, 9, 4, None],
             3: [20, 2, None, 6, None, 3]}


def _run_schedule(model, cfg, gpu, schedule, seed0, with_z=True, seeds=None):
    S = len(schedule)
    ins = {sl: _inputs(cfg, (sum(f for f in fr if f) - 1) * HOP, gpu, seed=seed0 + sl) for sl, fr in schedule.items()}
    s = model.open_stream(slots=S)
    fd = _Ragged(s)
    for sl in schedule:
        fd.start(sl, ins[sl][2], ins[sl][3] if with_z else None)
    rows = []
    for k in range(len(schedule[0])):
        counts = {sl: fr[k] for sl, fr in schedule.items() if fr[k]}
        kw = {}
        if seeds is not None:
            kw['seeds'] = [seeds[sl] if fd.fpos[sl] == 0 else None for sl in counts]
        rows.append(fd.tick(counts, **kw)[1])
    return s, fd, ins, rows


@pytest.mark.parametrize('config', ['default', 'small_wide'])
@pytest.mark.parametrize('precision', ['f16x3', 'f32'])
def test_contract_short_input_instantiation(gpu, knobs, precision, config):
    """Four sessions of different lengths on schedules of their own (_SCHEDULE): every session's pieces are torch.equal to its own
    IAFVocoder(1, L_i) one-shot forward; every launching push is one packed streaming launch per flow."""
    from pwv_amd import _lib
    cfg = O.ModelConfig() if config == 'default' else _small_wide()
    model, _ = _model(gpu, cfg, precision)
    with _Log(knobs) as lg, _Hook(knobs) as hk:
        s, fd, ins, rows = _run_schedule(model, cfg, gpu, _SCHEDULE, 300)
        kinds = _check_packed(lg.log, cfg, rows, gpu)
    assert rows[1] == 80 + 560 + 160 and rows[2] == 960 + 800    # (tick 1: sessions 0, 1 and 3; tick 2: session 2's single frame adds no rows)
    assert set(kinds) == {1}, kinds                                # short inputs: the short-input instantiation
    want_prec = _lib.PREC_F32 if precision == 'f32' else _lib.PREC_F16X3
    assert hk.seen and all(v == (want_prec, True, True, True, True) for v in hk.seen), hk.seen
    for sl in _SCHEDULE:
        L = ins[sl][3].shape[0]
        assert s.emitted(sl) == L
        want = _one_shot(model, ins[sl][2], ins[sl][3])
        assert torch.equal(fd.result(sl), want), (sl, float((fd.result(sl) - want).abs().max()))


@pytest.mark.parametrize('precision', ['f16x3', 'f32'])
def test_contract_general_instantiation(gpu, knobs, precision):
    """Default model, 8 sessions: two ticks of ~ 4000 samples each (one of them gives session 7 a single frame: T = 80 next to T = 4160)
    run the general instantiation, the short last chunks the short-input one; bits as above."""
    cfg = O.ModelConfig()
    model, _ = _model(gpu, cfg, precision)
    sched = {i: [51 + i, 1 if i == 7 else 52, 3 + i] for i in range(8)}
    with _Log(knobs) as lg, _Hook(knobs) as hk:
        s, fd, ins, rows = _run_schedule(model, cfg, gpu, sched, 320)
        kinds = _check_packed(lg.log, cfg, rows, gpu)
    assert rows[1] == 7 * 4160 + 80
    n = cfg.n_iaf
    assert kinds[:2 * n] == [0] * (2 * n) and kinds[2 * n:] == [1] * n, kinds
    assert all(v[1:] == (True, True, True, True) for v in hk.seen), hk.seen
    for sl in sched:
        want = _one_shot(model, ins[sl][2], ins[sl][3])
        assert torch.equal(fd.result(sl), want), (sl, float((fd.result(sl) - want).abs().max()))


@pytest.mark.parametrize('precision', ['f16x3', 'f32'])
def test_contract_with_seeds(gpu, knobs, precision):
    """Without z: session i draws from its own counter stream (seeds[i] at its first push, counter = emitted afterwards) and equals the
    one-shot model with noise_seed = seeds[i], noise_offset = 0."""
    cfg = O.ModelConfig()
    model, _ = _model(gpu, cfg, precision)
    seeds = {0: 11, 1: (1 << 63) + 5, 2: 0, 3: 123456789012}
    with _Log(knobs) as lg:
        s, fd, ins, rows = _run_schedule(model, cfg, gpu, _SCHEDULE, 340, with_z=False, seeds=seeds)
        _check_packed(lg.log, cfg, rows, gpu)
    for sl in _SCHEDULE:
        want = _one_shot(model, ins[sl][2], None, seed=seeds[sl])
        assert torch.equal(fd.result(sl), want), (sl, float((fd.result(sl) - want).abs().max()))
    with pytest.raises(ValueError, match='running'):
        s.push_varlen([ins[0][2][:2], ins[1][2][:2]], slots=[0, 1], seeds=[3, None])


def _two_streams(model, gpu, n_slots, running, seed):
    """Two streams in the same state: random histories in both generations, the slots in `running` running (a random kept frame, some
    samples emitted) -- the second brought there with state / load_state."""
    a = model.open_stream(slots=n_slots)
    _random_state(a, seed)
    g = torch.Generator(device='cpu').manual_seed(seed + 1)
    for sl in running:
        st = a.state(sl)
        st.update(running=True, emitted=800 + 80 * sl, kept=torch.empty(a.n_mels).uniform_(-1, 1, generator=g).to(gpu))
        a.load_state(sl, st)
    b = model.open_stream(slots=n_slots)
    b._hist.copy_(a._hist)
    for sl in range(n_slots):
        b.load_state(sl, a.state(sl))
    assert torch.equal(a._hist, b._hist) and torch.equal(a._kept, b._kept)
    return a, b


def _ragged_against_grouped(engine, model, cfg, gpu, n_slots, pushes, running, seed, route='packed'):
    """One push_varlen of `pushes` = [(slot, frames)] against what a caller did before: one uniform push per (frames, fresh or running)
    group, from the same state.  Returns nothing: asserts torch.equal pieces and torch.equal written blocks (whole blocks)."""
    from pwv_amd.stream import push_samples
    rng = np.random.default_rng(seed)
    a, b = _two_streams(model, gpu, n_slots, running, seed)
    before = a._hist.clone()
    mels = [torch.from_numpy(rng.uniform(-1, 1, (f, cfg.n_mels)).astype(np.float32)).to(gpu) for _, f in pushes]
    Ts = [push_samples(f, sl not in running, HOP) for sl, f in pushes]
    zs = [torch.from_numpy(np.clip(rng.logistic(0, 1, (T, 1)), -20, 20).astype(np.float32)).to(gpu) for T in Ts]
    slots = [sl for sl, _ in pushes]
    with _Log(engine) as lg:
        got = a.push_varlen(mels, slots=slots, z=zs)
        if route == 'packed':
            _check_packed(lg.log, cfg, [sum(Ts)], gpu)
        else:
            assert [e[3] for e in lg.log if e[0] == 'stream_ragged'] == ['grouped'] * cfg.n_iaf, lg.log
            assert not [e for e in lg.log if e[0] == 'persist'] and [e for e in lg.log if e[0] == 'layer_stream']
    groups = {}
    for i, (sl, f) in enumerate(pushes):
        groups.setdefault((f, sl in running), []).append(i)
    saved = engine.PERSIST
    engine.PERSIST = 'auto' if saved is False else saved
    try:
        for (f, _), members in groups.items():
            want = b.push(torch.stack([mels[i] for i in members]), slots=[slots[i] for i in members], z=torch.stack([zs[i] for i in members]))
            for k, i in enumerate(members):
                assert torch.equal(got[i], want[k]), (i, float((got[i] - want[k]).abs().max()))
    finally:
        engine.PERSIST = saved
    for sl in slots:
        assert a._gen[sl] == b._gen[sl] == 1 and a.emitted(sl) == b.emitted(sl)
        assert torch.equal(a._hist[2 * sl + 1], b._hist[2 * sl + 1]), (sl, int((a._hist[2 * sl + 1] != b._hist[2 * sl + 1]).sum()))
        assert torch.equal(a._hist[2 * sl], before[2 * sl])                        # the generation that was read
    idle = [blk for sl in range(n_slots) if sl not in slots for blk in (2 * sl, 2 * sl + 1)]
    assert torch.equal(a._hist[idle], before[idle])
    assert torch.equal(a._kept, b._kept)


# (slot, frames): fresh and running mixed, T from 80 (a unit spans two sessions; every history is carried over) to 4000, a session with
# one frame to a fresh slot (slot 6: T = 0), slots out of order
_PUSH_A = [(5, 10), (2, 1), (7, 50), (0, 11), (3, 2), (6, 1), (1, 1), (4, 7)]
_RUNNING_A = [5, 2, 7, 1]


@pytest.mark.parametrize('config', ['default', 'small_wide'])
@pytest.mark.parametrize('precision', ['f16x3', 'f32'])
def test_kernel_against_kernel(gpu, knobs, precision, config):
    """The packed launch against the grouped uniform pushes (the parent's kernels) from the same random state: same pieces, same
    written generation byte for byte over the whole block of every pushed session; 80- and 160-row sessions put session boundaries
    inside units."""
    cfg = O.ModelConfig() if config == 'default' else _small_wide()
    model, _ = _model(gpu, cfg, precision)
    _ragged_against_grouped(knobs, model, cfg, gpu, 9, _PUSH_A, _RUNNING_A, seed=21)
    # many short sessions in a row: every unit of the launch spans two (80 rows = 2.5 units), fresh ones among them
    _ragged_against_grouped(knobs, model, cfg, gpu, 9, [(i, 2 if i % 3 == 0 else 1) for i in range(9)], [1, 2, 4, 5, 7, 8], seed=22)


@pytest.mark.parametrize('precision', ['f16x3', 'f32'])
def test_kernel_against_kernel_general_instantiation(gpu, knobs, precision):
    """As above at more than 28672 rows on 256 CUs (the general instantiation): 12 sessions around 3200 samples, three of 80."""
    cfg = O.ModelConfig()
    model, _ = _model(gpu, cfg, precision)
    pushes = [(i, 1 if i % 5 == 4 else 38 + 2 * i) for i in range(15)]
    rows = sum(f * HOP for i, f in pushes) - HOP * len([i for i, _ in pushes if i % 2])      # (odd slots are fresh)
    assert _short_expected(rows, 512, gpu) == 0
    _ragged_against_grouped(knobs, model, cfg, gpu, 15, pushes, [i for i in range(15) if i % 2 == 0], seed=23)


@pytest.mark.parametrize('precision', ['f16x3', 'f32'])
def test_grouped_route_with_persist_off(gpu, knobs, precision):
    """engine.PERSIST = False: the sessions are grouped by length and run as the uniform per-layer streaming flow -- the route is in
    EVENT_LOG, the bits and the written blocks are those of the uniform pushes (and so of the packed route)."""
    cfg = O.ModelConfig()
    model, _ = _model(gpu, cfg, precision)
    knobs.PERSIST = False
    _ragged_against_grouped(knobs, model, cfg, gpu, 9, _PUSH_A, _RUNNING_A, seed=21, route='grouped')


@pytest.mark.parametrize('precision', ['f16x3', 'f32'])
def test_a_session_does_not_depend_on_its_companions(gpu, knobs, precision):
    """Session X's piece and written block do not change when its companions, their order or their lengths change."""
    cfg = O.ModelConfig()
    model, _ = _model(gpu, cfg, precision)
    rng = np.random.default_rng(31)

    def mel(f):
        return torch.from_numpy(rng.uniform(-1, 1, (f, cfg.n_mels)).astype(np.float32)).to(gpu)

    def noise(T):
        return torch.from_numpy(np.clip(rng.logistic(0, 1, (T, 1)), -20, 20).astype(np.float32)).to(gpu)

    X, fx = 3, 6
    mx, zx = mel(fx), noise(fx * HOP)
    res = []
    for companions in ([], [(0, 1), (5, 30)], [(5, 2), (1, 9), (0, 14), (4, 1)], [(4, 6), (0, 6)]):
        a, _ = _two_streams(model, gpu, 6, [X, 0, 4], seed=33)
        order = companions[:len(companions) // 2] + [(X, fx)] + companions[len(companions) // 2:]
        mels = [mx if sl == X else mel(f) for sl, f in order]
        zs = [zx if sl == X else noise((f - (0 if sl in (0, 4) else 1)) * HOP) for sl, f in order]
        with _Log(knobs) as lg:
            got = a.push_varlen(mels, slots=[sl for sl, _ in order], z=zs)
            assert all(e[3] == 'packed' for e in lg.log if e[0] == 'stream_ragged') and lg.log
        res.append((got[[sl for sl, _ in order].index(X)].clone(), a._hist[2 * X + 1].clone()))
    for piece, block in res[1:]:
        assert torch.equal(piece, res[0][0]) and torch.equal(block, res[0][1])


@pytest.mark.parametrize('precision', ['f16x3', 'f32'])
def test_bystanders_and_guard_bands(gpu, knobs, precision):
    """The histories inside a 0xFF-filled buffer (hist_alloc, tests/guarded.py): after ragged pushes on the packed route (the general instantiation
    included) the bands are untouched, no NaN came in, and the blocks of a slot that was never pushed are still zero."""
    cfg = O.ModelConfig()
    model, _ = _model(gpu, cfg, precision)
    bands = Guard(band_bytes=1 << 18)          # 0xFF on either side of the zero-filled histories, compared byte for byte afterwards
    S = 17                                   # slot 7 is never pushed
    s = model.open_stream(slots=S, hist_alloc=lambda floats: bands.allocate((floats,), torch.float32, gpu, 0.0))
    rng = np.random.default_rng(6)
    ticks = [{i: 30 + i for i in range(S) if i != 7},                    # ~ 37000 rows: general
             {0: 1, 16: 1, 3: 12},
             {i: (1 if i % 4 == 0 else 25 + i) for i in range(S) if i != 7},
             {16: 3, 0: 40, 9: 1}]
    rows = []
    with _Log(knobs) as lg:
        for counts in ticks:
            slots = list(counts)
            Ts = [(counts[sl] - (0 if s._running[sl] else 1)) * HOP for sl in slots]
            mels = [torch.from_numpy(rng.uniform(-1, 1, (counts[sl], cfg.n_mels)).astype(np.float32)).to(gpu) for sl in slots]
            zs = [torch.from_numpy(np.clip(rng.logistic(0, 1, (T, 1)), -20, 20).astype(np.float32)).to(gpu) for T in Ts]
            out = s.push_varlen(mels, slots=slots, z=zs)
            assert bool(torch.isfinite(out.packed).all()) and out.packed.shape[0] == sum(Ts)
            rows.append(sum(Ts))
        kinds = _check_packed(lg.log, cfg, rows, gpu)
    assert 0 in kinds and 1 in kinds, kinds
    torch.cuda.synchronize()
    bands.check()
    blocks = bands.allocations[0].payload().view(2 * S, -1)
    assert not bool(torch.isnan(blocks).any()) and not bool(blocks[14:16].any())


def _tick_inputs(cfg, gpu, seed):
    """A mixed tick on 4 slots after one uniform push made slots 0 and 1 running: (first mel [2, 11, n_mels], its z, the ragged tick's
    mels, slots, zs)."""
    rng = np.random.default_rng(seed)

    def u(*shape):
        return torch.from_numpy(rng.uniform(-1, 1, shape).astype(np.float32)).to(gpu)
    first, z0 = u(2, 11, cfg.n_mels), u(2, 800, 1)
    counts = [(0, 1), (1, 12), (2, 6), (3, 1)]                  # running 80, running 960, fresh 400, fresh with one frame
    Ts = [80, 960, 400, 0]
    return first, z0, [u(f, cfg.n_mels) for _, f in counts], [sl for sl, _ in counts], [u(T, 1) for T in Ts]


def test_give_up_is_a_transaction(gpu, knobs):
    """A give-up is not provoked: the status word is set behind a verify=False push_varlen.  verify() raises and commits nothing -- the
    fresh sessions are still fresh; the same tick pushed again runs on the grouped route (persistent launches are suspended) from
    the same generation and yields the bits of the packed route."""
    from pwv_amd._lib import PwvPersistError
    engine = knobs
    cfg = O.ModelConfig()
    model, _ = _model(gpu, cfg)
    first, z0, mels, slots, zs = _tick_inputs(cfg, gpu, 50)
    ref = model.open_stream(slots=4)
    ref.push(first, slots=[0, 1], z=z0)
    want = ref.push_varlen(mels, slots=slots, z=zs)
    s = model.open_stream(slots=4)
    s.push(first, slots=[0, 1], z=z0)
    gen, kept, running, hist = list(s._gen), s._kept.clone(), list(s._running), s._hist.clone()
    with _Log(engine) as lg:
        s.push_varlen(mels, slots=slots, z=zs, verify=False)
        _check_packed(lg.log, cfg, [80 + 960 + 400], gpu)
    with pytest.raises(_lib_error()):
        s.push_varlen(mels, slots=slots, z=zs)                   # _settled guards the call as it guards push
    torch.cuda.synchronize()
    engine.poke_persist_status(4)
    with pytest.raises(PwvPersistError):
        s.verify()
    assert s._gen == gen and s._running == running == [True, True, False, False] and torch.equal(s._kept, kept) and s._pending is None
    assert [s.emitted(i) for i in range(4)] == [800, 800, 0, 0]
    rd = [2 * sl + gen[sl] for sl in range(4)]
    assert torch.equal(s._hist[rd], hist[rd])                    # the generation the sessions stand on was not written
    assert engine.persist_suspended()
    with _Log(engine) as lg:
        got = s.push_varlen(mels, slots=slots, z=zs)
        assert [e[3] for e in lg.log if e[0] == 'stream_ragged'] == ['grouped'] * cfg.n_iaf
        assert 'suspended' in [e[4] for e in lg.log if e[0] == 'stream_ragged'][0]
        assert not [e for e in lg.log if e[0] == 'persist']
    engine.resume_persist()
    assert torch.equal(got.packed, want.packed) and [g.shape[0] for g in got] == [80, 960, 400, 0]
    assert s._running == [True] * 4 and [s.emitted(i) for i in range(4)] == [880, 1760, 400, 0]
    wr = [2 * sl + s._gen[sl] for sl in range(4)]
    assert torch.equal(s._hist[wr], ref._hist[[2 * sl + ref._gen[sl] for sl in range(4)]])


def _lib_error():
    from pwv_amd._lib import PwvError
    return PwvError


def test_a_give_up_inside_a_verified_push_is_rerun(gpu, knobs, monkeypatch):
    """The verified form: the status word raised behind the packed launch makes verified_call rerun the tick on the grouped route from
    the same generation; it warns, commits once, and the bits are the packed route's."""
    engine = knobs
    cfg = O.ModelConfig()
    model, _ = _model(gpu, cfg)
    first, z0, mels, slots, zs = _tick_inputs(cfg, gpu, 51)
    ref = model.open_stream(slots=4)
    ref.push(first, slots=[0, 1], z=z0)
    want = ref.push_varlen(mels, slots=slots, z=zs)
    s = model.open_stream(slots=4)
    s.push(first, slots=[0, 1], z=z0)
    real, poked = engine._run_stack_persist, []

    def spy(*a, **k):
        r = real(*a, **k)
        if not poked:
            poked.append(1)
            engine.poke_persist_status(4)
        return r
    monkeypatch.setattr(engine, '_run_stack_persist', spy)
    with _Log(engine) as lg:
        with pytest.warns(UserWarning, match='per-layer launches'):
            got = s.push_varlen(mels, slots=slots, z=zs)
        routes = [e[3] for e in lg.log if e[0] == 'stream_ragged']
        assert routes == ['packed'] * cfg.n_iaf + ['grouped'] * cfg.n_iaf, routes
        assert [e[0] for e in lg.log[-1:]] == ['layer_stream']
    assert poked and s._gen == [0, 0, 1, 1] and [s.emitted(i) for i in range(4)] == [880, 1760, 400, 0]
    assert torch.equal(got.packed, want.packed)


def test_range_rerun_takes_the_fp32_ragged_launch(gpu, knobs):
    """A tick that trips the range guard of the split-fp16 arithmetic is rerun in exact fp32 from the same state on the same noise: the
    hook shows the split-fp16 packed streaming launches and then the fp32 ones (both arithmetics have the ragged kernel); the result is
    the fp32 stream's from the same state, and the sessions go on from it."""
    from pwv_amd import _lib
    from pwv_amd.models import IAFVocoder
    engine = knobs
    cfg = _small()
    model, _ = _model(gpu, cfg)
    m32 = IAFVocoder(batch_size=1, length=80, store=model.store, precision='f32')
    ins = [_inputs(cfg, L, gpu, seed=60 + i) for i, L in enumerate((720, 1200))]
    hot = ins[0][2].clone()
    hot[4:6] *= 1e5
    s = model.open_stream(slots=2)
    first = s.push_varlen([hot[:4], ins[1][2][:9]], z=[ins[0][3][:240], ins[1][3][:640]])
    assert torch.equal(first[0], _one_shot(model, hot[:4], ins[0][3][:240]))
    before = [s.state(0), s.state(1)]
    tick = ([hot[4:7], ins[1][2][9:10]], [ins[0][3][240:480], ins[1][3][640:720]])
    with _Log(engine) as lg, _Hook(engine) as hk:
        with pytest.warns(UserWarning, match='rerun in exact fp32'):
            tripped = s.push_varlen(tick[0], z=tick[1])
        _check_packed(lg.log, cfg, [320, 320], gpu)
    n = cfg.n_iaf
    assert hk.seen == [(_lib.PREC_F16X3, True, True, True, True)] * n + [(_lib.PREC_F32, True, True, True, True)] * n, hk.seen
    assert [s.emitted(0), s.emitted(1)] == [480, 720] and bool(torch.isfinite(tripped.packed).all())
    s32 = m32.open_stream(slots=2)
    for i in range(2):
        s32.load_state(i, before[i])
    want = s32.push_varlen(tick[0], z=tick[1])
    assert torch.equal(tripped.packed, want.packed)
    after = s.push_varlen([hot[7:], ins[1][2][10:]], z=[ins[0][3][480:], ins[1][3][720:]])
    s2 = model.open_stream(slots=2)
    for i in range(2):
        s2.load_state(i, s32.state(i))
    want2 = s2.push_varlen([hot[7:], ins[1][2][10:]], z=[ins[0][3][480:], ins[1][3][720:]])
    assert torch.equal(after.packed, want2.packed) and [s.emitted(0), s.emitted(1)] == [720, 1200]


def test_push_and_push_varlen_alternate(gpu, knobs):
    """A session advanced by push and push_varlen alternately equals its one-shot forward."""
    cfg = O.ModelConfig()
    model, _ = _model(gpu, cfg)
    L = 4000
    ins = [_inputs(cfg, L, gpu, seed=70 + i) for i in range(2)]
    s = model.open_stream(slots=2)
    m = [ins[i][2] for i in range(2)]
    z = [ins[i][3] for i in range(2)]
    o = [[], []]
    g = s.push_varlen([m[0][:6], m[1][:11]], z=[z[0][:400], z[1][:800]])                   # fresh: 400 | 800
    o[0].append(g[0]), o[1].append(g[1])
    g = s.push(m[0][None, 6:11], slots=[0], z=z[0][None, 400:800])                          # uniform: slot 0 catches up
    o[0].append(g[0])
    g = s.push(torch.stack([m[0][11:21], m[1][11:21]]), z=torch.stack([z[0][800:1600], z[1][800:1600]]))
    o[0].append(g[0]), o[1].append(g[1])
    g = s.push_varlen([m[1][21:22], m[0][21:51]], slots=[1, 0], z=[z[1][1600:1680], z[0][1600:]])
    o[1].append(g[0]), o[0].append(g[1])
    g = s.push(m[1][None, 22:], slots=[1], z=z[1][None, 1680:])
    o[1].append(g[0])
    for i in range(2):
        assert s.emitted(i) == L and torch.equal(torch.cat(o[i]), _one_shot(model, m[i], z[i]))


def test_a_ragged_push_enqueues_one_more_call_than_a_uniform_one(gpu, knobs):
    """Counted at the C boundary as test_a_default_model_push_enqueues_few_launches does: a ragged push of the default model makes at
    most the library calls of a uniform push of the same rows plus one (pwv_varlen_unit_map) -- one pwv_wavenet_stack_persist_f32 per
    flow, one carry at most, no per-layer streaming launch."""
    from pwv_amd import _lib
    cfg = O.ModelConfig()
    model, _ = _model(gpu, cfg)
    s = model.open_stream(slots=2)
    rng = np.random.default_rng(9)
    mel = torch.from_numpy(rng.uniform(-1, 1, (2, 23, cfg.n_mels)).astype(np.float32)).to(gpu)
    z = torch.from_numpy(rng.uniform(-1, 1, (2, 1760, 1)).astype(np.float32)).to(gpu)
    s.push(mel[:, :21], z=z[:, :1600])                          # (plans, packs and projects: not counted)
    s.push_varlen([mel[0, :2], mel[1, :3]], z=[z[0, :160], z[1, :240]])
    lib = _lib.lib()
    calls = []

    class Counting(object):
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if not callable(fn) or not name.startswith('pwv_'):
                return fn

            def wrapped(*a):
                calls.append(name)
                return fn(*a)
            return wrapped

    quiet = ('pwv_persist_workspace_bytes', 'pwv_persist_short_input', 'pwv_tile32_floats', 'pwv_last_error', 'pwv_version')
    real = _lib.lib
    try:
        _lib.lib = lambda: Counting()
        for fa, fb, carry in ((19, 21, 0), (1, 3, 1)):          # 1520 + 1680 rows against 2 x 1600; 80 + 240 against 2 x 160
            del calls[:]
            s.push(mel[:, :(fa + fb) // 2], z=z[:, :(fa + fb) // 2 * HOP])
            uniform = [c for c in calls if c not in quiet]
            del calls[:]
            s.push_varlen([mel[0, :fa], mel[1, :fb]], z=[z[0, :fa * HOP], z[1, :fb * HOP]])
            ragged = [c for c in calls if c not in quiet]
            assert len(ragged) <= len(uniform) + 1, (uniform, ragged)
            assert ragged.count('pwv_wavenet_stack_persist_f32') == cfg.n_iaf and ragged.count('pwv_varlen_unit_map') == 1, ragged
            assert ragged.count('pwv_stream_carry_f32') == carry == uniform.count('pwv_stream_carry_f32'), (uniform, ragged)
            assert 'pwv_wavenet_layer_stream_f32' not in ragged and 'pwv_iaf_front_f32' not in ragged, ragged
    finally:
        _lib.lib = real


def test_generate_cli_stream_pushes_once_per_tick(gpu, tmp_path, monkeypatch):
    """`generate default --stream=5` on .npy mels of 3, 21 and 9 frames writes the sample counts `--varlen` writes, in ceil(21 / 5) = 5
    calls of push_varlen and none of push.  (The CLI draws OS seeds: the bits are the contract tests' business.)"""
    from scipy.io import wavfile
    from pwv_amd.generate import _fire, generate
    from pwv_amd.hparam import hparam as hp
    from pwv_amd.stream import StreamingVocoder
    rng = np.random.default_rng(4)
    frames = [3, 21, 9]
    for i, f in enumerate(frames):
        np.save(str(tmp_path / ('m%d.npy' % i)), rng.uniform(-1, 1, (f, 80)).astype(np.float32))
    logdir = tmp_path / 'out'
    monkeypatch.setenv('PWV_LOGDIR', str(logdir))
    orig = type(hp).set_hparam_yaml

    def patched(self, case, *a, **k):          # what a user's hparams.yaml case would override
        r = orig(self, case, *a, **k)
        self.data_path = str(tmp_path / '*.npy')
        self.train.dataset_ratio, self.generate.batch_size = 0.0, 3
        self.model.n_iaf, self.model.dilations = 1, [[1, 2, 4, 8]]
        return r

    monkeypatch.setattr(type(hp), 'set_hparam_yaml', patched)
    counts = {'push': 0, 'push_varlen': 0}
    for name in counts:
        def wrap(self, *a, _real=getattr(StreamingVocoder, name), _name=name, **k):
            counts[_name] += 1
            return _real(self, *a, **k)
        monkeypatch.setattr(StreamingVocoder, name, wrap)
    pred = _fire(generate, ['default', '--stream=5'])
    assert counts == {'push': 0, 'push_varlen': 5}, counts
    assert [p.shape for p in pred] == [((f - 1) * 80, 1) for f in frames]
    for i, f in enumerate(frames):
        rate, data = wavfile.read(str(logdir / ('pred_%d.wav' % i)))
        assert data.shape == ((f - 1) * 80,)


def test_pack_time_demotion_is_the_same_on_every_route(gpu, knobs):
    """Weights whose PACK-TIME bound fails (NetPlan._range_analysis: ||skip||_1 of the last layer, the bound on the head's operand, passes
    65000; every value an ordinary finite fp32, and nothing behind the skip product saturates) send that flow -- and only it -- to the exact-fp32 kernels on every route: the one-shot forward, generate_varlen, uniform pushes
    and a ragged schedule (a fresh session next to running ones, 80-row chunks: units that span two sessions) give the same bits on the
    same mel and noise, every persistent launch of the demoted flow carries PREC_F32, and the warning is raised once for its pair of nets."""
    import warnings
    from pwv_amd import _lib
    from pwv_amd.variables import variable_scope
    from tests.test_gpu_stream import _Feeder
    engine = knobs
    cfg = _small()
    model, w = _model(gpu, cfg, 'f16x3')
    name = 'iaf_vocoder/iaf1/scalar/dilated_stack/layer%d/skip' % (len(cfg.dilations[1]) - 1)
    model.store.assign(name, w[name] * 2.0e4)              # ||skip||_1 >= 64 * 0.088 * 2e4 = 1.1e5 (glorot: mean |w| = 0.088); max |w| = 3.5e3
    with variable_scope('iaf_vocoder'):
        flows = model._flows(model.store, False, 'f16x3')
    ok = [[engine.get_plan(net, 'frames', _lib.PREC_F16X3).f16x3_ok for net in iaf.nets()] for iaf in flows]
    assert ok[0] == [True, True] and sorted(ok[1]) == [False, True], ok      # (flow 1's scaler alone fails; its pair is demoted with it)
    key = tuple(net.full_scope for net in flows[1].nets())
    engine._range_warned.discard(key)
    layers = [len(d) - 1 for d in cfg.dilations[:cfg.n_iaf]]      # layers per persistent launch (the tail rides in it): tells the flows apart
    assert layers[0] != layers[1]
    seen = []
    schedule = {0: [4, 1, 5], 1: [None, 9, 7], 2: [None, None, 6]}       # 720, 1200 and 400 samples; sessions 1 and 2 start beside running ones
    engine.PERSIST_ARGS_HOOK = lambda pa: seen.append((int(pa.n_layers), int(pa.precision)))
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter('always')
            s, fd, ins, rows = _run_schedule(model, cfg, gpu, schedule, 80)
            ragged, seen[:] = list(seen), []
            want = [_one_shot(model, ins[sl][2], ins[sl][3]) for sl in schedule]
            one_shot, seen[:] = list(seen), []
            packed = model.generate_varlen([ins[sl][2] for sl in schedule], z=[ins[sl][3] for sl in schedule])
            varlen, seen[:] = list(seen), []
            u = model.open_stream(slots=3)
            uf = _Feeder(u)
            for sl, chunks in ((0, [240, 80, 400]), (1, [640, 560]), (2, [400])):
                uf.start(sl, ins[sl][2], ins[sl][3])
                for T in chunks:
                    uf.adv([sl], T)
            uniform = list(seen)
    finally:
        engine.PERSIST_ARGS_HOOK = None
    assert rows == [240, 80 + 640, 400 + 560 + 400]
    for sl in schedule:
        for route, got in (('generate_varlen', packed[sl]), ('push', uf.result(sl)), ('push_varlen', fd.result(sl))):
            assert torch.equal(got, want[sl]), (route, sl, float((got - want[sl]).abs().max()))
    for route, launches in (('one-shot', one_shot), ('generate_varlen', varlen), ('push', uniform), ('push_varlen', ragged)):
        demoted = [p for n, p in launches if n == layers[1]]
        assert demoted and all(p == _lib.PREC_F32 for p in demoted), (route, launches)
        assert [p for n, p in launches if n == layers[0]] == [_lib.PREC_F16X3] * len(demoted), (route, launches)
    told = [str(c.message) for c in caught if 'exceed the range' in str(c.message)]
    assert len(told) == 1 and key[0] in told[0], told
