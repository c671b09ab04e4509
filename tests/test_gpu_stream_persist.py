"""GPU: a streaming push as ONE persistent launch per flow (pwv_persist_args.hist, stack_persist_kernel<F32, MODE, false, STREAM = true>;
engine.run_flow_stream).  The contract of push does not change -- same bits, same history rows, same transaction rule as the per-layer
streaming launches (tests/test_gpu_stream.py, which run on the new kernels by default) -- so every case here first shows, from
engine.EVENT_LOG, that the new kernel RAN: each flow of each push is one streaming persistent launch with layer 0 and the tail inside
it, no pwv_wavenet_layer_stream_f32 route, in the instantiation the plan's arithmetic predicts from the device's CU count."""
import numpy as np
import pytest
import torch

from oracle import iaf_oracle as O
from tests.test_gpu_stream import _Feeder, _inputs, _model, _one_shot, _small, _small_wide
from tests.util import persist_plan_restated

pytestmark = pytest.mark.gpu


@pytest.fixture()
def knobs():
    from pwv_amd import engine
    saved = (engine.PERSIST, engine.PERSIST_MAX_LAYERS, engine.EVENT_LOG)
    engine.resume_persist()
    try:
        yield engine
    finally:
        engine.PERSIST, engine.PERSIST_MAX_LAYERS, engine.EVENT_LOG = saved
        engine.clear_persist_status()
        engine.resume_persist()


def _short_expected(rows, dmax, gpu, G=2, min_units=4):
    """Whether the library takes the short-input instantiation for these rows on this device: tests/util.persist_plan_restated."""
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    return 1 if persist_plan_restated(cus, G, rows, dmax, min_units=min_units)['unit_mode'] == 2 else 0


class _Log:
    """EVENT_LOG of the pushes inside the block; check() = what every case asserts about the route."""

    def __init__(self, engine):
        self.engine = engine

    def __enter__(self):
        self.log = self.engine.EVENT_LOG = []
        return self

    def __exit__(self, *exc):
        self.engine.EVENT_LOG = None

    def check(self, cfg, pushes, gpu, runs_per_flow=None, stream=1):
        """`pushes`: rows (N * T) of every push, in order.  Each contributed one launch per flow (or per run of a flow cut into
        runs): 'persist' entries that stream ([8]), start at layer 0 folded ([5]) and end with the tail ([6]) -- nothing else."""
        flows = [list(d) for d in cfg.dilations[:cfg.n_iaf]]
        runs_per_flow = runs_per_flow or [1] * len(flows)
        assert not [e for e in self.log if e[0] != 'persist'], [e[0] for e in self.log]      # no 'layer_stream': no per-layer route
        assert len(self.log) == len(pushes) * sum(runs_per_flow), (len(self.log), len(pushes), runs_per_flow)
        k = 0
        for rows in pushes:
            for dil, nruns in zip(flows, runs_per_flow):
                es = self.log[k:k + nruns]
                k += nruns
                assert all(e[3] == 2 and e[8] == stream for e in es)
                assert es[0][5] == 1 and es[-1][6] == 1 and sum(e[4] for e in es) == len(dil) - 1      # layer 0 .. L-2 + the tail
                if nruns == 1:
                    assert es[0][7] == _short_expected(rows, max(dil), gpu), (rows, es[0][7])
        return [e[7] for e in self.log]


def _random_state(s, seed):
    """Random non-zero histories in BOTH generations (what the push must overwrite, and what it must leave alone)."""
    g = torch.Generator(device='cpu').manual_seed(seed)
    s._hist.copy_(torch.empty(s._hist.shape).uniform_(-1, 1, generator=g))


def _push_both_routes(engine, model, cfg, gpu, n_slots, slots, T, seed, log_check=True, runs_per_flow=None):
    """The same push from the same random state on the persistent route and with PERSIST = False: (outputs, whole history arrays)."""
    rng = np.random.default_rng(seed)
    n = len(slots)
    mel = torch.from_numpy(rng.uniform(-1, 1, (n, T // 80 + 1, cfg.n_mels)).astype(np.float32)).to(gpu)
    z = torch.from_numpy(np.clip(rng.logistic(0, 1, (n, T, 1)), -20, 20).astype(np.float32)).to(gpu)
    res = []
    for persist in (True, False):
        engine.PERSIST = persist
        s = model.open_stream(slots=n_slots)
        _random_state(s, seed)
        before = s._hist.clone()
        with _Log(engine) as lg:
            out = s.push(mel, slots=slots, z=z, verify=False)
            s.verify()
        if persist and log_check:
            lg.check(cfg, [n * T], gpu, runs_per_flow)
        elif not persist:
            assert [e[0] for e in lg.log] == ['layer_stream'] * cfg.n_iaf
        # the generation the push read is untouched, as are the slots that were not pushed
        rd = [2 * sl + 0 for sl in slots]
        assert torch.equal(s._hist[rd], before[rd])
        idle = [b for sl in range(n_slots) if sl not in slots for b in (2 * sl, 2 * sl + 1)]
        assert torch.equal(s._hist[idle], before[idle])
        res.append((out.clone(), s._hist.clone()))
    return res


_SHAPES = [(1, [0], 80), (1, [0], 160), (3, [0, 1, 2], 560), (1, [0], 7200), (32, None, 800), (8, None, 4000), (32, None, 1600),
           (8, [5, 2, 7, 0], 2400)]


@pytest.mark.parametrize('shape', _SHAPES, ids=['1x80', '1x160', '3x560', '1x7200', '32x800', '8x4000', '32x1600', 'subset_permuted'])
@pytest.mark.parametrize('precision', ['f16x3', 'f32'])
def test_kernel_against_kernel_default_model(gpu, knobs, precision, shape):
    """Default model, random non-zero histories: the persistent streaming launches and the per-layer streaming launches give
    torch.equal outputs AND torch.equal history arrays (every byte of the written generation)."""
    n_slots, slots, T = shape
    slots = list(range(n_slots)) if slots is None else slots
    cfg = O.ModelConfig()
    model, _ = _model(gpu, cfg, precision)
    (out_p, hist_p), (out_l, hist_l) = _push_both_routes(knobs, model, cfg, gpu, n_slots, slots, T, seed=100 + T)
    assert torch.equal(out_p, out_l), float((out_p - out_l).abs().max())
    assert torch.equal(hist_p, hist_l), int((hist_p != hist_l).sum())
    assert bool(torch.isfinite(out_p).all())


@pytest.mark.parametrize('config', [_small, _small_wide], ids=['small', 'small_wide'])
@pytest.mark.parametrize('precision', ['f16x3', 'f32'])
@pytest.mark.parametrize('shape', [(1, 80), (3, 560), (2, 2400)], ids=['1x80', '3x560', '2x2400'])
def test_kernel_against_kernel_small_models(gpu, knobs, precision, config, shape):
    """The small models of test_gpu_stream.py: _small_wide has dilations 200 and 3, no multiples of 32, a flow whose last dilation
    (160, the tail's look-back) is not its largest and one whose last dilation (256) is."""
    n, T = shape
    cfg = config()
    model, _ = _model(gpu, cfg, precision)
    (out_p, hist_p), (out_l, hist_l) = _push_both_routes(knobs, model, cfg, gpu, n, list(range(n)), T, seed=7 + T)
    assert torch.equal(out_p, out_l), float((out_p - out_l).abs().max())
    assert torch.equal(hist_p, hist_l), int((hist_p != hist_l).sum())


@pytest.mark.parametrize('precision', ['f16x3', 'f32'])
def test_kernel_against_kernel_flows_cut_into_runs(gpu, knobs, precision):
    """PERSIST_MAX_LAYERS = 4: the default model's flows are cut into several persistent runs; every run's layers find their own
    history offsets, the first run the scalar history, the last run the tail's."""
    cfg = O.ModelConfig()
    knobs.PERSIST_MAX_LAYERS = 4
    runs = [len(knobs._persist_runs(len(d), 0)) for d in cfg.dilations[:cfg.n_iaf]]
    assert max(runs) >= 3
    model, _ = _model(gpu, cfg, precision)
    for n, T in ((2, 400), (4, 1600)):
        (out_p, hist_p), (out_l, hist_l) = _push_both_routes(knobs, model, cfg, gpu, n, list(range(n)), T, seed=3, runs_per_flow=runs)
        assert torch.equal(out_p, out_l) and torch.equal(hist_p, hist_l)


@pytest.mark.parametrize('precision', ['f16x3', 'f32'])
def test_contract_on_the_general_instantiation(gpu, knobs, precision):
    """Default model, 8 sessions of L = 24000 in pushes of 4000 (32000 rows per push: the general instantiation with many workgroups);
    session 3 is advanced alone in between (1 x 4000: the short-input instantiation), so the instantiations mix along its life.
    Every session equals its own IAFVocoder(1, L) one-shot forward."""
    cfg = O.ModelConfig()
    L, T, S = 24000, 4000, 8
    model, _ = _model(gpu, cfg, precision)
    ins = [_inputs(cfg, L, gpu, seed=60 + i) for i in range(S)]
    s = model.open_stream(slots=S)
    fd = _Feeder(s)
    for i in range(S):
        fd.start(i, ins[i][2], ins[i][3])
    others = [i for i in range(S) if i != 3]
    with _Log(knobs) as lg:
        fd.adv(list(range(S)), T)
        fd.adv(list(range(S)), T)
        fd.adv([3], T)                      # session 3 runs ahead ...
        fd.adv(list(range(S)), T)
        fd.adv(list(range(S)), T)
        fd.adv(list(range(S)), T)
        fd.adv(others, T)                   # ... and the others catch up
        kinds = lg.check(cfg, [S * T, S * T, T, S * T, S * T, S * T, (S - 1) * T], gpu)
    assert 0 in kinds and 1 in kinds, kinds            # both instantiations ran
    assert _short_expected(S * T, 512, gpu) == 0 and _short_expected(T, 512, gpu) == 1
    for i in range(S):
        assert s.emitted(i) == L
        want = _one_shot(model, ins[i][2], ins[i][3])
        assert torch.equal(fd.result(i), want), (i, float((fd.result(i) - want).abs().max()))


@pytest.mark.parametrize('precision', ['f16x3', 'f32'])
def test_generations_and_carry(gpu, knobs, precision):
    """A schedule that alternates T below and above the largest dilation (the carry launch runs, then not): the persistent route
    ends in the same history blocks, byte for byte, as the same schedule with PERSIST = False -- and in the one-shot bits."""
    cfg = O.ModelConfig()
    schedule = [80, 2400, 160, 4000, 80, 800, 400, 1600]
    L = sum(schedule)
    model, _ = _model(gpu, cfg, precision)
    ins = [_inputs(cfg, L, gpu, seed=70 + i) for i in range(2)]
    end = []
    for persist in (True, False):
        knobs.PERSIST = persist
        s = model.open_stream(slots=2)
        fd = _Feeder(s)
        fd.start(0, ins[0][2], ins[0][3]), fd.start(1, ins[1][2], ins[1][3])
        with _Log(knobs) as lg:
            for T in schedule:
                fd.adv([0, 1], T)
            if persist:
                lg.check(cfg, [2 * T for T in schedule], gpu)
            else:
                assert {e[0] for e in lg.log} == {'layer_stream'}
        assert s._gen == [len(schedule) % 2] * 2
        end.append((s._hist.clone(), fd.result(0), fd.result(1)))
    assert torch.equal(end[0][0], end[1][0]), int((end[0][0] != end[1][0]).sum())
    for i in range(2):
        assert torch.equal(end[0][1 + i], end[1][1 + i])
        assert torch.equal(end[0][1 + i], _one_shot(model, ins[i][2], ins[i][3]))


@pytest.mark.parametrize('precision', ['f16x3', 'f32'])
def test_guard_bands_on_the_persistent_route(gpu, knobs, precision):
    """As test_gpu_stream.py::test_guard_bands_around_the_histories: the histories inside a NaN-filled buffer; after pushes on the
    persistent route, 32 x 1600 (the general instantiation) included, the bands are untouched and no NaN came in."""
    cfg = O.ModelConfig()
    model, _ = _model(gpu, cfg, precision)
    guard, keep = 1 << 16, []

    def alloc(floats):
        buf = torch.full((floats + 2 * guard,), float('nan'), device=gpu)
        buf[guard:guard + floats].zero_()
        keep.append((buf, floats))
        return buf[guard:guard + floats]

    S = 33                                   # slot 32 is never pushed
    s = model.open_stream(slots=S, hist_alloc=alloc)
    rng = np.random.default_rng(5)
    pushes = []
    with _Log(knobs) as lg:
        for slots, T in ((list(range(32)), 1600), ([0, 31], 80), (list(range(32)), 1600), ([31, 5, 0], 560), ([7], 4000)):
            f = T // 80 + (0 if s._running[slots[0]] else 1)
            mel = torch.from_numpy(rng.uniform(-1, 1, (len(slots), f, cfg.n_mels)).astype(np.float32)).to(gpu)
            z = torch.from_numpy(np.clip(rng.logistic(0, 1, (len(slots), T, 1)), -20, 20).astype(np.float32)).to(gpu)
            out = s.push(mel, slots=slots, z=z)
            assert bool(torch.isfinite(out).all())
            pushes.append(len(slots) * T)
        lg.check(cfg, pushes, gpu)
    torch.cuda.synchronize()
    buf, floats = keep[0]
    assert bool(torch.isnan(buf[:guard]).all()) and bool(torch.isnan(buf[guard + floats:]).all())
    blocks = buf[guard:guard + floats].view(2 * S, -1)
    assert not bool(torch.isnan(blocks).any()) and not bool(blocks[64:66].any())


def test_give_up_is_a_transaction(gpu, knobs):
    """A give-up is not provoked: the thread's persist status word is set after a verify=False push, as a launch that gave up would
    leave it.  verify() raises PwvPersistError and commits nothing; the chunk pushed again runs on per-layer launches (the persistent
    ones are suspended) from the same generation and yields the one-shot bits."""
    from pwv_amd._lib import PwvPersistError
    engine = knobs
    cfg = O.ModelConfig()
    L = 4800
    model, _ = _model(gpu, cfg)
    _, _, mel_t, z_t = _inputs(cfg, L, gpu, seed=80)
    s = model.open_stream(slots=1)
    with _Log(engine) as lg:
        first = s.push(mel_t[None, :21], z=z_t[None, :1600])
        lg.check(cfg, [1600], gpu)
    gen, kept, hist = list(s._gen), s._kept.clone(), s._hist[s._gen[0]].clone()
    with _Log(engine) as lg:
        s.push(mel_t[None, 21:41], z=z_t[None, 1600:3200], verify=False)
        lg.check(cfg, [1600], gpu)
    torch.cuda.synchronize()
    engine.poke_persist_status(4)
    with pytest.raises(PwvPersistError):
        s.verify()
    assert s.emitted(0) == 1600 and s._gen == gen and torch.equal(s._kept, kept) and s._pending is None
    assert torch.equal(s._hist[s._gen[0]], hist)              # the generation the sessions stand on was not written
    assert engine.persist_suspended()
    with _Log(engine) as lg:
        second = s.push(mel_t[None, 21:41], z=z_t[None, 1600:3200])
        assert [e[0] for e in lg.log] == ['layer_stream'] * cfg.n_iaf      # suspended: the per-layer streaming launches
    engine.resume_persist()
    with _Log(engine) as lg:
        third = s.push(mel_t[None, 41:], z=z_t[None, 3200:])
        lg.check(cfg, [1600], gpu)
    want = _one_shot(model, mel_t, z_t)
    assert torch.equal(torch.cat([first[0], second[0], third[0]]), want)


def test_a_give_up_inside_a_verified_push_is_rerun(gpu, knobs, monkeypatch):
    """The verified form: the status word raised behind the persistent launches of a push (as test_safe_call.py does for a forward) makes
    verified_call rerun the push on the per-layer launches from the same generation; it warns, commits once, and the bits are the
    one-shot's."""
    engine = knobs
    cfg = O.ModelConfig()
    L = 3200
    model, _ = _model(gpu, cfg)
    _, _, mel_t, z_t = _inputs(cfg, L, gpu, seed=81)
    s = model.open_stream(slots=1)
    first = s.push(mel_t[None, :21], z=z_t[None, :1600])
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
            second = s.push(mel_t[None, 21:], z=z_t[None, 1600:])
        assert [e[0] for e in lg.log] == ['persist'] * cfg.n_iaf + ['layer_stream'] * cfg.n_iaf
    assert poked and s.emitted(0) == L and s._gen == [0]
    assert torch.equal(torch.cat([first[0], second[0]]), _one_shot(model, mel_t, z_t))


def test_range_rerun_takes_the_fp32_streaming_launch(gpu, knobs):
    """As test_gpu_stream.py::test_range_rerun_is_transactional, on a model whose flows have L >= 4: the chunk that trips the range guard
    is rerun in exact fp32 from the same state; the event log shows the split-fp16 streaming persistent launches and then the fp32
    ones (both arithmetics have the STREAM instantiations: the fp32 escape was not taken)."""
    engine = knobs
    cfg = _small()
    model, _ = _model(gpu, cfg)
    from pwv_amd.models import IAFVocoder
    m32 = IAFVocoder(batch_size=1, length=80, store=model.store, precision='f32')
    L = 720
    _, _, mel_t, z_t = _inputs(cfg, L, gpu, seed=40)
    mel_t = mel_t.clone()
    mel_t[4:6] *= 1e5
    s = model.open_stream(slots=1)
    first = s.push(mel_t[None, :4], z=z_t[None, :240])
    assert torch.equal(first[0], _one_shot(model, mel_t[:4], z_t[:240]))
    before = s.state(0)
    precs = []
    engine.PERSIST_ARGS_HOOK = lambda pa: precs.append((int(pa.precision), bool(pa.hist)))
    try:
        with _Log(engine) as lg:
            with pytest.warns(UserWarning, match='rerun in exact fp32'):
                tripped = s.push(mel_t[None, 4:7], z=z_t[None, 240:480])
            lg.check(cfg, [240, 240], gpu)
    finally:
        engine.PERSIST_ARGS_HOOK = None
    from pwv_amd import _lib
    assert precs == [(_lib.PREC_F16X3, True)] * cfg.n_iaf + [(_lib.PREC_F32, True)] * cfg.n_iaf, precs
    assert s.emitted(0) == 480 and bool(torch.isfinite(tripped).all())
    s32 = m32.open_stream(slots=1)
    s32.load_state(0, before)
    want = s32.push(mel_t[None, 4:7], z=z_t[None, 240:480])
    assert torch.equal(tripped, want)
    after = s.push(mel_t[None, 7:], z=z_t[None, 480:])
    s2 = model.open_stream(slots=1)
    s2.load_state(0, s32.state(0))
    assert torch.equal(after, s2.push(mel_t[None, 7:], z=z_t[None, 480:])) and s.emitted(0) == L


def test_a_default_model_push_enqueues_few_launches(gpu, knobs):
    """What a push of the default model enqueues, counted at the C boundary: the prologue (at most 3 calls), the carry (0 or 1) and
    ONE pwv_wavenet_stack_persist_f32 per flow -- no pwv_wavenet_layer_stream_f32, no affine launch."""
    from pwv_amd import _lib
    cfg = O.ModelConfig()
    model, _ = _model(gpu, cfg)
    s = model.open_stream(slots=2)
    rng = np.random.default_rng(9)
    mel = torch.from_numpy(rng.uniform(-1, 1, (2, 21, cfg.n_mels)).astype(np.float32)).to(gpu)
    z = torch.from_numpy(rng.uniform(-1, 1, (2, 1600, 1)).astype(np.float32)).to(gpu)
    s.push(mel, z=z)                          # (plans, packs and projects: not counted)
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

    real = _lib.lib
    try:
        _lib.lib = lambda: Counting()
        for T in (1600, 80):
            del calls[:]
            s.push(mel[:, :T // 80], z=z[:, :T])
            launches = [c for c in calls if c not in ('pwv_persist_workspace_bytes', 'pwv_persist_short_input', 'pwv_tile32_floats', 'pwv_last_error',
                                                      'pwv_version')]
            assert launches.count('pwv_wavenet_stack_persist_f32') == cfg.n_iaf, launches
            assert 'pwv_wavenet_layer_stream_f32' not in launches and 'pwv_iaf_front_f32' not in launches, launches
            assert launches.count('pwv_stream_carry_f32') == (1 if T < 512 else 0), launches
            rest = [c for c in launches if c not in ('pwv_wavenet_stack_persist_f32', 'pwv_stream_carry_f32')]
            assert len(rest) <= 3, launches            # the prologue
    finally:
        _lib.lib = real
