"""-m gpu: every route of the package run twice from the same inputs -- first as every other test runs it, then inside poisoned,
guard-banded device buffers (tests/guarded.py: every `torch.empty` / `zeros` of the package lies in a larger 0xFF buffer; a float
`empty` starts as NaN).  The bit-identity tests elsewhere run a route several times on the same shapes, and the caching allocator
hands the same blocks back: a store that never lands leaves the previous run's correct value in place and passes torch.equal.  Here
it leaves a NaN, and a store that lands next to its buffer leaves a mark in a band.

For every route the helper asserts, after a synchronise: (a) the guarded result is torch.equal to the ordinary one (and holds no NaN);
(b) no band of any guarded allocation was touched; (c) no persistent launch gave up and no range flag was raised (verify=False +
verify(), as tests/util.run_vocoder_hip: no repair route ran instead of the one asked for); (d) engine.EVENT_LOG shows the launch kind
-- and the persistent instantiation, entry [7] -- that was asked for; (e) for the one-shot cases max|y - y_fp64| <= TOL_F32 against
oracle/iaf_oracle.py (precision 'f16': the bars of tests/test_gpu_f16.py).

Shapes (the conditions matter, the numbers may move): total rows no multiple of 32, utterance / session boundaries in the middle of a
unit, at least two workgroups with the look-back crossing between them wherever an instantiation is asked for.
  M2 = hop_cfg(80), two flows of 4 and 6 layers, n = 3, T = 240: 720 rows = 22.5 units, boundaries at row 16 of units 7 and 15.
       PERSIST_MIN_UNITS 0: 6 workgroups of 4 units, the short-input instantiation; 16: 2 of 12, the general one; 32: one workgroup.
  D7 = one flow over DIL7, n = 1, T = 2000: 62.5 units, d = 512 reaches 16 units back.  PERSIST_MAX_LAYERS = 4 cuts the stack into
       runs that hand the ring on (every rotation); PERSIST_MIN_UNITS 16: 4 workgroups of 16 units, general; 0: 16 of 4, short-input."""
import functools

import numpy as np
import pytest
import torch

from oracle import iaf_oracle as O
from tests.guarded import guarded
from tests.test_gpu_f16 import TOL_F16, TOL_F16_RMS
from tests.util import DIL7, TOL_F32, hop_cfg, set_hparams, small_cfg

pytestmark = pytest.mark.gpu

COUNTS = {}      # route -> guarded allocations of its run (printed: the proxy really was in the path)


def _mods():
    from pwv_amd import engine, graph, modules, stream
    return engine, stream, graph, modules


@pytest.fixture()
def knobs(monkeypatch):
    """engine, with every knob a case may set restored afterwards and the sticky words left clean."""
    from pwv_amd import engine
    for name in ('PERSIST', 'PERSIST_MIN_UNITS', 'PERSIST_MAX_LAYERS', 'TWO_STREAMS', 'FUSE_TAIL', 'FOLD_FIRST', 'FUSE_PROLOGUE',
                 'EVENT_LOG', 'PERSIST_ARGS_HOOK', 'VARLEN_PADDED'):
        monkeypatch.setattr(engine, name, getattr(engine, name))
    engine.resume_persist()
    engine.PERSIST = True          # forced, whatever the size (a case that wants per-layer launches says so)
    yield engine
    torch.cuda.synchronize()
    engine.clear_persist_status()
    engine.clear_range_flag()
    engine.resume_persist()


class _Run(object):
    def __init__(self, outs, log, result_guarded=True, extra=None):
        self.outs, self.log, self.result_guarded, self.extra = list(outs), log, result_guarded, extra


def _settled(engine, verify):
    """(c): after a synchronise neither sticky word is raised; then the caller's own verify()."""
    torch.cuda.synchronize()
    assert engine.persist_status() == 0, 'a persistent launch gave up'
    assert not engine.range_flag_raised(), 'a range flag was raised'
    verify()


def _pair(name, run, expect_log, shapes=()):
    """`run()` builds its store and model and runs the route under an EVENT_LOG: once as it is, then guarded.  Returns (ordinary, guarded,
    the Guard).  `shapes`: allocation shapes the registry has to hold (the ring, ...)."""
    want = run()
    expect_log(want.log)
    with guarded(*_mods()) as g:
        got = run()
        torch.cuda.synchronize()
        assert len(got.outs) == len(want.outs)
        for k, (a, b) in enumerate(zip(want.outs, got.outs)):
            assert a.shape == b.shape and a.dtype == b.dtype
            if b.is_floating_point():
                assert not bool(torch.isnan(b).any()), (name, k, 'NaN left in the guarded result', int(torch.isnan(b).sum()))
            assert torch.equal(a, b), (name, k, 'guarded and ordinary run differ', int((a != b).sum()))      # (a)
        g.check()                                                                                                # (b)
        expect_log(got.log)                                                                                      # (d)
        assert g.allocations, 'nothing was allocated through the proxy'
        if got.result_guarded:
            assert g.holds(got.outs[0]), 'the result does not lie in a guarded allocation'
        have = [a.shape for a in g.allocations]
        for s in shapes:
            assert s in have, (name, s, 'not among the guarded allocations')
        COUNTS[name] = len(g.allocations)
        print('guarded[%s]: %d allocations, %d call sites' % (name, len(g.allocations), len(g.sites())))
    return want, got, g


# ---- the cases' inputs and fp64 references: made once, shared, never written to --------------------------------------------------
M2_N, M2_T = 3, 240
D7_N, D7_T = 1, 2000
NOISE_SEED = 1234


@functools.lru_cache(maxsize=None)
def _case(kind):
    """(cfg, weights, mel, z, y_fp64) of a one-shot case."""
    if kind == 'd7':
        cfg, n, t = small_cfg(dilations=[DIL7], n_iaf=1), D7_N, D7_T
    else:
        kw = {'m2': {}, 'shared': dict(shared_nets=True), 'transposed': dict(cond_upsample_method='transposed_conv'),
              'skip': dict(use_skip_connection=True), 'in': dict(normalize='in'), 'bn': dict(normalize='bn')}[kind]
        cfg, n, t = hop_cfg(80, **kw), M2_N, M2_T
    w = O.init_weights(cfg, seed=2)
    mel, z = O.synthetic_inputs(n, t, cfg)
    y = O.iaf_vocoder_forward(w, mel, z, cfg)
    for a in (mel, z, y):
        a.setflags(write=False)
    return cfg, w, mel, z, y


def _tile32_floats(rows, channels=64):
    return (rows + 31) // 32 * 32 * channels


def _one_shot(engine, gpu, kind, precision, z=True):
    """run() of a one-shot forward of _case(kind); z = False: the model draws its own noise from NOISE_SEED."""
    from pwv_amd.models import IAFVocoder
    from pwv_amd.variables import VariableStore
    cfg, w, mel, zz, _ = _case(kind)
    mel_t = torch.from_numpy(np.array(mel)).to(gpu)
    z_t = torch.from_numpy(np.array(zz)).to(gpu) if z else None

    def run():
        set_hparams(cfg)
        store = VariableStore(device=gpu)
        store.load_dict(w)
        model = IAFVocoder(batch_size=mel.shape[0], length=zz.shape[1], store=store, precision=precision)
        model.noise_seed, model.noise_offset = NOISE_SEED, 0
        log = engine.EVENT_LOG = []
        try:
            out = model(None, mel_t, is_training=False, z=z_t, verify=False)
            _settled(engine, model.verify)
        finally:
            engine.EVENT_LOG = None
        return _Run([out], log)
    return run


def _expect_persist(cfg, short, tail=1, G=2, stream=0, runs_per_flow=None, launches=1):
    """(d) for persistent routes: per forward and flow `runs` 'persist' entries over all nets, layer 0 inside the first ([5]), the tail
    inside the last ([6] == tail), together the flow's layers, every one the instantiation asked for ([7]), [8] = streaming."""
    flows = [list(d) for d in cfg.dilations[:cfg.n_iaf]]
    runs_per_flow = runs_per_flow or [1] * len(flows)

    def expect(log):
        assert [e[0] for e in log] == ['persist'] * (launches * sum(runs_per_flow)), [e[0] for e in log]
        k = 0
        for _ in range(launches):
            for dil, nruns in zip(flows, runs_per_flow):
                es = log[k:k + nruns]
                k += nruns
                assert all(e[3] == G and e[7] == short and e[8] == stream for e in es), [(e[3], e[7], e[8]) for e in es]
                assert es[0][5] == 1 and es[-1][6] == tail and all(e[6] == 0 for e in es[:-1])
                assert sum(e[4] for e in es) == len(dil) - 1
    return expect


def _expect_per_layer(cfg, two_streams):
    def expect(log):
        per_flow = 2 if two_streams else 1
        assert [e[0] for e in log] == ['layer_residual'] * (per_flow * cfg.n_iaf), [e[0] for e in log]
        k = 0
        for dil in cfg.dilations[:cfg.n_iaf]:
            for e in log[k:k + per_flow]:
                assert e[3] == (1 if two_streams else 2) and e[4] == len(dil) - 1
            k += per_flow
    return expect


def _oracle_bar(got, kind, precision='f16x3', want=None):
    """(e)"""
    y = _case(kind)[4] if want is None else want
    d = got.outs[0].cpu().numpy().astype(np.float64) - y
    err = float(np.abs(d).max())
    print('max|y - y_fp64| [%s, %s] = %.3g' % (kind, precision, err))
    if precision == 'f16':
        assert err <= TOL_F16 and float(np.sqrt((d ** 2).mean())) <= TOL_F16_RMS, err
    else:
        assert err <= TOL_F32, err


# ---- one-shot, M2 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('min_units,short', [(0, 1), (16, 0), (32, 0)], ids=['6wg_short', '2wg_general', '1wg_general'])
@pytest.mark.parametrize('precision', ['f16x3', 'f32'])
def test_one_shot_persistent(gpu, knobs, precision, min_units, short):
    engine = knobs
    engine.PERSIST_MIN_UNITS = min_units
    cfg = _case('m2')[0]
    name = 'one_shot/%s/min_units=%d' % (precision, min_units)
    _, got, _ = _pair(name, _one_shot(engine, gpu, 'm2', precision), _expect_persist(cfg, short),
                      shapes=[(3, _tile32_floats(M2_N * M2_T)), (M2_N, M2_T, 1)])
    _oracle_bar(got, 'm2', precision)


_VARIANTS = ['per_layer_two_streams', 'per_layer_one_stream', 'no_fused_tail', 'unfolded_first', 'separate_prologue', 'f16', 'shared_nets',
             'transposed_conv', 'skip_connection', 'normalize_in', 'normalize_bn', 'own_noise']


@pytest.mark.parametrize('variant', _VARIANTS)
def test_one_shot_variants(gpu, knobs, variant):
    """M2 on every other one-shot route: per-layer launches on two streams and on one, the tail / the folded layer 0 / the one-launch
    prologue switched off, the fp16 storage mode, one shared net per flow, per-sample conditioning, skip accumulation, the two
    normalisers behind a flow, and the model drawing its own noise."""
    engine = knobs
    kind, precision, z = 'm2', 'f16x3', True
    cfg = _case('m2')[0]
    expect = _expect_persist(cfg, 1)
    ring = (3, _tile32_floats(M2_N * M2_T))
    pair_buf = (_tile32_floats(M2_N * M2_T),)
    shapes = [ring]
    if variant in ('per_layer_two_streams', 'per_layer_one_stream'):
        engine.PERSIST, engine.TWO_STREAMS = False, variant == 'per_layer_two_streams'
        expect, shapes = _expect_per_layer(cfg, engine.TWO_STREAMS), [pair_buf]
    elif variant == 'no_fused_tail':
        engine.FUSE_TAIL = False
        expect = _expect_persist(cfg, 1, tail=0)
    elif variant == 'unfolded_first':       # (the short-input instantiation has layer 0 in its folded form only: the general one runs)
        engine.FOLD_FIRST = False
        expect = _expect_persist(cfg, 0)
    elif variant == 'separate_prologue':
        engine.FUSE_PROLOGUE = False
    elif variant == 'f16':                  # (the fp16 storage mode has per-layer launches only)
        precision, expect, shapes = 'f16', _expect_per_layer(cfg, engine.TWO_STREAMS), [pair_buf]
    elif variant == 'shared_nets':
        kind = 'shared'
        expect, shapes = _expect_persist(_case(kind)[0], 1, G=1), [ring, (M2_N, M2_T, 2)]
    elif variant == 'transposed_conv':      # per-sample conditioning: the condition GEMM inside the per-layer kernels
        kind = 'transposed'
        expect, shapes = _expect_per_layer(_case(kind)[0], engine.TWO_STREAMS), [pair_buf, (2 * _tile32_floats(M2_N * M2_T, 80),)]
    elif variant == 'skip_connection':      # skip sums: per-layer launches
        kind = 'skip'
        expect, shapes = _expect_per_layer(_case(kind)[0], engine.TWO_STREAMS), [pair_buf, (_tile32_floats(M2_N * M2_T, 128),)]
    elif variant in ('normalize_in', 'normalize_bn'):
        kind = variant[-2:]
        expect = _expect_persist(_case(kind)[0], 1)
    elif variant == 'own_noise':
        z = False
    _, got, _ = _pair('one_shot/' + variant, _one_shot(engine, gpu, kind, precision, z=z), expect, shapes=shapes)
    if variant == 'own_noise':          # the reference on the noise the sampler drew (the sampler itself: tests/test_gpu_parity.py)
        cfg, w, mel, _, _ = _case('m2')
        drawn = engine.logistic_noise_op((M2_N, M2_T, 1), gpu, seed=NOISE_SEED, offset=0).cpu().numpy()
        _oracle_bar(got, kind, precision, want=O.iaf_vocoder_forward(w, mel, drawn, cfg))
    else:
        _oracle_bar(got, kind, precision)


# ---- one-shot, D7 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('max_layers,runs', [(4, 2), (32, 1)], ids=['runs_of_3', 'one_run'])
@pytest.mark.parametrize('min_units,short', [(16, 0), (0, 1)], ids=['general', 'short'])
@pytest.mark.parametrize('precision', ['f16x3', 'f32'])
def test_one_shot_long_look_back(gpu, knobs, precision, min_units, short, max_layers, runs):
    engine = knobs
    engine.PERSIST_MIN_UNITS, engine.PERSIST_MAX_LAYERS = min_units, max_layers
    cfg = _case('d7')[0]
    assert [c for _, c in engine._persist_runs(len(DIL7), 0)] == ([3, 3] if runs == 2 else [6])
    name = 'd7/%s/min_units=%d/max_layers=%d' % (precision, min_units, max_layers)
    _, got, _ = _pair(name, _one_shot(engine, gpu, 'd7', precision), _expect_persist(cfg, short, runs_per_flow=[runs]),
                      shapes=[(3, _tile32_floats(D7_T)), (D7_N, D7_T, 1)])
    _oracle_bar(got, 'd7', precision)


# ---- packed ------------------------------------------------------------------------------------------------------------------------
PACKED_LENGTHS = [80, 480, 160, 800]       # 1520 rows = 47.5 units, every boundary in the middle of a unit
PACKED_SEEDS = [11, (1 << 63) + 5, 13, 14]


def _packed_mels(cfg, gpu, lengths=PACKED_LENGTHS):
    rng = np.random.default_rng(8)
    return [torch.from_numpy(rng.uniform(-1, 1, (L // cfg.hop_length + 1, cfg.n_mels)).astype(np.float32)).to(gpu) for L in lengths]


def _packed(engine, gpu, cfg, w, mels):
    from pwv_amd.models import IAFVocoder
    from pwv_amd.variables import VariableStore

    def run():
        set_hparams(cfg)
        store = VariableStore(device=gpu)
        store.load_dict(w)
        model = IAFVocoder(batch_size=1, length=80, store=store)
        padded = engine.VARLEN_PADDED
        log = engine.EVENT_LOG = []
        try:
            out = model.generate_varlen(mels, seeds=PACKED_SEEDS, verify=False)
            _settled(engine, model.verify)
        finally:
            engine.EVENT_LOG = None
        return _Run([out.packed], log, result_guarded=engine.VARLEN_PADDED == padded, extra=engine.VARLEN_PADDED - padded)
    return run


@pytest.mark.parametrize('route', ['short', 'general', 'padded'])
def test_packed(gpu, knobs, route):
    """generate_varlen with one noise stream per utterance: the packed persistent launches in both instantiations (12 workgroups of 4
    units; 3 of 16) and, with PERSIST off, the padded fallback."""
    engine = knobs
    cfg, w = _case('m2')[:2]
    rows = sum(PACKED_LENGTHS)
    if route == 'padded':
        engine.PERSIST = False
        expect = _expect_per_layer(cfg, engine.TWO_STREAMS)
        shapes = [(len(PACKED_LENGTHS) * max(PACKED_LENGTHS), 1), (rows, 1)]      # the padded batch (pad_rows), the packed noise
    else:
        engine.PERSIST_MIN_UNITS = 0 if route == 'short' else 16
        expect = _expect_persist(cfg, 1 if route == 'short' else 0)
        shapes = [(3, _tile32_floats(rows)), (rows, 1), (1, rows, 1)]             # ring, noise, the flows' outputs
    want, got, g = _pair('packed/' + route, _packed(engine, gpu, cfg, w, _packed_mels(cfg, gpu)), expect, shapes=shapes)
    assert want.extra == got.extra == (cfg.n_iaf if route == 'padded' else 0)
    if route != 'padded':
        assert any(a.dtype == torch.int32 and a.site.startswith('engine.py') for a in g.allocations)      # the unit map


# ---- streaming ---------------------------------------------------------------------------------------------------------------------
def _stream_inputs(cfg, gpu):
    rng = np.random.default_rng(21)
    return torch.from_numpy(rng.uniform(-1, 1, (3, 16, cfg.n_mels)).astype(np.float32)).to(gpu)      # frames of sessions 0, 1, 2


def _streaming(engine, gpu, cfg, w, frames):
    """Two pushes of 2 frames on slots [0, 2], then two ragged pushes with [1, 2, 4] frames on slots [0, 1, 2]: slot 1 fresh in the
    first (480 rows), all three running in the second (560 rows = 17.5 units); slot 3 is never pushed.  Every session draws its own
    noise.  After each push: the generation every pushed session READ is unchanged."""
    from pwv_amd.models import IAFVocoder
    from pwv_amd.variables import VariableStore

    def run():
        set_hparams(cfg)
        store = VariableStore(device=gpu)
        store.load_dict(w)
        model = IAFVocoder(batch_size=1, length=80, store=store)
        s = model.open_stream(slots=4)
        outs, pos = [], [0, 0, 0]
        log = engine.EVENT_LOG = []

        def advance(slots, counts, push):
            before, gen = s._hist.clone(), list(s._gen)
            mels = [frames[sl, pos[sl]:pos[sl] + f] for sl, f in zip(slots, counts)]
            fresh = [not s._running[sl] for sl in slots]
            seeds = [100 + sl if fr else None for sl, fr in zip(slots, fresh)]
            if push:
                out = s.push(torch.stack(mels), slots=slots, seeds=seeds if all(fresh) else None, verify=False)
                pieces = [out]
            else:
                out = s.push_varlen(mels, slots=slots, seeds=seeds, verify=False)
                pieces = [out.packed]
            _settled(engine, s.verify)
            read = [2 * sl + gen[sl] for sl in slots]
            assert torch.equal(s._hist[read], before[read]), 'a push wrote the generation it reads'
            assert [s._gen[sl] for sl in slots] == [1 - gen[sl] for sl in slots]
            for sl, f in zip(slots, counts):
                pos[sl] += f
            outs.extend(pieces)
        try:
            advance([0, 2], [2, 2], True)
            advance([0, 2], [2, 2], True)
            advance([0, 1, 2], [1, 2, 4], False)
            advance([0, 1, 2], [1, 2, 4], False)
        finally:
            engine.EVENT_LOG = None
        assert [tuple(o.shape) for o in outs] == [(2, 80, 1), (2, 160, 1), (480, 1), (560, 1)]
        assert not bool(s._hist[6:8].any()), 'the blocks of the slot that was never pushed are no longer zero'
        assert [s.emitted(k) for k in range(4)] == [400, 240, 880, 0]
        return _Run(outs + [s._hist, s._kept], log, extra=s)
    return run


@pytest.mark.parametrize('persist', [True, False], ids=['persistent', 'per_layer'])
def test_streaming(gpu, knobs, persist):
    engine = knobs
    engine.PERSIST = persist
    cfg, w = _case('m2')[:2]

    def expect(log):
        kinds = [e[0] for e in log]
        if persist:      # per flow one streaming persistent launch, layer 0 and the tail inside; the ragged pushes in their packed form
            assert kinds == ['persist'] * 4 + ['stream_ragged', 'persist'] * 4, kinds
            assert all(e[8] == 1 and e[5] == 1 and e[6] == 1 and e[3] == 2 for e in log if e[0] == 'persist')
            assert all(e[3] == 'packed' for e in log if e[0] == 'stream_ragged')
        else:            # L streaming layer launches per flow; the ragged pushes grouped by chunk length
            assert kinds[:4] == ['layer_stream'] * 4 and set(kinds[4:]) == {'stream_ragged', 'layer_stream'}, kinds
            assert all(e[3] == 'grouped' for e in log if e[0] == 'stream_ragged')
    _, got, g = _pair('streaming/' + ('persistent' if persist else 'per_layer'), _streaming(engine, gpu, cfg, w, _stream_inputs(cfg, gpu)), expect)
    s = got.extra
    assert g.holds(s._hist) and g.holds(s._kept) and g.holds(s._sess)


# ---- the graph wrappers ------------------------------------------------------------------------------------------------------------
def _model_in(gpu, cfg, w, n=1, length=80):
    from pwv_amd.models import IAFVocoder
    from pwv_amd.variables import VariableStore
    set_hparams(cfg)
    store = VariableStore(device=gpu)
    store.load_dict(w)
    return IAFVocoder(batch_size=n, length=length, store=store)


def test_graphed_vocoder(gpu, knobs):
    """GraphedVocoder constructed, captured and replayed three times inside the context (once on noise its captured sampler draws, twice
    on the caller's): the eager forward's bits, its static buffers and the sampler state among the banded allocations."""
    from pwv_amd.graph import GraphedVocoder
    engine = knobs
    cfg, w, mel, z, _ = _case('m2')
    mel_t, z_t = torch.from_numpy(np.array(mel)).to(gpu), torch.from_numpy(np.array(z)).to(gpu)
    eager_z = _one_shot(engine, gpu, 'm2', 'f16x3')().outs[0].clone()
    eager_own = _one_shot(engine, gpu, 'm2', 'f16x3', z=False)().outs[0].clone()
    with guarded(*_mods()) as g:
        model = _model_in(gpu, cfg, w, M2_N, M2_T)
        gv = GraphedVocoder(model)
        got = [gv(mel_t, seed=NOISE_SEED).clone(), gv(mel_t, z=z_t).clone(), gv(mel_t, z=z_t).clone()]
        _settled(engine, gv.verify)
        assert gv.captures == 1
        for a, b in zip([eager_own, eager_z, eager_z], got):
            assert not bool(torch.isnan(b).any()) and torch.equal(a, b), int((a != b).sum())
        g.check()
        assert all(g.holds(t) for t in (gv.mel, gv.z, gv.noise_state, gv.out))
        assert (3, _tile32_floats(M2_N * M2_T)) in [a.shape for a in g.allocations]
        COUNTS['graph/vocoder'] = len(g.allocations)
        print('guarded[graph/vocoder]: %d allocations' % len(g.allocations))


def test_graphed_packed_vocoder(gpu, knobs):
    from pwv_amd.graph import GraphedPackedVocoder
    engine = knobs
    cfg, w = _case('m2')[:2]
    mels = _packed_mels(cfg, gpu)
    eager = _packed(engine, gpu, cfg, w, mels)().outs[0].clone()
    rows = sum(PACKED_LENGTHS)
    with guarded(*_mods()) as g:
        model = _model_in(gpu, cfg, w)
        gp = GraphedPackedVocoder(model, slots=len(mels), rows=rows)
        got = []
        for _ in range(3):
            got.append(gp(mels, PACKED_SEEDS).packed.clone())
        _settled(engine, gp.verify)
        assert gp.captures == 1 and gp.eager_calls == 0
        for b in got:
            assert not bool(torch.isnan(b).any()) and torch.equal(eager, b), int((eager != b).sum())
        g.check()
        assert all(g.holds(t) for t in (gp.mel, gp.z, gp._tables, gp.cu_rows, gp.streams, gp._unit_map, gp.out))
        COUNTS['graph/packed'] = len(g.allocations)
        print('guarded[graph/packed]: %d allocations' % len(g.allocations))


def _ticks(engine, gpu, cfg, w, frames, ragged, graphed):
    """Sessions 0, 1, 2 of a 4-slot stream started with the eager one-frame push, then three ticks: uniform -- slots [0, 2], 2 frames each
    --, or ragged -- slots [0, 1, 2] with [1, 2, 4] frames (560 rows).  Every session draws its own noise.  (outputs, stream, graph)"""
    model = _model_in(gpu, cfg, w)
    s = model.open_stream(slots=4)
    slots, counts = ([0, 1, 2], [1, 2, 4]) if ragged else ([0, 2], [2, 2])
    s.push_varlen([frames[sl, :1] for sl in slots], slots=slots, seeds=[100 + sl for sl in slots])
    gr = None
    if graphed:
        gr = s.graphed_varlen(3, 560) if ragged else s.graphed(2, 2)
    outs, pos = [], 1
    for _ in range(3):
        mels = [frames[sl, pos * f:(pos + 1) * f] for sl, f in zip(slots, counts)]
        if ragged:
            out = gr.tick(mels, slots) if graphed else s.push_varlen(mels, slots=slots, verify=False)
            outs.append(out.packed.clone())
        else:
            out = gr.tick(torch.stack(mels), slots) if graphed else s.push(torch.stack(mels), slots=slots, verify=False)
            outs.append(out.clone())
        if not graphed:
            _settled(engine, s.verify)
        pos += 1
    if graphed:
        torch.cuda.synchronize()
        assert engine.persist_status() == 0 and not engine.range_flag_raised()
        assert gr.verify() == 3 and gr.captures == 1 and gr.eager_calls == 0
    return outs, s, gr


@pytest.mark.parametrize('ragged', [False, True], ids=['uniform', 'ragged'])
def test_graphed_stream_ticks(gpu, knobs, ragged):
    """s.graphed(n, frames) / s.graphed_varlen(slots, rows): three replays inside the context give the eager pushes' bits and the same
    histories; the session table, the commit's counters and the kept frames are banded allocations."""
    engine = knobs
    cfg, w = _case('m2')[:2]
    frames = _stream_inputs(cfg, gpu)
    want, s0, _ = _ticks(engine, gpu, cfg, w, frames, ragged, graphed=False)
    with guarded(*_mods()) as g:
        got, s, gr = _ticks(engine, gpu, cfg, w, frames, ragged, graphed=True)
        for a, b in zip(want, got):
            assert not bool(torch.isnan(b).any()) and torch.equal(a, b), int((a != b).sum())
        called = [0, 1, 2] if ragged else [0, 2]
        current = [2 * sl + s._gen[sl] for sl in called]
        assert list(s._gen) == list(s0._gen) and torch.equal(s._hist[current], s0._hist[current]) and torch.equal(s._kept, s0._kept)
        assert [s.emitted(k) for k in range(4)] == [s0.emitted(k) for k in range(4)]
        g.check()
        assert all(g.holds(t) for t in (s._sess, gr._counters, s._kept, s._hist, gr._entries, gr._tab, gr.mel, gr.z, gr.out))
        name = 'graph/' + ('ragged_ticks' if ragged else 'ticks')
        COUNTS[name] = len(g.allocations)
        print('guarded[%s]: %d allocations' % (name, len(g.allocations)))


# ---- the harness itself: the only deliberate misdirection, inside memory the test owns --------------------------------------------------
@pytest.mark.parametrize('which', ['tail_out_forward', 'affine_out_back'])
def test_a_misplaced_store_is_named(gpu, knobs, monkeypatch, which):
    """M2 / f16x3 / short-input, the last flow's launch handed a pointer 16 bytes off through engine.PERSIST_ARGS_HOOK: tail_out[0] (the
    scalar net's output) 16 bytes forward, or affine_out (the flow's result) 16 bytes back.  check() names that allocation, on that side,
    within 16 bytes of the payload, and the buffer differs from the ordinary run's.  The moved pointer stays 16-byte aligned and inside
    the guarded allocation.  (tail_out: the affine reads the nets' outputs through the same moved pointer, so the FLOW's result is the
    ordinary one -- what differs is the net's own output tensor, taken here from the call that allocates it.)"""
    engine = knobs
    engine.PERSIST_MIN_UNITS = 0
    cfg = _case('m2')[0]
    nets_outs = []
    launch = engine._run_stack_persist

    def spy(path, nets, plans, projs, bufs, outs, *a, **k):
        nets_outs.append(outs)
        return launch(path, nets, plans, projs, bufs, outs, *a, **k)
    monkeypatch.setattr(engine, '_run_stack_persist', spy)
    run = _one_shot(engine, gpu, 'm2', 'f16x3')
    want = run()
    want_net = nets_outs[-1][0].clone()
    del nets_outs[:]
    seen = []

    def move(pa):
        seen.append(pa)
        if len(seen) == cfg.n_iaf:          # the last flow's launch: nothing consumes what it writes
            assert pa.tail_q == 1 and pa.affine_out and pa.tail_out[0] % 16 == 0 and pa.affine_out % 16 == 0
            if which == 'tail_out_forward':
                pa.tail_out[0] = pa.tail_out[0] + 16
            else:
                pa.affine_out = pa.affine_out - 16
    with guarded(*_mods()) as g:
        assert g.band_bytes >= 4096
        engine.PERSIST_ARGS_HOOK = move
        try:
            got = run()
        finally:
            engine.PERSIST_ARGS_HOOK = None
        torch.cuda.synchronize()
        assert len(seen) == cfg.n_iaf and all(e[7] == 1 for e in got.log)
        nbytes = M2_N * M2_T * 4
        found = g.touched()
        assert len(found) == 1, found
        site, shape, dtype, side, offset, count = found[0]
        if which == 'tail_out_forward':
            net = nets_outs[-1][0]
            alloc = g.find(net)
            assert (site, shape, dtype, side) == (alloc.site, (M2_N, M2_T, 1), torch.float32, 'behind') and nbytes <= offset and 1 <= count and offset + count <= nbytes + 16
            assert bool(torch.isnan(net.reshape(-1)[:4]).all()) and torch.equal(net.reshape(-1)[4:], want_net.reshape(-1)[:-4])
            assert not torch.equal(net, want_net) and torch.equal(got.outs[0], want.outs[0])
        else:
            alloc = g.find(got.outs[0])
            assert (site, shape, dtype, side) == (alloc.site, (M2_N, M2_T, 1), torch.float32, 'front') and -16 <= offset and 1 <= count and offset + count <= 0
            y, y0 = got.outs[0].reshape(-1), want.outs[0].reshape(-1)
            assert bool(torch.isnan(y[-4:]).all()) and torch.equal(y[:-4], y0[4:]) and not torch.equal(y, y0)
        with pytest.raises(AssertionError, match=side):
            g.check()
