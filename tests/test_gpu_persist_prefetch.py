"""-m gpu: the general loop of the persistent kernel (csrc/pwv_persist_tasks.inc, MODE 0) on the smallest shapes that reach every
path of load_x() -- the loads of the next unit's rows, which tests/test_persist_prefetch_isa.py looks at in the assembly: the look-back
inside the unit (d = 1, 2), on unit boundaries (32, 64), off them (48) and longer than a workgroup's range (512: the first 16 units have
rows left of the utterance start, zeroed per lane), units that span two utterances (has_prev is not wave-uniform), the unfolded layer 0
(FOLD_FIRST off: the four-scalar path), a packed batch and a streaming push onto a carried history.  Persistent launch against per-layer
launches, torch.equal, both arithmetics.  PERSIST_MIN_UNITS = 16 forces the general instantiation at these sizes (13 to 16 units per
workgroup); every case asserts from EVENT_LOG and PERSIST_ARGS_HOOK that this is what ran."""
import ctypes

import pytest
import torch

from oracle import iaf_oracle as O
from tests.util import set_hparams, small_cfg

pytestmark = pytest.mark.gpu

DIL6 = [1, 2, 32, 64, 48, 512]
# ... and with one more layer behind it: the launch covers all layers but the last, so only here does d = 512 run INSIDE the loop
DIL7 = DIL6 + [4]


@pytest.fixture()
def knobs():
    from pwv_amd import engine
    names = ('PERSIST', 'PERSIST_MIN_UNITS', 'PERSIST_MAX_LAYERS', 'FOLD_FIRST', 'FUSE_TAIL', 'EVENT_LOG', 'PERSIST_ARGS_HOOK')
    saved = [getattr(engine, k) for k in names]
    engine.resume_persist()
    try:
        yield engine
    finally:
        for k, v in zip(names, saved):
            setattr(engine, k, v)
        engine.resume_persist()


class _Launches:
    """Every persistent launch inside the block: (units per workgroup by persist_plan's arithmetic, the library's short-input verdict,
    packed?, streaming?, layer 0 folded?) from the filled-in pwv_persist_args, and EVENT_LOG."""

    def __init__(self, engine):
        self.engine, self.seen = engine, []

    def _hook(self, pa):
        from pwv_amd import _lib
        lib = _lib.lib()
        rows = int(pa.varlen_rows) if pa.cu_rows else pa.N * pa.T
        units = -(-rows // 32)
        nwg = min(lib.pwv_device_cus() // pa.G, max(1, -(-units // (pa.min_units_per_workgroup or 4))))
        self.seen.append(dict(per_wg=-(-units // nwg), short=int(lib.pwv_persist_short_input(ctypes.byref(pa))), packed=bool(pa.cu_rows),
                              stream=bool(pa.hist), x_first=bool(pa.x_first), folded=bool(pa.first_fold[0]), rows=rows))

    def __enter__(self):
        self.log = self.engine.EVENT_LOG = []
        self.engine.PERSIST_ARGS_HOOK = self._hook
        return self

    def __exit__(self, *exc):
        self.engine.EVENT_LOG = None
        self.engine.PERSIST_ARGS_HOOK = None

    def check_general(self, rows, launches):
        """`launches` persistent launches of `rows` rows, all of the general instantiation with more than 7 units per workgroup"""
        assert [e[0] for e in self.log] == ['persist'] * launches and len(self.seen) == launches, ([e[0] for e in self.log], len(self.seen))
        assert all(e[7] == 0 for e in self.log)
        assert all(a['short'] == 0 and a['per_wg'] > 7 and a['rows'] == rows for a in self.seen), self.seen


def _nets(gpu, dilations, G=2, seed=3):
    from pwv_amd.modules import WaveNet
    from pwv_amd.variables import VariableStore
    store = VariableStore(device=gpu, seed=seed)
    kw = dict(batch_size=1, dilations=list(dilations), filter_width=2, residual_channels=64, dilation_channels=64, skip_channels=128,
              quantization_channels=1, use_biases=True, condition_channels=80, use_skip_connection=False, is_training=False, store=store)
    return store, [WaveNet(name='n%d' % g, **kw) for g in range(G)]


@pytest.mark.parametrize('precision', ['f16x3', 'f32'])
@pytest.mark.parametrize('fold', [True, False], ids=['folded', 'unfolded'])
@pytest.mark.parametrize('n,t,dilations', [(1, 2080, DIL6), (3, 1000, DIL6), (1, 2080, DIL7)], ids=['1x2080', '3x1000', '1x2080_d512_inside'])
def test_general_loop_is_bit_identical_to_per_layer_launches(gpu, knobs, n, t, dilations, fold, precision):
    engine = knobs
    engine.FOLD_FIRST = fold
    store, nets = _nets(gpu, dilations)
    g = torch.Generator().manual_seed(n * 7 + len(dilations))
    x = torch.randn((n, t, 1), generator=g).to(gpu)
    cond = engine.RepeatedCondition(torch.rand((n, t // 80 + 1, 80), generator=g).to(gpu), 80, 40, t)
    engine.PERSIST = False
    engine.run_nets(nets, x, cond, precision=precision)      # creates the variables
    for name in list(store.vars):
        if store.vars[name].dim() == 1:
            store.vars[name].normal_(0, 0.1)
    store.version += 1
    ref = [o.clone() for o in engine.run_nets(nets, x, cond, precision=precision)]
    engine.PERSIST, engine.PERSIST_MIN_UNITS = True, 16
    with _Launches(engine) as la:
        for _ in range(2):
            got = engine.run_nets(nets, x, cond, precision=precision)
            torch.cuda.synchronize()
            assert engine.persist_status() == 0
            for a, b in zip(ref, got):
                assert torch.equal(a, b), float((a - b).abs().max())
        la.check_general(n * t, 2)
        # one launch per forward: layers 0 .. L-2, starting at the net's layer 0 in the form asked for
        assert all(e[4] == len(dilations) - 1 and e[5] == 1 for e in la.log)
        assert all(a['x_first'] and a['folded'] == fold and not a['packed'] and not a['stream'] for a in la.seen)


@pytest.mark.parametrize('precision', ['f16x3', 'f32'])
def test_general_loop_packed_batch(gpu, knobs, precision):
    """3 x 1000 as a packed batch (no condition, so the lengths need not be multiples of a hop): units span two utterances; every utterance
    equals its own flow on per-layer launches."""
    from pwv_amd.modules import LinearIAFLayer, WaveNet
    from pwv_amd.variables import VariableStore
    engine = knobs
    set_hparams(O.ModelConfig())
    store = VariableStore(device=gpu)
    kw = dict(batch_size=1, dilations=list(DIL6), filter_width=2, residual_channels=64, dilation_channels=64, skip_channels=128,
              use_skip_connection=False, is_training=False, store=store, precision=precision, quantization_channels=1)
    flow = LinearIAFLayer(1, WaveNet(name='scalar', **kw), WaveNet(name='shifter', **kw))
    geom = engine.VarlenGeometry([1000, 1000, 1000], 1, gpu)
    R = geom.rows
    torch.manual_seed(0)
    x = torch.randn((R, 1), device=gpu)
    for net in flow.nets():           # create the variables (a uniform call), small random weights
        net(x[:64][None], None)
    for k, v in store.vars.items():
        v.copy_(torch.randn_like(v) * 0.1)
    store.version += 1
    engine.PERSIST = False
    want = [engine.run_flow(flow.nets(), x[a:b][None], None, precision=precision).clone() for a, b in zip(geom.cu_rows_host, geom.cu_rows_host[1:])]
    engine.PERSIST, engine.PERSIST_MIN_UNITS = True, 16
    out = torch.empty((1, R, 1), device=gpu)
    with _Launches(engine) as la:
        res = engine._run_nets(flow.nets(), x.view(1, R, 1), None, precision, 0, out, geom)
        torch.cuda.synchronize()
        assert engine.persist_status() == 0
        assert res is not None and res[1], 'the packed flow must run as a persistent launch with the affine inside'
        la.check_general(R, 1)
        assert all(a['packed'] and a['x_first'] and a['folded'] for a in la.seen)
    for (a, b), w in zip(zip(geom.cu_rows_host, geom.cu_rows_host[1:]), want):
        assert torch.equal(out[0, a:b], w[0]), float((out[0, a:b] - w[0]).abs().max())


@pytest.mark.parametrize('precision', ['f16x3', 'f32'])
def test_general_loop_streaming_push_onto_carried_history(gpu, knobs, precision):
    """Two sessions, two pushes of 2 x 1040 rows each: the second continues the history the first has left (every dilation but 512 is
    below the chunk: rows left of the chunk come from the history, not zeros).  Outputs and every byte of the history arrays equal
    those of the per-layer streaming launches."""
    from tests.test_gpu_stream import _Feeder, _inputs, _model
    engine = knobs
    cfg = small_cfg(dilations=[DIL6, [1, 2, 4, 8]])
    model, _ = _model(gpu, cfg, precision)
    T, S = 1040, 2
    ins = [_inputs(cfg, 2 * T, gpu, seed=40 + i) for i in range(S)]
    res = {}
    for persist in (False, True):
        engine.PERSIST, engine.PERSIST_MIN_UNITS = persist, 16
        s = model.open_stream(slots=S)
        fd = _Feeder(s)
        for i in range(S):
            fd.start(i, ins[i][2], ins[i][3])
        fd.adv([0, 1], T)
        with _Launches(engine) as la:
            fd.adv([0, 1], T)
            torch.cuda.synchronize()
            if persist:
                assert engine.persist_status() == 0
                la.check_general(S * T, cfg.n_iaf)      # one streaming launch per flow: layer 0 folded .. the tail
                assert all(a['stream'] and a['x_first'] and a['folded'] and not a['packed'] for a in la.seen)
                assert all(e[8] == 1 and e[5] == 1 and e[6] == 1 for e in la.log)
            else:
                assert [e[0] for e in la.log] == ['layer_stream'] * cfg.n_iaf and not la.seen
        res[persist] = ([fd.result(i).clone() for i in range(S)], s._hist.clone())
    for a, b in zip(res[True][0], res[False][0]):
        assert torch.equal(a, b), float((a - b).abs().max())
    assert torch.equal(res[True][1], res[False][1]), int((res[True][1] != res[False][1]).sum())
    assert all(bool(torch.isfinite(a).all()) for a in res[True][0])
