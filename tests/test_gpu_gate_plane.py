"""-m gpu: the fused gate tanh(F) * sigmoid(G) (gate_act, csrc/pwv_layer_common.h) where no other test takes it -- over the whole (F, G)
plane and with saturated gates on every route.

Every other parity and bit-identity test keeps the pre-activations below |F| = 8.6, |G| = 9.1; gate_act's clamp engages at |F| = 20 and
G = -40, so one instantiation could lose it and every such test would still compare equal.  Here:

1. tests/util.gate_plane() -- 16384 (F, G) pairs, both sides of every threshold of the formula, out to 1e30 -- through one layer launch
   per arithmetic with x_in = 0 (the accumulators are exactly P, which carries the pre-scaled plane), through the packer's own pre-scaling
   (a biases-only row), and through the unfused path's tanhf / expf kernel: assert_gate_plane, whose bars come from the host emulation
   (tests/test_gate_formula_host.py, which also shows that the same assertions reject five wrong gates).
2. tests/util.saturating_weights -- a third of the gates beyond |F| = 20, a tenth below G = -40, a quarter in the ordinary range, the model
   still well conditioned -- on every route: per-layer launches (layer 0 folded and not), both persistent instantiations, the tail inside
   the launch and not, the shared two-output net, packed batches, streaming pushes, the per-sample condition, the fp16 storage mode.
   max |y - y_fp64| <= TOL_F32 (unscaled), torch.equal between routes wherever the suite claims bit identity, and every case shows from
   EVENT_LOG / PERSIST_ARGS_HOOK which kernel ran and that the requested arithmetic was kept."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import iaf_oracle as O
from tests.test_gpu_persist_prefetch import _Launches, knobs  # noqa: F401  (knobs: a fixture)
from tests.test_gpu_stream_persist import _Log, _short_expected
from tests.util import (K_F, K_G, TOL_F32, assert_gate_plane, f16_storage_model, gate_bounds, gate_exact, gate_plane,
                        run_vocoder_hip, saturated_case, set_hparams, small_cfg, untile_f16)

pytestmark = pytest.mark.gpu
PRECS = ['f16x3', 'f32']


@pytest.fixture(autouse=True)
def _default_hparams_afterwards():
    """The hparams are a process-wide singleton: leave the default model behind for whatever runs next."""
    yield
    set_hparams(small_cfg())


# ---- 1. the plane through the kernels -----------------------------------------------------------------------------------------------------
def _gated_layer(gpu, precision, P, T, cond_hop, cond_frames):
    """Layer 0 of a glorot net through pwv_wavenet_layer_f32: G = 1, N = 1, T rows, out_mode PWV_OUT_GATED, no skip, no per-sample condition,
    x_in all zero -- so the accumulators in front of gate_act are exactly the P row of the sample (row (t + 0) / cond_hop of `P`
    [cond_frames, 128]; cond_hop 0: row 0).  Returns the gated output [T, 64] as float64."""
    from pwv_amd import _lib, engine
    from pwv_amd.modules import WaveNet
    from pwv_amd.variables import VariableStore, variable_scope
    lib = _lib.lib()
    prec = engine.PRECISIONS[precision]
    cfg = O.ModelConfig(dilations=[[1, 2]], n_iaf=1, use_skip_connection=False, use_biases=True, cond_upsample_method='none')
    store = VariableStore(device=gpu)
    store.load_dict(O.init_weights(cfg, seed=5))
    with variable_scope('iaf_vocoder'), variable_scope('iaf0'):
        net = WaveNet(batch_size=1, dilations=[1, 2], filter_width=2, residual_channels=64, dilation_channels=64, skip_channels=128,
                      quantization_channels=1, input_channels=1, use_biases=True, condition_channels=None, use_skip_connection=False,
                      name='scalar', store=store, precision=precision)
    plan = engine.get_plan(net, 'none', prec)
    assert plan.precision == prec and plan.f16x3_ok
    assert P.dtype == torch.float32 and tuple(P.shape) == (cond_frames, 128) and P.is_contiguous()
    assert cond_hop == 0 or (T - 1) // cond_hop < cond_frames          # every P row the launch reads exists
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    nb = lib.pwv_tile32_floats(T, 64)
    dtype = torch.float16 if precision == 'f16' else torch.float32
    x_in = torch.zeros(nb, dtype=dtype, device=gpu)
    x_out = torch.full((nb,), 7.0, dtype=dtype, device=gpu)
    a = _lib.LayerArgs()
    a.G, a.N, a.T, a.dilation, a.skip_init = 1, 1, T, 1, 1
    a.proj_row_stride = 128
    a.cond_hop, a.cond_offset, a.cond_frames = cond_hop, 0, cond_frames
    a.precision, a.out_mode = prec, _lib.OUT_GATED
    a.x_in[0], a.x_out[0], a.packed[0], a.proj[0] = x_in.data_ptr(), x_out.data_ptr(), plan.packed_layers[0].data_ptr(), P.data_ptr()
    _lib.check(lib.pwv_wavenet_layer_f32(ctypes.byref(a), s), 'pwv_wavenet_layer_f32')
    torch.cuda.synchronize()
    if precision == 'f16':
        return untile_f16(x_out, T)
    rows = torch.empty((T, 64), device=gpu)
    _lib.check(lib.pwv_tile32_to_rows_f32(x_out.data_ptr(), rows.data_ptr(), T, 64, s), 'pwv_tile32_to_rows_f32')
    torch.cuda.synchronize()
    return rows.cpu().numpy().astype(np.float64)


def _f16_ulp(F, G):
    """One fp16 ulp at max(|want|, 2^-14): what storing the gated output as fp16 may add."""
    return np.spacing(np.maximum(np.abs(gate_exact(F, G)), 2.0 ** -14).astype(np.float16)).astype(np.float64)


def _plane_report(what, got, F, G, precision):
    """assert_gate_plane, and the measured errors next to the bars; an fp16 output against A + one fp16 ulp (its relative error is its rounding's)."""
    A, R = gate_bounds()[:2]
    if precision == 'f16':
        extra = _f16_ulp(F, G)
        err_abs, _ = assert_gate_plane(got, F, G, extra_abs=extra)
        used = float((np.abs(got - gate_exact(F, G)) / (A + extra)).max())
        print('%s: max absolute error %.3g, at most %.2f of A + one fp16 ulp (A = %.3g)' % (what, err_abs, used, A))
    else:
        err_abs, err_rel = assert_gate_plane(got, F, G)
        print('%s: max absolute error %.3g (A = %.3g), max relative error %.3g (R = %.3g)' % (what, err_abs, A, err_rel, R))


@pytest.mark.parametrize('precision', ['f32', 'f16x3', 'f16'])
def test_the_plane_through_a_layer_launch(gpu, precision):
    """512 rows (16 units, several workgroups), cond_hop 2: rows 2k and 2k + 1 read P row k, which carries pairs 64k .. 64k + 63 of the
    permuted plane, pre-scaled on the host in fp32 and laid out in pwv_proj_column_map's order."""
    from pwv_amd import _lib
    F, G, _ = gate_plane()
    cmap = np.array(_lib.proj_column_map())
    assert sorted(cmap.tolist()) == list(range(128))
    by_channel = np.concatenate([F.reshape(256, 64) * K_F, G.reshape(256, 64) * K_G], axis=1)      # [filter 0..63 | gate 64..127], fp32
    assert by_channel.dtype == np.float32
    P = torch.from_numpy(np.ascontiguousarray(by_channel[:, cmap])).to(gpu)
    o = _gated_layer(gpu, precision, P, 512, 2, 256)
    assert np.array_equal(o[0::2], o[1::2], equal_nan=True)          # (a NaN is for assert_gate_plane to report)
    _plane_report('plane through the %s layer kernel' % precision, o[0::2].ravel(), F, G, precision)


def _extreme_pairs():
    """64 (F, G) pairs from the plane's extremes: every fixed value of the axes (tests/util._PLANE_FIXED, both signs, and 0) and seven more
    between them as F, the same values in a seeded order as G."""
    from tests.util import _PLANE_FIXED
    vals = np.array([0.0] + [s * v for v in _PLANE_FIXED for s in (1.0, -1.0)] + [25.0, -25.0, 50.0, -50.0, 70.0, -70.0, 35.0], dtype=np.float32)
    assert vals.shape == (64,)
    return vals, vals[np.random.RandomState(64).permutation(64)]


@pytest.mark.parametrize('precision', ['f32', 'f16x3', 'f16'])
def test_extreme_biases_through_the_packer_and_a_layer_launch(gpu, precision):
    """filter_bias / gate_bias = 64 pairs of extremes, pre-scaled by pwv_pack_proj_f32 itself (no condition: the biases-only row, cond_hop 0),
    70 rows (a ragged third unit): the packer's scaling and column order and the kernel's agree, every row is the same."""
    from pwv_amd import _lib
    F, G = _extreme_pairs()
    fb, gb = torch.from_numpy(F).to(gpu), torch.from_numpy(G).to(gpu)
    proj_b = torch.full((128,), 7.0, device=gpu)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.lib().pwv_pack_proj_f32(None, None, fb.data_ptr(), gb.data_ptr(), 0, 0, 1, None, proj_b.data_ptr(), s), 'pwv_pack_proj_f32')
    o = _gated_layer(gpu, precision, proj_b.view(1, 128), 70, 0, 1)
    assert np.array_equal(o, np.broadcast_to(o[0], o.shape), equal_nan=True)
    _plane_report('extreme biases through pwv_pack_proj_f32 and the %s layer kernel' % precision, o[0], F, G, precision)


def test_the_plane_through_the_unfused_gate(gpu):
    """pwv_gate_f32 (tanhf / expf on the unscaled arguments: the unfused path) at the same bars as the fused gate."""
    from pwv_amd import engine
    F, G, _ = gate_plane()
    got = engine.gate_op(torch.from_numpy(F.copy()).to(gpu), torch.from_numpy(G.copy()).to(gpu))
    torch.cuda.synchronize()
    err_abs, err_rel = assert_gate_plane(got.cpu().numpy(), F, G)
    print('plane through pwv_gate_f32: max absolute error %.3g, max relative error %.3g' % (err_abs, err_rel))


# ---- 2. saturated gates on every route ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _want(kind):
    """The fp64 oracle of tests/util.saturated_case(kind): computed once, shared, never written to."""
    cfg, w, mel, z = saturated_case(kind)
    y = O.iaf_vocoder_forward(w, mel, z, cfg)
    y.setflags(write=False)
    return y


class _Watch(_Launches):
    """_Launches, and the arithmetic: the precision of every flow the engine prepared inside the block (a flow whose split-fp16 plan fails
    its pack-time bounds is prepared in 'f32' instead) and of every persistent launch, and whether the launch carried the affine."""

    def __init__(self, engine, precision):
        super().__init__(engine)
        self.precision, self.precs = precision, []

    def _hook(self, pa):
        super()._hook(pa)
        self.seen[-1].update(prec=int(pa.precision), affine=bool(pa.affine_x))

    def __enter__(self):
        self._real = (self.engine._prepare_flow, self.engine._prepare_flow_stream)

        def spy(real):
            def wrapped(*a, **k):
                prep = real(*a, **k)
                self.precs.append(prep.precision)
                return prep
            return wrapped
        self.engine._prepare_flow, self.engine._prepare_flow_stream = spy(self._real[0]), spy(self._real[1])
        return super().__enter__()

    def __exit__(self, *exc):
        self.engine._prepare_flow, self.engine._prepare_flow_stream = self._real
        super().__exit__(*exc)
        if exc[0] is None:
            torch.cuda.synchronize()
            assert self.engine.persist_status() == 0 and not self.engine.range_flag_raised()
            assert self.precs and set(self.precs) == {self.precision}, self.precs          # the requested arithmetic, in every flow
            assert all(a['prec'] == self.engine.PRECISIONS[self.precision] for a in self.seen), self.seen

    def kinds(self):
        return [e[0] for e in self.log]


def _forward(engine, kind, gpu, precision):
    """saturated_case(kind) through the reference-shaped call (enqueue-only + verify(): no self-repair): (y, the watch)."""
    cfg, w, mel, z = saturated_case(kind)
    with _Watch(engine, precision) as wt:
        got = run_vocoder_hip(cfg, w, mel, z, gpu, precision=precision)
    return got, wt


def _meets_oracle(got, want, what):
    err = float(np.abs(got - want).max())
    print('%s: max |y - y_fp64| = %.3g (TOL_F32 = %.3g)' % (what, err, TOL_F32))
    assert got.shape == want.shape and np.isfinite(got).all() and err <= TOL_F32, (what, err)


@pytest.mark.parametrize('precision', PRECS)
def test_saturated_per_layer_launches_folded_and_unfolded(gpu, knobs, precision):
    engine = knobs
    engine.PERSIST = False
    want, res = _want('small'), {}
    for fold in (True, False):
        engine.FOLD_FIRST = fold
        res[fold], wt = _forward(engine, 'small', gpu, precision)
        assert wt.kinds() and set(wt.kinds()) == {'layer_residual'} and not wt.seen, wt.kinds()
        _meets_oracle(res[fold], want, 'per-layer launches, layer 0 %s, %s' % ('folded' if fold else 'unfolded', precision))
    # (another evaluation order of layer 0: the same function within the path's tolerance, as in test_folded_layer0_is_the_same_function_on_every_path)
    assert np.abs(res[True] - res[False]).max() <= 2e-5 * max(1.0, float(np.abs(res[True]).max()))


@pytest.mark.parametrize('precision', PRECS)
def test_saturated_persistent_short_input_instantiation(gpu, knobs, precision):
    """hop_cfg(80), 2 x 480: one persistent launch per flow in the short-input instantiation, the tail inside it (FUSE_TAIL) and as a launch of
    its own -- both the per-layer launches' bits."""
    engine = knobs
    cfg = saturated_case('small')[0]
    engine.PERSIST = False
    per_layer, _ = _forward(engine, 'small', gpu, precision)
    engine.PERSIST, engine.PERSIST_MIN_UNITS = True, 0
    for fuse_tail in (True, False):
        engine.FUSE_TAIL = fuse_tail
        got, wt = _forward(engine, 'small', gpu, precision)
        assert wt.kinds() == ['persist'] * cfg.n_iaf and len(wt.seen) == cfg.n_iaf, wt.kinds()
        for e, a, dil in zip(wt.log, wt.seen, cfg.dilations):
            assert e[3] == 2 and e[4] == len(dil) - 1 and e[5] == 1 and e[6] == int(fuse_tail), e
            assert e[7] == a['short'] == 1 == _short_expected(2 * 480, max(dil), gpu), (e[7], a)
            assert a['folded'] and a['x_first'] and a['affine'] == fuse_tail and not a['packed'] and not a['stream'], a
        _meets_oracle(got, _want('small'), 'persistent, short-input instantiation, tail %s, %s' % ('inside' if fuse_tail else 'separate', precision))
        assert np.array_equal(got, per_layer), float(np.abs(got - per_layer).max())


@pytest.mark.parametrize('precision', PRECS)
def test_saturated_persistent_general_instantiation(gpu, knobs, precision):
    """Dilations [1, 2, 32, 64, 48, 512, 4] at 1 x 2080 with PERSIST_MIN_UNITS = 16: 13 units per workgroup, the general loop with d = 512 inside
    it; the tail inside the launch and not."""
    engine = knobs
    engine.PERSIST = False
    per_layer, _ = _forward(engine, 'dil7', gpu, precision)
    engine.PERSIST, engine.PERSIST_MIN_UNITS = True, 16
    for fuse_tail in (True, False):
        engine.FUSE_TAIL = fuse_tail
        got, wt = _forward(engine, 'dil7', gpu, precision)
        wt.check_general(2080, 1)
        assert all(e[4] == 6 and e[5] == 1 and e[6] == int(fuse_tail) for e in wt.log), wt.log
        assert all(a['folded'] and a['x_first'] and a['affine'] == fuse_tail for a in wt.seen), wt.seen
        _meets_oracle(got, _want('dil7'), 'persistent, general instantiation, tail %s, %s' % ('inside' if fuse_tail else 'separate', precision))
        assert np.array_equal(got, per_layer), float(np.abs(got - per_layer).max())


@pytest.mark.parametrize('precision', PRECS)
def test_saturated_shared_two_output_net(gpu, knobs, precision):
    """One net per flow with scale and shift as its two outputs: the persistent launch evaluates the affine in place."""
    engine = knobs
    cfg = saturated_case('shared')[0]
    engine.PERSIST = False
    per_layer, wt = _forward(engine, 'shared', gpu, precision)
    assert set(wt.kinds()) == {'layer_residual'} and not wt.seen
    _meets_oracle(per_layer, _want('shared'), 'shared net, per-layer launches, %s' % precision)
    engine.PERSIST = True
    got, wt = _forward(engine, 'shared', gpu, precision)
    assert wt.kinds() == ['persist'] * cfg.n_iaf and all(e[3] == 1 and e[5] == 1 and e[6] == 1 for e in wt.log), wt.log
    assert all(a['affine'] and a['folded'] for a in wt.seen), wt.seen
    _meets_oracle(got, _want('shared'), 'shared net, persistent launch with the affine, %s' % precision)
    assert np.array_equal(got, per_layer), float(np.abs(got - per_layer).max())


@pytest.mark.parametrize('precision', PRECS)
def test_saturated_per_sample_condition(gpu, knobs, precision):
    """cond_upsample_method 'transposed_conv': the condition GEMM runs inside the layer kernels, in front of the same gate (layer 0 folded and
    not); no persistent form."""
    engine = knobs
    engine.PERSIST = True
    for fold in (True, False):
        engine.FOLD_FIRST = fold
        got, wt = _forward(engine, 'transposed', gpu, precision)
        assert set(wt.kinds()) == {'layer_residual'} and not wt.seen, wt.kinds()
        _meets_oracle(got, _want('transposed'), 'per-sample condition, layer 0 %s, %s' % ('folded' if fold else 'unfolded', precision))


def _model(gpu, kind, precision):
    from pwv_amd.models import IAFVocoder
    from pwv_amd.variables import VariableStore
    cfg, w, _, _ = saturated_case(kind)
    set_hparams(cfg)
    store = VariableStore(device=gpu)
    store.load_dict(w)
    return IAFVocoder(batch_size=1, length=cfg.hop_length, store=store, precision=precision), cfg, w


def _alone(model, cfg, mel_t, z_t):
    """The one-shot forward of one utterance on the default route."""
    from pwv_amd.models import IAFVocoder
    one = IAFVocoder(batch_size=1, length=(mel_t.shape[0] - 1) * cfg.hop_length, store=model.store, precision=model.precision)
    return one(None, mel_t[None], is_training=False, z=z_t[None])[0]


@pytest.mark.parametrize('precision', PRECS)
def test_saturated_packed_batch(gpu, knobs, monkeypatch, precision):
    """generate_varlen with lengths 160, 480 and 320: one packed persistent launch per flow; every piece equals its utterance alone bit for
    bit and meets the oracle."""
    engine = knobs
    model, cfg, w = _model(gpu, 'small', precision)
    lengths = [160, 480, 320]
    rng = np.random.default_rng(3)
    mels = [rng.uniform(-1, 1, (L // cfg.hop_length + 1, cfg.n_mels)).astype(np.float32) for L in lengths]
    zs = [np.clip(rng.logistic(0, 1, (L, 1)), -20, 20).astype(np.float32) for L in lengths]
    mel_t, z_t = [torch.from_numpy(m).to(gpu) for m in mels], [torch.from_numpy(z).to(gpu) for z in zs]
    monkeypatch.setattr(engine, 'VARLEN_PADDED', 0)
    with _Watch(engine, precision) as wt:
        out = model.generate_varlen(mel_t, z=z_t, verify=False)
        model.verify()
    assert engine.VARLEN_PADDED == 0 and wt.kinds() == ['persist'] * cfg.n_iaf
    assert all(a['packed'] and a['rows'] == sum(lengths) and a['affine'] for a in wt.seen) and len(wt.seen) == cfg.n_iaf, wt.seen
    for L, m, z, mt, zt, piece in zip(lengths, mels, zs, mel_t, z_t, out):
        assert torch.equal(piece, _alone(model, cfg, mt, zt)), L
        _meets_oracle(piece.cpu().numpy(), O.iaf_vocoder_forward(w, m[None], z[None], cfg)[0], 'packed batch, utterance of %d, %s' % (L, precision))


@pytest.mark.parametrize('route', ['persistent', 'per_layer'])
@pytest.mark.parametrize('precision', PRECS)
def test_saturated_streaming_pushes(gpu, knobs, precision, route):
    """Two sessions: the first frame, then pushes of 2, 1 and 3 frames onto the history the earlier ones left, as one persistent streaming
    launch per flow and push, or as the per-layer streaming launches.  The pieces concatenate to each session's one-shot forward bit for
    bit, and meet the oracle."""
    engine = knobs
    model, cfg, _ = _model(gpu, 'small', precision)
    _, _, mel, z = saturated_case('small')
    n, hop, schedule = mel.shape[0], cfg.hop_length, [2, 1, 3]
    assert sum(schedule) * hop == z.shape[1]
    mel_t, z_t = torch.from_numpy(mel).to(gpu), torch.from_numpy(z).to(gpu)
    engine.PERSIST = True if route == 'persistent' else False
    s = model.open_stream(slots=n)
    outs, f0, e0 = [], 1, 0
    with _Watch(engine, precision) as wt:
        assert tuple(s.push(mel_t[:, :1], z=z_t[:, :0]).shape) == (n, 0, 1)
        for f in schedule:
            outs.append(s.push(mel_t[:, f0:f0 + f], z=z_t[:, e0:e0 + f * hop], verify=False))
            s.verify()
            f0, e0 = f0 + f, e0 + f * hop
    if route == 'persistent':
        lg = _Log(engine)
        lg.log = wt.log
        lg.check(cfg, [n * f * hop for f in schedule], gpu)
        assert all(a['stream'] and a['folded'] for a in wt.seen) and len(wt.seen) == cfg.n_iaf * len(schedule)
    else:
        assert wt.kinds() == ['layer_stream'] * (cfg.n_iaf * len(schedule)) and not wt.seen
    got = torch.cat(outs, dim=1)
    engine.PERSIST = 'auto'
    for i in range(n):
        assert torch.equal(got[i], _alone(model, cfg, mel_t[i], z_t[i])), i
    _meets_oracle(got.cpu().numpy(), _want('small'), 'streaming pushes of 2, 1, 3 frames, %s launches, %s' % (route, precision))


def test_saturated_f16_storage_mode(gpu):
    """precision 'f16' against the fp64 oracle run on the mode's own storage model (tests/util.f16_storage_model), at the bar of
    tests/test_gpu_f16.py; bitwise repeatable."""
    from tests.test_gpu_f16 import TOL_F16
    cfg, w, mel, z = saturated_case('small')
    w16, r16 = f16_storage_model(w, cfg)
    want = O.iaf_vocoder_forward(w16, mel, z, cfg, act_round=r16)
    a = run_vocoder_hip(cfg, w, mel, z, gpu, precision='f16')
    b = run_vocoder_hip(cfg, w, mel, z, gpu, precision='f16')
    err = float(np.abs(a - want).max())
    print('f16 storage mode, saturated gates: max |y - storage model| = %.3g (TOL_F16 = %.3g), against the exact model %.3g'
          % (err, TOL_F16, np.abs(a - _want('small')).max()))
    assert np.array_equal(a, b) and np.isfinite(a).all() and err <= TOL_F16, err
