"""GPU: the conditioning geometry at hop lengths other than 80, on every route (the CPU side: tests/test_hop_geometry_host.py, which
also shows that a condition off by one sample or one frame moves the oracle by >= 100 x TOL_F32 on the very cases used here).

Sample t of utterance n reads P row n * cond_frames + (t + cond_offset) / cond_hop (cu_frames[i] + ... in packed launches); the division
is a host-built magic multiply (make_magic / fast_div, csrc/pwv_layer_common.h) at one site in each per-layer kernel and four in the
persistent ones.  Every other test runs hop 80 / offset 40: neither a power of two nor below the 32-row unit.  Here: tests/util.HOPS
through the one-shot forward on per-layer launches and on both persistent instantiations, arbitrary (hop, offset) pairs at the layer
level, pwv_upsample_repeat_f32 / pwv_crop_time_f32 called directly, packed batches (with an utterance under 32 samples, which hop 80
cannot build: the padded fallback), their graph replay, streaming pushes of 16 rows, a ragged tick with a 16-row session (the grouped
route with PERSIST at its default), graphed ticks, the fp16 storage mode, time shards, and the refusal of odd hops.  A test that claims
a route shows from engine.EVENT_LOG / PERSIST_ARGS_HOOK that it ran.  Oracle comparisons: TOL_F32; route against route: equal bits."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import iaf_oracle as O
from tests.test_gpu_parity import _wavenet_case
from tests.test_gpu_persist import persist_knobs  # noqa: F401  (a fixture)
from tests.test_gpu_stream import _inputs, _model
from tests.test_gpu_stream_persist import _Log, _random_state, _short_expected, knobs  # noqa: F401  (knobs: a fixture)
from tests.util import HOP_CASES, HOPS, TOL_F32, hop_cfg, run_vocoder_hip, set_hparams, small_cfg

pytestmark = pytest.mark.gpu
PRECS = ['f16x3', 'f32']


@pytest.fixture(autouse=True)
def _hop_80_afterwards():
    """The hparams are a process-wide singleton: leave the reference's hop behind for whatever runs next."""
    yield
    set_hparams(small_cfg())


def _wide_cfg(hop):
    # tests/test_gpu_stream.py's _small_wide: most dilations above a chunk of a few frames, two that are no multiple of 32
    return small_cfg(dilations=[[1, 96, 128, 256], [2, 64, 200, 512, 3, 160]], hop_length=hop)


def _one_shot(model, hop, mel_t, z_t=None, seed=None, precision=None):
    from pwv_amd.models import IAFVocoder
    one = IAFVocoder(batch_size=1, length=(mel_t.shape[0] - 1) * hop, store=model.store, precision=precision or model.precision)
    if seed is not None:
        one.noise_seed, one.noise_offset = seed, 0
    return one(None, mel_t[None], is_training=False, z=None if z_t is None else z_t[None])[0]


_CASES = {}


def _case(hop, method='repeat'):
    """(cfg, weights, mel, z, fp64 oracle) of the one-shot case of `hop`: computed once, shared, never written to."""
    key = (hop, method)
    if key not in _CASES:
        cfg = hop_cfg(hop, cond_upsample_method=method)
        n, length = HOP_CASES[hop]
        w = O.init_weights(cfg, seed=2)
        mel, z = O.synthetic_inputs(n, length, cfg)
        want = O.iaf_vocoder_forward(w, mel, z, cfg)
        want.setflags(write=False)
        _CASES[key] = (cfg, w, mel, z, want)
    return _CASES[key]


def _logged(engine, fn):
    """fn() with the event log on and every persistent launch's arguments recorded: (result, log, launches)."""
    from pwv_amd import _lib
    seen = []

    def hook(pa):
        seen.append(dict(N=pa.N, T=pa.T, hop=pa.cond_hop, offset=pa.cond_offset, frames=pa.cond_frames, min_units=pa.min_units_per_workgroup,
                         packed=bool(pa.cu_rows), short=int(_lib.lib().pwv_persist_short_input(ctypes.byref(pa)))))
    log = engine.EVENT_LOG = []
    engine.PERSIST_ARGS_HOOK = hook
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        engine.EVENT_LOG, engine.PERSIST_ARGS_HOOK = None, None
    return out, log, seen


def _one_shot_routes(gpu, engine, hop, precision, method='repeat'):
    """The case of `hop` on per-layer launches, on the persistent launch as the library plans it (min_units 0: short inputs take the
    short-input instantiation) and on the persistent launch of one workgroup per net (min_units 64: the general instantiation): each
    shown to have run, each within the fp32 bar of the oracle, the persistent results bit-identical to the per-layer one."""
    cfg, w, mel, z, want = _case(hop, method)
    n, length = HOP_CASES[hop]
    tol = TOL_F32 * max(1.0, float(np.abs(want).max()))
    cond_geom = (hop, hop // 2, length // hop + 1) if method == 'repeat' else (0, 0, 0)
    kinds, per_layer = set(), None
    for persist, min_units in ((False, 0), (True, 0), (True, 64)):
        engine.PERSIST, engine.PERSIST_MIN_UNITS = persist, min_units
        got, log, seen = _logged(engine, lambda: run_vocoder_hip(cfg, w, mel, z, gpu, precision=precision))
        err = float(np.abs(got - want).max())
        print('hop %d %s %s persist=%s min_units=%d: max|y - oracle| = %.3g (bar %.3g), pwv_persist_short_input = %s'
              % (hop, method, precision, persist, min_units, err, tol, [a['short'] for a in seen]))
        assert got.shape == want.shape and err <= tol, (hop, persist, min_units, err)
        if not persist:
            assert log and not seen and all(e[0] == 'layer_residual' for e in log), [e[0] for e in log]
            per_layer = got
            continue
        assert [e[0] for e in log] == ['persist'] * cfg.n_iaf, [e[0] for e in log]
        for e, a, dil in zip(log, seen, cfg.dilations):
            assert e[3] == 2 and e[4] == len(dil) - 1 and e[5] == 1 and e[6] == 1, e          # both nets, layers 0 .. L-2 and the tail
            assert (a['N'], a['T'], a['hop'], a['offset'], a['frames']) == (n, length) + cond_geom and not a['packed'], a
            assert e[7] == a['short'] == _short_expected(n * length, max(dil), gpu, min_units=min_units or 4), (e[7], a)
            kinds.add(e[7])
        assert np.array_equal(got, per_layer), float(np.abs(got - per_layer).max())
    assert kinds == {0, 1}, kinds          # the library offers both instantiations for every one of these shapes


# ---- 1. the one-shot forward against the fp64 oracle, per route ------------------------------------------------------------------------
@pytest.mark.parametrize('precision', PRECS)
@pytest.mark.parametrize('hop', HOPS)
def test_one_shot_forward_on_every_route(gpu, persist_knobs, hop, precision):
    _one_shot_routes(gpu, persist_knobs, hop, precision)


@pytest.mark.parametrize('precision', PRECS)
def test_one_shot_forward_without_a_condition(gpu, persist_knobs, precision):
    """cond_upsample_method 'none' at hop 48 (cond_hop == 0: no division at all; the hop still sets t_mel and the legal lengths)."""
    _one_shot_routes(gpu, persist_knobs, 48, precision, method='none')


# ---- 2. any (hop, offset) at the layer level -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', PRECS)
@pytest.mark.parametrize('hop,offset,T', [(3, 0, 70), (3, 2, 70), (7, 3, 70), (32, 0, 70), (32, 31, 70), (80, 79, 170), (256, 128, 500)])
def test_layer_level_any_hop_and_offset(gpu, persist_knobs, hop, offset, T, precision):
    """engine.RepeatedCondition and pwv_layer_args take any (hop, offset); the oracle condition is frames[:, (t + offset) // hop].  Two
    utterances of T rows (at least two frame boundaries inside each, T no multiple of 32) and three of 20 rows (T < 32: the per-lane
    division of unit_rows), on per-layer launches and on the persistent launch; the frames hold exactly the rows needed, and once one
    spare row per utterance (the P row of utterance n is n * cond_frames + ..., not n * the rows used)."""
    engine = persist_knobs
    assert (T - 1 + offset) // hop >= 2
    for persist in (False, True):
        for n, t, spare in ((2, T, 0), (3, 20, 0)) + (((2, T, 1), (3, 20, 1)) if persist else ((2, T, 1),)):
            engine.PERSIST = persist
            _, log, seen = _logged(engine, lambda: _wavenet_case(gpu, 'frames', False, True, 1, T=t, N=n, precision=precision,
                                                                  geom=(hop, offset), spare=spare))
            if persist:
                assert [e[0] for e in log] == ['persist'] and len(seen) == 1, [e[0] for e in log]
                assert (seen[0]['N'], seen[0]['T'], seen[0]['hop'], seen[0]['offset']) == (n, t, hop, offset), seen
                assert seen[0]['frames'] == (t - 1 + offset) // hop + 1 + spare
            else:
                assert log and not seen and all(e[0] == 'layer_residual' for e in log), [e[0] for e in log]


# ---- 3. pwv_upsample_repeat_f32 and pwv_crop_time_f32, called directly -----------------------------------------------------------------
_PAIRS = [(3, 0), (3, 2), (7, 3), (32, 0), (32, 31), (80, 79), (256, 128), (2, 1), (16, 8), (48, 24)]


@pytest.mark.parametrize('C', [4, 80])
@pytest.mark.parametrize('hop,offset', _PAIRS)
def test_upsample_repeat_direct(gpu, hop, offset, C):
    """out[n, t, :] = frames[n, (t + offset) / hop, :] (include/pwv_hip.h): a copy, so exactly numpy's; T = 0 writes nothing; a T that
    needs more than t_mel frames is PWV_EINVAL (one sample past the last frame's reach)."""
    from pwv_amd import _lib
    lib, s = _lib.lib(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rng = np.random.RandomState(hop * 131 + offset)
    N, t_mel = 3, 4
    frames = rng.randn(N, t_mel, C).astype(np.float32)
    f_t = torch.from_numpy(frames).to(gpu)
    longest = t_mel * hop - offset
    for T in (longest, max(1, longest - hop - 3), 1, 0):
        buf = torch.full((N * T * C + 64,), -7.0, device=gpu)          # (64 floats behind the result: a guard band)
        _lib.check(lib.pwv_upsample_repeat_f32(f_t.data_ptr(), buf.data_ptr(), N, t_mel, C, T, hop, offset, s), 'pwv_upsample_repeat_f32')
        want = frames[:, (np.arange(T) + offset) // hop, :]
        assert np.array_equal(buf[:N * T * C].view(N, T, C).cpu().numpy(), want), (hop, offset, T)
        assert bool((buf[N * T * C:] == -7.0).all())
    out = torch.full((N, longest + 1, C), -7.0, device=gpu)
    assert lib.pwv_upsample_repeat_f32(f_t.data_ptr(), out.data_ptr(), N, t_mel, C, longest + 1, hop, offset, s) == -1      # PWV_EINVAL
    assert b't_mel' in lib.pwv_last_error()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())          # refused before anything was launched


@pytest.mark.parametrize('C', [4, 80])
@pytest.mark.parametrize('hop', [2, 3, 7, 16, 32, 48, 80, 256])
def test_crop_time_direct(gpu, hop, C):
    """out[n, t, :] = in[n, t + offset, :] (the crop at models.py:124): [hop // 2 : -(hop // 2)] of t_mel * hop rows and odd crops, exactly
    numpy's; T_out = 0; offset + T_out > T_in is PWV_EINVAL."""
    from pwv_amd import _lib
    lib, s = _lib.lib(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rng = np.random.RandomState(hop)
    N, T_in = 3, 3 * hop + 1
    x = rng.randn(N, T_in, C).astype(np.float32)
    x_t = torch.from_numpy(x).to(gpu)
    for T_out, offset in ((T_in - 1 - 2 * (hop // 2), hop // 2), (T_in - hop, hop - 1), (T_in, 0), (1, T_in - 1), (0, 5)):
        buf = torch.full((N * T_out * C + 64,), -7.0, device=gpu)          # (64 floats behind the result: a guard band)
        _lib.check(lib.pwv_crop_time_f32(x_t.data_ptr(), buf.data_ptr(), N, T_in, C, T_out, offset, s), 'pwv_crop_time_f32')
        assert np.array_equal(buf[:N * T_out * C].view(N, T_out, C).cpu().numpy(), x[:, offset:offset + T_out, :]), (hop, T_out, offset)
        assert bool((buf[N * T_out * C:] == -7.0).all())
    out = torch.full((N, T_in, C), -7.0, device=gpu)
    assert lib.pwv_crop_time_f32(x_t.data_ptr(), out.data_ptr(), N, T_in, C, T_in, 1, s) == -1      # PWV_EINVAL: one row past the end
    assert b'bad crop' in lib.pwv_last_error()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


def test_materialised_condition_matches_the_oracle(gpu):
    """IAFVocoder._upsample_cond (RepeatedCondition.materialize -> pwv_upsample_repeat_f32) against the oracle's tile / reshape / crop."""
    from pwv_amd.models import IAFVocoder
    from pwv_amd.variables import VariableStore
    for hop in HOPS:
        cfg, w, mel, _, _ = _case(hop)
        n, length = HOP_CASES[hop]
        set_hparams(cfg)
        store = VariableStore(device=gpu)
        store.load_dict(w)
        got = IAFVocoder(n, length, store=store)._upsample_cond(torch.from_numpy(mel).to(gpu), is_training=False, strides=[4, 4, 5])
        want = O.upsample_cond_repeat(w, mel, hop)
        assert tuple(got.shape) == want.shape == (n, length, 80)
        assert np.abs(got.cpu().numpy() - want).max() <= 1e-5


# ---- 4. packed batches -----------------------------------------------------------------------------------------------------------------
def _packed_inputs(cfg, lengths, gpu, seed):
    rng = np.random.default_rng(seed)
    mels = [rng.uniform(-1, 1, (L // cfg.hop_length + 1, cfg.n_mels)).astype(np.float32) for L in lengths]
    zs = [np.clip(rng.logistic(0, 1, (L, 1)), -20, 20).astype(np.float32) for L in lengths]
    return mels, zs, [torch.from_numpy(m).to(gpu) for m in mels], [torch.from_numpy(z).to(gpu) for z in zs]


@pytest.mark.parametrize('precision', PRECS)
@pytest.mark.parametrize('hop,lengths', [(2, [70, 34, 100]), (16, [48, 32, 112]), (48, [144, 48, 240])])
def test_packed_batch(gpu, persist_knobs, monkeypatch, hop, lengths, precision):
    """generate_varlen with mixed lengths (every utterance >= 32 samples; utterances end inside units): every flow is one packed
    persistent launch with the hop's geometry, every piece equals its own single forward bit for bit and meets the oracle."""
    engine = persist_knobs
    cfg = hop_cfg(hop)
    model, w = _model(gpu, cfg, precision)
    mels, zs, mel_t, z_t = _packed_inputs(cfg, lengths, gpu, seed=hop)
    monkeypatch.setattr(engine, 'VARLEN_PADDED', 0)
    out, log, seen = _logged(engine, lambda: model.generate_varlen(mel_t, z=z_t, verify=False))
    model.verify()
    assert engine.VARLEN_PADDED == 0 and [e[0] for e in log] == ['persist'] * cfg.n_iaf
    assert all(a['packed'] and a['N'] == len(lengths) and a['hop'] == hop and a['offset'] == hop // 2 for a in seen) and len(seen) == cfg.n_iaf
    for L, m, z, mt, zt, piece in zip(lengths, mels, zs, mel_t, z_t, out):
        assert torch.equal(piece, _one_shot(model, hop, mt, zt)), L
        want = O.iaf_vocoder_forward(w, m[None], z[None], cfg)[0]
        err = float(np.abs(piece.cpu().numpy() - want).max())
        assert err <= TOL_F32 * max(1.0, float(np.abs(want).max())), (L, err)


@pytest.mark.parametrize('precision', PRECS)
@pytest.mark.parametrize('hop,lengths', [(2, [70, 30, 100]), (16, [48, 16, 80])])
def test_packed_batch_with_an_utterance_under_32_samples(gpu, persist_knobs, monkeypatch, hop, lengths, precision):
    """What hop 80 cannot build: an utterance below _lib.VARLEN_MIN_ROWS.  Every flow takes the padded fallback, for exactly that
    reason, and the bits are the single forwards'."""
    engine = persist_knobs
    cfg = hop_cfg(hop)
    model, w = _model(gpu, cfg, precision)
    mels, zs, mel_t, z_t = _packed_inputs(cfg, lengths, gpu, seed=100 + hop)
    why, real = [], engine.varlen_fallback_reason

    def spy(*a, **k):
        why.append(real(*a, **k))
        return why[-1]
    monkeypatch.setattr(engine, 'varlen_fallback_reason', spy)
    monkeypatch.setattr(engine, 'VARLEN_PADDED', 0)
    monkeypatch.setattr(engine, 'VARLEN_PADDED_WHY', None)
    out, log, seen = _logged(engine, lambda: model.generate_varlen(mel_t, z=z_t, verify=False))
    model.verify()
    assert why == ['an utterance shorter than 32 samples'] * cfg.n_iaf
    assert engine.VARLEN_PADDED == cfg.n_iaf and engine.VARLEN_PADDED_WHY == 'an utterance shorter than 32 samples'
    assert not any(a['packed'] for a in seen)          # (the padded batch runs the flows' ordinary launches)
    for L, m, z, mt, zt, piece in zip(lengths, mels, zs, mel_t, z_t, out):
        assert tuple(piece.shape) == (L, 1) and torch.equal(piece, _one_shot(model, hop, mt, zt)), L
        want = O.iaf_vocoder_forward(w, m[None], z[None], cfg)[0]
        assert float(np.abs(piece.cpu().numpy() - want).max()) <= TOL_F32 * max(1.0, float(np.abs(want).max())), L


@pytest.mark.parametrize('precision', PRECS)
@pytest.mark.parametrize('hop,filler,rows,lengths', [(16, 32, 208, [48, 64]), (48, 48, 624, [144, 96])])
def test_packed_graph_replay(gpu, persist_knobs, hop, filler, rows, lengths, precision):
    """graph.GraphedPackedVocoder at 4 slots: the filler utterance is 32 rows at hop 16 (two hops) and one hop at hop 48; a replay
    with two utterances (two filler slots) equals the eager packed forward bit for bit; lengths under 32 or off the hop are refused."""
    from pwv_amd.graph import GraphedPackedVocoder
    engine = persist_knobs
    cfg = hop_cfg(hop)
    model, _ = _model(gpu, cfg, precision)
    g = GraphedPackedVocoder(model, 4, rows)
    assert g.filler == filler and g.captures == 1
    assert g._layout(lengths) == lengths + [filler, rows - sum(lengths) - filler]
    _, _, mel_t, _ = _packed_inputs(cfg, lengths, gpu, seed=7)
    seeds, offsets = [2 ** 63 + 5, 11], [0, 12345]
    out = g(mel_t, seeds, offsets)
    g.verify()
    got = [o.clone() for o in out]
    assert g.eager_calls == 0 and g.captures == 1
    want = model.generate_varlen(mel_t, seeds=seeds, offsets=offsets)
    for a, b, L in zip(got, want, lengths):
        assert tuple(a.shape) == (L, 1) and torch.equal(a, b), L
    for bad in ([hop] if hop < 32 else []) + [hop + hop // 2, 40]:
        assert not g.fits([bad])
        with pytest.raises(ValueError, match='multiples of hop_length'):
            g._layout([bad])
    with pytest.raises(ValueError, match='multiple of %d' % hop):
        GraphedPackedVocoder(model, 4, rows + 1)
    with pytest.raises(ValueError, match='at least %d' % (4 * filler)):
        GraphedPackedVocoder(model, 4, 4 * filler - hop)


# ---- 5. streaming ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('route', ['auto', 'per_layer'])
@pytest.mark.parametrize('precision', PRECS)
@pytest.mark.parametrize('hop,schedule', [(16, [1] * 12), (16, [3, 1, 2, 5, 1]), (48, [1] * 8), (48, [2, 1, 4, 1])],
                         ids=['hop16_one_frame', 'hop16_ragged', 'hop48_one_frame', 'hop48_ragged'])
def test_stream_pushes_concatenate_to_the_one_shot_forward(gpu, knobs, hop, schedule, precision, route):
    """Three sessions advanced together, `schedule` frames per push, on the wide small model: at hop 16 a one-frame push is 16 rows per
    session -- below the 32-row unit (three sessions share two units: the per-lane division of unit_rows) and below most dilations.
    Every push is one persistent streaming launch per flow (route 'auto') or the per-layer streaming launches (PERSIST = False); the
    pieces concatenate to each session's own one-shot forward bit for bit, and session 0 meets the oracle."""
    cfg = _wide_cfg(hop)
    n, L = 3, sum(schedule) * hop
    model, w = _model(gpu, cfg, precision)
    ins = [_inputs(cfg, L, gpu, seed=60 + i) for i in range(n)]
    mel, z = torch.stack([u[2] for u in ins]), torch.stack([u[3] for u in ins])
    default = knobs.PERSIST
    if route == 'per_layer':
        knobs.PERSIST = False
    s = model.open_stream(slots=n)
    outs, f0, e = [], 1, 0
    with _Log(knobs) as lg:
        assert tuple(s.push(mel[:, :1], z=z[:, :0]).shape) == (n, 0, 1)
        for f in schedule:
            outs.append(s.push(mel[:, f0:f0 + f], z=z[:, e:e + f * hop], verify=False))
            s.verify()
            f0, e = f0 + f, e + f * hop
    if route == 'auto':
        lg.check(cfg, [n * f * hop for f in schedule], gpu)
    else:
        assert [ev[0] for ev in lg.log] == ['layer_stream'] * (cfg.n_iaf * len(schedule))
    knobs.PERSIST = default
    got = torch.cat(outs, dim=1)
    assert [s.emitted(i) for i in range(n)] == [L] * n
    for i in range(n):
        want = _one_shot(model, hop, ins[i][2], ins[i][3])
        assert torch.equal(got[i], want), (i, float((got[i] - want).abs().max()))
    want = O.iaf_vocoder_forward(w, ins[0][0][None], ins[0][1][None], cfg)[0]
    err = float(np.abs(got[0].cpu().numpy() - want).max())
    assert err <= TOL_F32 * max(1.0, float(np.abs(want).max())), err


@pytest.mark.parametrize('precision', PRECS)
def test_ragged_tick_with_a_session_under_32_rows_takes_the_grouped_route(gpu, knobs, precision):
    """push_varlen at hop 16, PERSIST at its default.  Tick 0 starts three sessions (48, 32 and 0 samples), tick 1 gives session 0 ONE
    frame -- 16 rows, below _lib.VARLEN_MIN_ROWS -- next to 80 and 48 rows, tick 2 gives 32, 32 and 64.  Ticks 0 and 2 are packed launches;
    tick 1 must take the grouped route, for exactly that reason, with one group per length.  Every piece equals the same chunk pushed to
    a stream of its own, and every session its one-shot forward."""
    hop = 16
    assert knobs.PERSIST is not False
    cfg = hop_cfg(hop)
    model, _ = _model(gpu, cfg, precision)
    ticks = [{0: 4, 1: 3, 2: 1}, {0: 1, 1: 5, 2: 3}, {0: 2, 1: 2, 2: 4}]
    frames = {sl: sum(t[sl] for t in ticks) for sl in range(3)}
    ins = {sl: _inputs(cfg, (frames[sl] - 1) * hop, gpu, seed=80 + sl) for sl in range(3)}
    s = model.open_stream(slots=3)
    alone = {sl: model.open_stream(slots=1) for sl in range(3)}
    fpos, pieces, routes = {sl: 0 for sl in range(3)}, {sl: [] for sl in range(3)}, []
    for t in ticks:
        mels = [ins[sl][2][fpos[sl]:fpos[sl] + t[sl]] for sl in range(3)]
        T = [(t[sl] - (1 if fpos[sl] == 0 else 0)) * hop for sl in range(3)]
        zs = [ins[sl][3][s.emitted(sl):s.emitted(sl) + T[sl]] for sl in range(3)]
        with _Log(knobs) as lg:
            got = s.push_varlen(mels, z=zs, verify=False)
            s.verify()
        routes.append([ev[3:] for ev in lg.log if ev[0] == 'stream_ragged'])
        for sl in range(3):
            assert tuple(got[sl].shape) == (T[sl], 1)
            own = alone[sl].push(mels[sl][None], z=zs[sl][None])[0]
            assert torch.equal(got[sl], own), (sl, T[sl])
            pieces[sl].append(got[sl])
            fpos[sl] += t[sl]
    assert routes[0] == [('packed', None, 1)] * cfg.n_iaf and routes[2] == [('packed', None, 1)] * cfg.n_iaf, routes
    assert routes[1] == [('grouped', 'an utterance shorter than 32 samples', 3)] * cfg.n_iaf, routes[1]
    for sl in range(3):
        want = _one_shot(model, hop, ins[sl][2], ins[sl][3])
        assert torch.equal(torch.cat(pieces[sl]), want), sl


def _mid_utterance(s, rng, gpu, hop):
    """Every slot of `s` running, as load_state leaves it: a random kept frame, some samples emitted."""
    for sl in range(s.n_slots):
        st = s.state(sl)
        st['kept'] = torch.from_numpy(rng.uniform(-1, 1, (s.n_mels,)).astype(np.float32)).to(gpu)
        st['running'], st['emitted'] = True, hop * (3 + sl)
        s.load_state(sl, st)


@pytest.mark.parametrize('precision', PRECS)
@pytest.mark.parametrize('hop,n,frames', [(16, 3, 1), (16, 2, 3), (48, 2, 2)], ids=['hop16_3x16', 'hop16_2x48', 'hop48_2x96'])
def test_graphed_tick_against_push(gpu, knobs, hop, n, frames, precision):
    """s.graphed(n, frames) captures at these hops -- a tick of 16 rows per session included -- and one tick equals one eager push from
    the same random histories: outputs, every history block of both generations, kept frames, emitted counts."""
    cfg = _wide_cfg(hop)
    model, _ = _model(gpu, cfg, precision)
    T = frames * hop
    rng = np.random.default_rng(hop + frames)
    mel = torch.from_numpy(rng.uniform(-1, 1, (n, frames, cfg.n_mels)).astype(np.float32)).to(gpu)
    z = torch.from_numpy(np.clip(rng.logistic(0, 1, (n, T, 1)), -20, 20).astype(np.float32)).to(gpu)
    res = []
    for graphed in (True, False):
        s = model.open_stream(slots=n)
        if graphed:
            with _Log(knobs) as lg:
                g = s.graphed(n, frames, sample=False)
            lg.check(cfg, [n * T] * 2, gpu)          # the warm-up ticks: one persistent streaming launch per flow
            assert g.captures == 1 and g.eager_calls == 0
        _mid_utterance(s, np.random.default_rng(5), gpu, hop)
        _random_state(s, 100 + frames)
        if graphed:
            out = g.tick(mel, list(range(n)), z=z).clone()
            assert g.verify() == 1 and g.eager_calls == 0
        else:
            out = s.push(mel, z=z)
        res.append((out, s._hist.clone(), s._kept.clone(), [s.emitted(sl) for sl in range(n)], list(s._gen)))
    (out_g, hist_g, kept_g, em_g, gen_g), (out_p, hist_p, kept_p, em_p, gen_p) = res
    assert tuple(out_g.shape) == (n, T, 1) and bool(torch.isfinite(out_g).all())
    assert torch.equal(out_g, out_p), float((out_g - out_p).abs().max())
    assert torch.equal(hist_g, hist_p), int((hist_g != hist_p).sum())
    assert torch.equal(kept_g, kept_p) and em_g == em_p == [hop * (3 + sl) + T for sl in range(n)] and gen_g == gen_p


# ---- 6. one case each at hop 48 --------------------------------------------------------------------------------------------------------
def test_f16_storage_mode_at_hop_48(gpu):
    """precision 'f16' (csrc/pwv_layer_h16.hip has its own division site) against the fp64 oracle at the mode's own stated bars
    (tests/test_gpu_f16.py: 5e-3 max, 1e-3 rms on O(1) outputs); bitwise repeatable."""
    from tests.test_gpu_f16 import TOL_F16, TOL_F16_RMS
    cfg, w, mel, z, want = _case(48)
    a = run_vocoder_hip(cfg, w, mel, z, gpu, precision='f16')
    b = run_vocoder_hip(cfg, w, mel, z, gpu, precision='f16')
    d = a - want
    print('f16 at hop 48: max %.3g rms %.3g' % (np.abs(d).max(), np.sqrt((d ** 2).mean())))
    assert np.array_equal(a, b) and a.shape == want.shape
    assert np.abs(d).max() <= TOL_F16 and np.sqrt((d ** 2).mean()) <= TOL_F16_RMS


@pytest.mark.parametrize('precision', PRECS)
def test_time_shards_at_hop_48(gpu, precision):
    """Three time shards (overlap-and-discard with the chain's halo: 80 samples of look-back -> 96 = two hops) equal the unsharded forward
    bit for bit; a halo one hop short does not."""
    from pwv_amd.models import IAFVocoder
    from pwv_amd.timeshard import chain_halo, generate_time_sharded, shard_plan, vocoder_forward_factory
    hop, L = 48, 48 * 30
    cfg = hop_cfg(hop)
    model, _ = _model(gpu, cfg, precision)
    _, _, mel_t, z_t = _inputs(cfg, L, gpu, seed=9)
    want = IAFVocoder(1, L, store=model.store, precision=precision)(None, mel_t[None], is_training=False, z=z_t[None]).clone()
    halo = chain_halo(cfg.dilations, cfg.filter_width, cfg.n_iaf, hop)
    assert halo == 96 and [a - c for c, a, _ in shard_plan(L, 3, halo, hop)] == [0, 96, 96]
    fwd = vocoder_forward_factory(model.store, precision=precision)
    got = generate_time_sharded(fwd, mel_t[None], z_t[None], hop, halo, n_shards=3)
    assert torch.equal(got, want)
    assert not torch.equal(generate_time_sharded(fwd, mel_t[None], z_t[None], hop, halo - hop, n_shards=3), want)


# ---- 7. odd hops -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('method', ['repeat', 'none'])
@pytest.mark.parametrize('hop', [1, 81])
def test_an_odd_hop_is_refused_before_any_launch(gpu, monkeypatch, hop, method):
    """The reference crops [hop // 2 : -(hop // 2)] (models.py:124,133): hop + 1 samples per frame step of an odd hop, nothing of hop 1 --
    it has no answer there, so IAFVocoder refuses with a ValueError that says so, before anything is enqueued.  (RepeatedCondition and
    the C ABI stay general: test_layer_level_any_hop_and_offset.)"""
    from pwv_amd import engine
    from pwv_amd.models import IAFVocoder
    from pwv_amd.variables import VariableStore
    cfg = small_cfg(hop_length=hop, cond_upsample_method=method)
    set_hparams(cfg)
    store = VariableStore(device=gpu)
    store.load_dict(O.init_weights(cfg, seed=2))
    calls, real = [], engine.check

    def spy(code, what=''):
        calls.append(what)
        return real(code, what)
    monkeypatch.setattr(engine, 'check', spy)
    model = IAFVocoder(2, 2 * hop, store=store)
    with pytest.raises(ValueError, match=r'hop_length \(%d\) must be even.*models\.py:124,133' % hop):
        model(None, torch.zeros(2, 3, 80, device=gpu), False, z=torch.zeros(2, 2 * hop, 1, device=gpu))
    assert calls == []
