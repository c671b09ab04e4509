"""GPU: the training gradients at batch shapes other than the 416 rows of tests/test_gpu_train.py and tests/test_gpu_train_varlen.py:
row counts that leave the last 32-row unit partly filled, hop lengths from 2 to 256 (one to nine dP slots per P row, a frame larger than
a unit), N = 1, 3 and 5, utterances shorter than a unit, a look-ahead with a V that is not zero, and the front backward on its own.
Kernel level through the C ABI (layer backward in both forms, the look-ahead, the front backward, uniform and packed) and model level
(loss_and_grad, loss_and_grad_varlen: all 149 gradients, partials, repetition, guarded buffers, one optimiser step).

Bars as in tests/test_gpu_train.py, unchanged: err = max|g - g64| / max|g64| per output or variable against float64 on the CPU
(tests/train_oracle.py, tests/train_varlen_oracle.py), E32 = the largest err of the same function evaluated in float32 on the CPU
(autograd; for the front backward the float32 numpy restatement), computed at run time per case, and the kernels must stay within
MARGIN = 8 times E32.  An output whose float64 gradient is identically zero must be exact zeros.  No launch is on more than 720 rows.
Measured maxima are in DESIGN.md section 9, "Training" and "Packed training"."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import test_gpu_train as GT
from tests import test_gpu_train_varlen as GV
from tests import train_oracle as TO
from tests import train_varlen_oracle as VO
from tests.guarded import guarded
from tests.util import TOL_F32, set_hparams

pytestmark = pytest.mark.gpu

MARGIN = GT.MARGIN
_dev = GT._dev

# (N, T, hop, offset) of the uniform layer cases                  rows = units    what the case reaches
LAYER_SHAPES = [
    (3, 208, 16, 8),            # 624 = 19.5    a partial last unit; one utterance boundary on a unit edge, one inside a unit
    (2, 200, 80, 40),           # 400 = 12.5    four dP slots, a frame larger than a unit, a partial last unit
    (3, 80, 80, 40),            # 240 = 7.5     utterances of two 40-row frames
    (2, 100, 7, 3),             # 200 = 6.25    an odd hop that does not divide T; five or six frames per unit
    (2, 72, 2, 1),              # 144 = 4.5     16 frames per unit: the flush loop of dP at its densest
    (3, 48, 32, 31),            # 144 = 4.5     hop = the unit size, the offset at its extreme
    (1, 300, 256, 128),         # 300 = 9.4     nine dP slots; N = 1
    (1, 16, 16, 8),             # 16 = 0.5      one partial unit, a grid of one workgroup
]
# (shape, d, max_workgroups): d in {1, 48} everywhere; d = 256 >= T and 1, 3 partials at the first two
LAYER_CASES = ([(s, d, 0) for s in LAYER_SHAPES for d in (1, 48)] + [(s, 256, 0) for s in LAYER_SHAPES[:2]]
               + [(s, d, m) for s in LAYER_SHAPES[:2] for d in (1, 48) for m in (1, 3)])
LOOK_AHEAD_SHAPES = [LAYER_SHAPES[0], LAYER_SHAPES[1], LAYER_SHAPES[7]]
FRONT_SHAPES = [(3, 208), (2, 200), (5, 16), (1, 16)]
# (lengths, hop, dilations) of the packed layer cases
PACKED_CASES = [
    ((208, 16, 48, 128), 16, (1, 48)),                  # 400 rows = 12.5 units
    ((240, 80, 80), 80, (1, 48)),                       # 400 rows; four dP slots
    ((40, 8, 8, 24, 16, 8), 8, (1, 3)),                 # 104 rows = 3.25 units; four utterances in a unit
    ((16,), 16, (1, 48)),                               # one utterance of half a unit
]
MODEL_SHAPES = [(3, 208, 16), (3, 240, 80), (5, 16, 16), (1, 16, 16), (2, 200, 40)]
PACKED_MODELS = [((208, 16, 48, 128), 16), ((240, 80, 80), 80), ((16,), 16)]
_id = lambda v: '-'.join(str(e) for e in v) if isinstance(v, tuple) else str(v)


@pytest.fixture(autouse=True)
def _default_hparams_afterwards():
    yield
    from pwv_amd.hparam import hparam as hp
    hp.set_hparam_yaml('default')


def _check_outputs(got, g64, e32, what):
    """Every output of `g64` within MARGIN e32 of it, exact zeros where it is identically zero; returns the worst err."""
    worst = 0.0
    for k, want in g64.items():
        assert got[k].shape == want.shape and np.isfinite(got[k]).all(), (what, k)
        if np.abs(want).max() == 0:
            assert np.abs(got[k]).max() == 0, (what, k)
            continue
        err = TO.rel_err(got[k], want)
        worst = max(worst, err)
        print('%s %s err %.3g (E32 %.3g)' % (what, k, err, e32))
        assert err <= MARGIN * e32, (what, k, err, e32)
    return worst


def _e32(g32, g64):
    return max(TO.rel_err(g32[k], g64[k]) for k in g64 if np.abs(g64[k]).max() > 0)


# ---- the uniform layer backward -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _layer_reference(shape, d, last):
    N, T, hop, offset = shape
    c = TO.layer_case(d, hop=hop, N=N, T=T, offset=offset)
    g64, g32 = TO.layer_grads(c, last, torch.float64), TO.layer_grads(c, last, torch.float32)
    return c, g64, _e32(g32, g64)


@pytest.mark.parametrize('last', [False, True], ids=['residual', 'last_head'])
@pytest.mark.parametrize('shape, d, max_workgroups', LAYER_CASES, ids=['%s-d%d-wg%d' % (_id(s), d, m) for s, d, m in LAYER_CASES])
def test_layer_backward_at_ragged_shapes(gpu, shape, d, max_workgroups, last):
    """Every output of the layer backward (x, P, filter, gate, and dense, dense_bias or the head's six) against float64 autograd of that
    layer at the shapes of LAYER_SHAPES, within 8 x the error of float32 autograd of the same layer."""
    c, g64, e32 = _layer_reference(shape, d, last)
    assert c['frames'] == (shape[1] - 1 + shape[3]) // shape[2] + 1 and shape[0] * shape[1] <= 720
    got = GT._layer_backward(c, last, gpu, max_workgroups=max_workgroups)
    _check_outputs(got, g64, e32, '%s d=%d wg=%d %s' % (_id(shape), d, max_workgroups, 'last' if last else 'residual'))
    if d >= shape[1]:       # no row has a look-back: the tap at t - d sees zeros only
        assert np.abs(got['filter'][0]).max() == 0 and np.abs(got['gate'][0]).max() == 0
        assert np.abs(g64['filter'][0]).max() == 0 and np.abs(g64['gate'][0]).max() == 0


@pytest.mark.parametrize('dn', [3, 48])
@pytest.mark.parametrize('shape', LOOK_AHEAD_SHAPES, ids=_id)
def test_layer_backward_gathers_the_look_ahead(gpu, shape, dn):
    """The residual form with a random U and a random V that is not zero, gathered with next_dilation 3 and 48: the gradient that
    arrives is g[t] = U[t] + V[t + dn] inside the utterance (float64), and every output follows it.  At dn >= T nothing is added: the
    result is the bits of the run with V = 0."""
    N, T, hop, offset = shape
    for d in (1, 48):
        c = TO.layer_case(d, hop=hop, N=N, T=T, offset=offset)
        V = np.random.RandomState(70 + dn + d).randn(N, T, 64).astype(np.float32)
        assert np.abs(V).min() > 0
        cu = [n * T for n in range(N + 1)]
        g = TO.look_ahead(c['g'].reshape(N * T, 64).astype(np.float64), V.reshape(N * T, 64).astype(np.float64), dn, cu).reshape(N, T, 64)
        g64, g32 = TO.layer_grads(c, False, torch.float64, g=g), TO.layer_grads(c, False, torch.float32, g=g)
        got = GT._layer_backward(c, False, gpu, next_dilation=dn, v_next=V)
        _check_outputs(got, g64, _e32(g32, g64), '%s d=%d dn=%d' % (_id(shape), d, dn))
        if dn >= T:
            assert np.array_equal(g, c['g'].astype(np.float64))
            plain = GT._layer_backward(c, False, gpu, next_dilation=dn)
            for k in g64:
                assert np.array_equal(got[k], plain[k]), k
        else:
            assert not np.array_equal(g, c['g'].astype(np.float64))


# ---- the front backward ---------------------------------------------------------------------------------------------------------------
def _front_backward(c, base, device, packed=False, hop=16, max_workgroups=0):
    """One pwv_train_front_bwd_f32 (packed: pwv_train_varlen_front_bwd_f32) on the case `c`; the workspace and the outputs start as NaN,
    d_in inside an allocation of rows + 32 floats.  Returns ({'cf', 'd_in'} float64 numpy, the 32 floats behind d_in)."""
    from pwv_amd import _lib
    lib = _lib.lib()
    lengths, rows = c['lengths'], len(c['in'])
    assert rows <= 720
    nan = lambda *shape: torch.full(shape, float('nan'), dtype=torch.float32, device=device)
    t = {k: _dev(c[k], device) for k in ('in', 'cf', 'd_out', 'scale')}
    u, v = _dev(TO.to_tile32(c['U']), device), _dev(TO.to_tile32(c['V']), device)
    d_in, d_cf = nan(rows + 32), nan(2, 1, 64)
    if base == 'accumulate':
        d_in[:rows] = _dev(c['d_in0'], device)
    ptr = lambda a: a.data_ptr()
    flat = _lib.TrainArgs(N=1, T=rows, max_workgroups=max_workgroups)
    ws = nan(lib.pwv_train_workspace_bytes(ctypes.byref(flat)) // 4)
    assert ws.numel() > 0
    kw = dict(max_workgroups=max_workgroups, dilation=1, next_dilation=c['dn'], accumulate=int(base == 'accumulate'), in_=ptr(t['in']),
              causal_filter=ptr(t['cf']), u_next=ptr(u), v_next=ptr(v), d_in=ptr(d_in), d_causal_filter=ptr(d_cf), workspace=ptr(ws),
              workspace_bytes=ws.numel() * 4)
    if base == 'affine':
        kw.update(d_out=ptr(t['d_out']), scale=ptr(t['scale']))
    stream = torch.cuda.current_stream().cuda_stream
    if packed:
        frames = [1 + T // hop for T in lengths]
        cu_r = _dev(np.asarray(c['cu_rows'], dtype=np.int32), device)
        cu_f = _dev(np.asarray([0] + list(np.cumsum(frames)), dtype=np.int32), device)
        a = _lib.TrainVarlenArgs(cond_hop=hop, cond_offset=hop // 2, proj_row_stride=128, d_proj_row_stride=128, cu_rows=ptr(cu_r),
                                 cu_frames=ptr(cu_f), n=len(lengths), rows=rows, proj_rows=sum(frames), **kw)
        _lib.check(lib.pwv_train_varlen_front_bwd_f32(ctypes.byref(a), stream), 'varlen front_bwd')
    else:
        assert len(set(lengths)) == 1
        a = _lib.TrainArgs(N=len(lengths), T=lengths[0], cond_hop=hop, cond_offset=hop // 2, cond_frames=1 + lengths[0] // hop, proj_row_stride=128,
                           d_proj_row_stride=128, **kw)
        _lib.check(lib.pwv_train_front_bwd_f32(ctypes.byref(a), stream), 'front_bwd')
    torch.cuda.synchronize()
    out = d_in.cpu().numpy()
    return {'cf': d_cf.cpu().numpy().astype(np.float64), 'd_in': out[:rows].astype(np.float64)}, out[rows:]


def _check_front(c, device, packed, what):
    worst = 0.0
    for base in TO.FRONT_BASES:
        g64, g32 = TO.front_backward(c, base, np.float64), TO.front_backward(c, base, np.float32)
        got, behind = _front_backward(c, base, device, packed=packed)
        worst = max(worst, _check_outputs(got, g64, _e32(g32, g64), '%s %s' % (what, base)))
        assert len(behind) == 32 and np.isnan(behind).all(), (what, base)        # d_in has exactly `rows` elements
    return worst


@pytest.mark.parametrize('dn', [1, 3])
@pytest.mark.parametrize('shape', FRONT_SHAPES, ids=_id)
def test_front_backward_matches_float64(gpu, shape, dn):
    """d_causal_filter and d_in of pwv_train_front_bwd_f32 against the float64 restatement (tests.train_oracle.front_backward, pinned
    by autograd on the CPU), d_in starting from nothing, from d_out * scale and from what it held; within 8 x the error of the float32
    restatement, and the 32 floats behind d_in stay NaN."""
    N, T = shape
    _check_front(TO.front_case([T] * N, dn), gpu, False, 'front %s dn=%d' % (_id(shape), dn))


@pytest.mark.parametrize('dn', [1, 3])
@pytest.mark.parametrize('lengths, hop', [c[:2] for c in PACKED_CASES[:2]], ids=[_id(c[0]) for c in PACKED_CASES[:2]])
def test_packed_front_backward_matches_float64(gpu, lengths, hop, dn):
    """pwv_train_varlen_front_bwd_f32 on the first two packed cases, the three ways d_in starts."""
    c = TO.front_case(list(lengths), dn)
    _check_front(c, gpu, True, 'packed front %s dn=%d' % (_id(lengths), dn))


# ---- the packed layer backward --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _packed_layer_reference(lengths, hop, d, last):
    c = VO.layer_case(d, lengths=lengths, hop=hop)
    g64, g32 = VO.layer_grads(c, last, torch.float64), VO.layer_grads(c, last, torch.float32)
    return c, g64, _e32(g32, g64)


@pytest.mark.parametrize('last', [False, True], ids=['residual', 'last_head'])
@pytest.mark.parametrize('lengths, hop, dilations', PACKED_CASES, ids=[_id(c[0]) for c in PACKED_CASES])
def test_packed_layer_backward_at_ragged_shapes(gpu, lengths, hop, dilations, last):
    """Every output of the packed layer backward against float64 autograd of the layer run utterance by utterance, at row counts that
    are no whole number of units."""
    assert sum(lengths) % 32 and sum(lengths) <= 720
    for d in dilations:
        c, g64, e32 = _packed_layer_reference(lengths, hop, d, last)
        got = GV._layer_backward(c, last, gpu)
        _check_outputs(got, g64, e32, 'packed %s d=%d %s' % (_id(lengths), d, 'last' if last else 'residual'))


# ---- the whole model ------------------------------------------------------------------------------------------------------------------
def _store(w, device):
    from pwv_amd.variables import VariableStore
    store = VariableStore(device=device)
    store.load_dict(w)
    return store


def _model(device, shape):
    from pwv_amd.models import IAFVocoder
    N, T, hop = shape
    assert N * T <= 720
    cfg, w, mel, z, wav = TO.problem(N, T, hop)
    set_hparams(cfg)
    return IAFVocoder(batch_size=N, length=T, store=_store(w, device), precision='f32'), _dev(wav, device), _dev(mel, device), _dev(z, device)


def _packed_model(device, lengths, hop):
    from pwv_amd.models import IAFVocoder
    assert sum(lengths) <= 720
    cfg, w, mels, zs, wavs = VO.problem(lengths, hop)
    set_hparams(cfg)
    model = IAFVocoder(batch_size=1, length=max(lengths), store=_store(w, device), precision='f32')
    return model, [_dev(a[0, :, 0], device) for a in wavs], [_dev(a[0], device) for a in mels], [_dev(a[0], device) for a in zs]


def _check_grads(grads, ref, what):
    """All 149 gradients within MARGIN E32 of float64 autograd, exact zeros for the 32 variables the model never reads."""
    g64, bar = ref['g64'], MARGIN * ref['E32']
    assert sorted(grads) == sorted(g64)
    worst, zeros = 0.0, 0
    for k, want in g64.items():
        got = grads[k].detach().cpu().numpy().astype(np.float64)
        if want is None:
            assert got.shape == TO.problem()[1][k].shape and np.abs(got).max() == 0, (what, k)
            zeros += 1
            continue
        assert got.shape == want.shape and np.isfinite(got).all(), (what, k)
        err = TO.rel_err(got, want)
        worst = max(worst, err)
        assert err <= bar, (what, k, err, bar)
    print('%s worst gradient err %.3g (E32 %.3g, bar %.3g)' % (what, worst, ref['E32'], bar))
    assert zeros == 32 and len(g64) - zeros == 149
    return worst


def _check_uniform(run, ref, shape, what):
    loss, pred, grads = run
    assert tuple(pred.shape) == (shape[0], shape[1], 1) and loss.dim() == 0 and loss.is_cuda
    _check_grads(grads, ref, what)
    assert abs(float(loss) - ref['loss']) <= 2e-6 * max(1.0, abs(ref['loss']))
    assert np.abs(pred.detach().cpu().numpy().astype(np.float64) - ref['pred']).max() <= TOL_F32


def _check_packed(run, ref, lengths, what):
    loss, preds, grads = run
    assert loss.dim() == 0 and loss.is_cuda and [tuple(p.shape) for p in preds] == [(T, 1) for T in lengths]
    _check_grads(grads, ref, what)
    assert abs(float(loss) - ref['terms']['total']) <= 2e-6 * max(1.0, abs(ref['terms']['total']))
    for p, want in zip(preds, ref['preds']):
        assert np.abs(p.detach().cpu().numpy().astype(np.float64).reshape(-1) - want).max() <= TOL_F32


def _same(a, b):
    preds = lambda r: r[1] if isinstance(r[1], (list, tuple)) else [r[1]]
    assert torch.equal(a[0], b[0]) and all(torch.equal(p, q) for p, q in zip(preds(a), preds(b)))
    assert sorted(a[2]) == sorted(b[2])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k


@pytest.mark.parametrize('shape', MODEL_SHAPES, ids=_id)
def test_model_gradients_at_ragged_shapes(gpu, shape):
    """All 149 gradients, the loss and pred of the small model against float64 autograd at N x T x hop = 3 x 208 x 16 (19.5 units),
    3 x 240 x 80 (22.5 units, four dP slots), 5 x 16 x 16 and 1 x 16 x 16 (utterances of half a unit) and 2 x 200 x 40 (12.5 units)."""
    from pwv_amd import train as TR
    model, wav, mel, z = _model(gpu, shape)
    run = TR.loss_and_grad(model, wav, mel, z=z)
    torch.cuda.synchronize()
    _check_uniform(run, TO.reference(*shape), shape, 'uniform %s' % _id(shape))


@pytest.mark.parametrize('lengths, hop', PACKED_MODELS, ids=[_id(c[0]) for c in PACKED_MODELS])
def test_packed_model_gradients_at_ragged_shapes(gpu, lengths, hop):
    """The same on packed batches of 400, 400 (hop 80) and 16 rows against float64 autograd of the utterances run one by one."""
    from pwv_amd import train as TR
    model, wavs, mels, zs = _packed_model(gpu, lengths, hop)
    run = TR.loss_and_grad_varlen(model, wavs, mels, z=zs)
    torch.cuda.synchronize()
    _check_packed(run, VO.reference(lengths=lengths, hop=hop), lengths, 'packed %s' % _id(lengths))


def test_three_equal_lengths_give_the_bits_of_the_uniform_batch(gpu):
    """[208, 208, 208] packed at hop 16 = the uniform 3 x 208 call, bit for bit: the loss, every pred, every gradient ("Packed
    training"), at 624 rows = 19.5 units."""
    from pwv_amd import train as TR
    shape = (3, 208, 16)
    model, wav, mel, z = _model(gpu, shape)
    a = TR.loss_and_grad(model, wav, mel, z=z)
    b = TR.loss_and_grad_varlen(model, [wav[i, :, 0] for i in range(3)], [mel[i] for i in range(3)], z=[z[i] for i in range(3)])
    torch.cuda.synchronize()
    _same((a[0], [a[1][i] for i in range(3)], a[2]), b)
    _check_uniform(a, TO.reference(*shape), shape, 'uniform 3 x 208 = packed')


@pytest.mark.parametrize('max_workgroups', [1, 3, 0])
def test_partials_and_repetition_uniform(gpu, max_workgroups):
    """3 x 208 with 1, 3 and the default number of partials: each holds the bar and is bit-identical to its repetition."""
    from pwv_amd import train as TR
    shape = (3, 208, 16)
    model, wav, mel, z = _model(gpu, shape)
    runs = []
    for _ in range(2):
        runs.append(TR.loss_and_grad(model, wav, mel, z=z, max_workgroups=max_workgroups))
        torch.cuda.synchronize()
    _check_uniform(runs[0], TO.reference(*shape), shape, '3 x 208 max_workgroups=%d' % max_workgroups)
    _same(runs[0], runs[1])


@pytest.mark.parametrize('max_workgroups', [1, 3, 0])
def test_partials_and_repetition_packed(gpu, max_workgroups):
    """[240, 80, 80] at hop 80 with 1, 3 and the default number of partials: each holds the bar and is bit-identical to its repetition."""
    from pwv_amd import train as TR
    lengths, hop = PACKED_MODELS[1]
    model, wavs, mels, zs = _packed_model(gpu, lengths, hop)
    runs = []
    for _ in range(2):
        runs.append(TR.loss_and_grad_varlen(model, wavs, mels, z=zs, max_workgroups=max_workgroups))
        torch.cuda.synchronize()
    _check_packed(runs[0], VO.reference(lengths=lengths, hop=hop), lengths, '[240, 80, 80] max_workgroups=%d' % max_workgroups)
    _same(runs[0], runs[1])


def _check_guarded(g, loss, preds, grads):
    g.check()
    assert any('train.py' in s for s in g.sites())
    assert torch.isfinite(loss).all() and all(torch.isfinite(p).all() for p in preds)
    for k, v in grads.items():
        assert torch.isfinite(v).all(), k


def test_guarded_uniform_hop_80(gpu):
    """3 x 240 at hop 80 inside poisoned, guard-banded buffers: no band is touched -- the [rows] buffers of y, d_out and d_in are what a
    missing tail mask would overrun --, no NaN in the loss, pred or any gradient, and the gradients hold the bar."""
    from pwv_amd import engine
    from pwv_amd import train as TR
    shape = (3, 240, 80)
    with guarded(TR, engine) as g:
        model, wav, mel, z = _model(gpu, shape)
        run = TR.loss_and_grad(model, wav, mel, z=z)
        torch.cuda.synchronize()
        _check_guarded(g, run[0], [run[1]], run[2])
        _check_uniform(run, TO.reference(*shape), shape, 'guarded 3 x 240 hop 80')


def test_guarded_packed_ragged(gpu):
    """[208, 16, 48, 128] inside poisoned, guard-banded buffers, as above."""
    from pwv_amd import engine
    from pwv_amd import train as TR
    lengths, hop = PACKED_MODELS[0]
    with guarded(TR, engine) as g:
        model, wavs, mels, zs = _packed_model(gpu, lengths, hop)
        run = TR.loss_and_grad_varlen(model, wavs, mels, z=zs)
        torch.cuda.synchronize()
        _check_guarded(g, run[0], run[1], run[2])
        _check_packed(run, VO.reference(lengths=lengths, hop=hop), lengths, 'guarded [208, 16, 48, 128]')


def test_one_optimiser_step_at_hop_80(gpu):
    """One Trainer.step on 3 x 240 and one Trainer.step_varlen on [240, 80, 80], both at hop 80: the loss after the step is lower than
    before it and every shadow is finite (the update itself is checked at 416 rows)."""
    from pwv_amd import train as TR
    model, wav, mel, z = _model(gpu, (3, 240, 80))
    tr = TR.Trainer(model, lr=TO.LR, beta2=TO.BETA2, ema_decay=TO.DECAY)
    before = float(tr.step(wav, mel, z=z))
    after = float(TR.loss_and_grad(model, wav, mel, z=z)[0])
    print('uniform: loss %.6f -> %.6f' % (before, after))
    assert tr.steps == 1 and after < before
    assert all(torch.isfinite(v).all() for v in tr.shadows().values()) and len(tr.shadows()) == 181
    model, wavs, mels, zs = _packed_model(gpu, *PACKED_MODELS[1])
    tr = TR.Trainer(model, lr=TO.LR, beta2=TO.BETA2, ema_decay=TO.DECAY)
    before = float(tr.step_varlen(wavs, mels, z=zs))
    after = float(TR.loss_and_grad_varlen(model, wavs, mels, z=zs)[0])
    print('packed: loss %.6f -> %.6f' % (before, after))
    assert tr.steps == 1 and after < before
    assert all(torch.isfinite(v).all() for v in tr.shadows().values()) and len(tr.shadows()) == 181
