"""GPU: training (pwv_amd/train.py -> pwv_train_*, csrc/pwv_train.hip) against float64 autograd on the CPU (tests/train_oracle.py): one
layer through the C ABI at every kind of dilation, the whole small model, the partials of the weight-gradient reductions, guarded
buffers, ten optimiser steps, and `python -m pwv_amd.train` -> `generate`.

The bar of a gradient is not a number fixed here: err(v) = max|g - g64| / max|g64| per variable, E32 = the largest err of float32
autograd on the CPU of the same function, computed at run time (1.8e-6 for the small model), and the kernels must stay within 8 E32: a
different summation order (partials and a tree against a sequential sum) and another tanh / sigmoid each cost a small factor over a
plain float32 evaluation, a wrong term is off by orders of magnitude.  Measured maxima are in DESIGN.md section 9, "Training"."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import train_oracle as TO
from tests.guarded import guarded
from tests.util import TOL_F32, set_hparams

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 8
DILATIONS = (1, 32, 48, 256)            # within a tile, tile-aligned, across tiles, larger than T


# ---- one layer through ctypes ---------------------------------------------------------------------------------------------------------
def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _layer_backward(c, last, device, g=None, max_workgroups=0, next_dilation=1, v_next=None):
    """The layer backward (and, in the last form, the head backward in front of it) on one net, at the shape of the case `c`; returns
    float64 numpy: the input gradient assembled with its look-ahead, dP with its slots added, every weight and bias gradient.  The
    residual form takes the gradient for its output as the layer above would leave it: U = g (default: c['g']) and V = v_next
    [N, T, 64] (default: zeros), gathered with next_dilation."""
    from pwv_amd import _lib
    lib = _lib.lib()
    N, T, d, hop, frames = c['N'], c['T'], c['d'], c['hop'], c['frames']
    rows = N * T
    kmax = (hop + 30) // 32 + 1
    t = {k: _dev(c[k], device) for k in ('P', 'filter', 'gate', 'dense', 'dense_bias', 'skip', 'skip_bias', 'post1', 'post1_bias', 'post2', 'post2_bias', 'dy')}
    x = _dev(TO.to_tile32(c['x'].reshape(rows, 64)), device)
    nan = lambda *shape: torch.full(shape, float('nan'), dtype=torch.float32, device=device)
    tile = lambda: nan(((rows + 31) // 32) * 32 * 64)
    u, v = tile(), tile()
    dP = torch.zeros((N * frames * kmax, 128), dtype=torch.float32, device=device)
    base = dict(N=N, T=T, cond_hop=hop, cond_offset=c['offset'], cond_frames=frames, proj_row_stride=128, d_proj_row_stride=128,
                max_workgroups=max_workgroups, dilation=d, next_dilation=next_dilation)
    ws = nan(lib.pwv_train_workspace_bytes(ctypes.byref(_lib.TrainArgs(**base))) // 4)
    assert ws.numel() > 0
    out = {k: nan(*c[k].shape) for k in (TO.LAYER_LAST if last else TO.LAYER_RESIDUAL) if k not in ('x', 'P')}
    ptr = lambda a: a.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    common = dict(base, x=ptr(x), proj=ptr(t['P']), filter=ptr(t['filter']), gate=ptr(t['gate']), u=ptr(u), v=ptr(v), d_proj=ptr(dP),
                  d_filter=ptr(out['filter']), d_gate=ptr(out['gate']), workspace=ptr(ws), workspace_bytes=ws.numel() * 4)
    if last:
        o, d_o = tile(), tile()
        a = _lib.TrainArgs(form=_lib.TRAIN_LAST, x_out=ptr(o), **{k: val for k, val in common.items() if k in base or k in ('x', 'proj', 'filter', 'gate')})
        _lib.check(lib.pwv_train_layer_fwd_f32(ctypes.byref(a), stream), 'layer_fwd')
        head = dict(skip=ptr(t['skip']), skip_bias=ptr(t['skip_bias']), post1=ptr(t['post1']), post1_bias=ptr(t['post1_bias']), post2=ptr(t['post2']),
                    post2_bias=ptr(t['post2_bias']))
        a = _lib.TrainArgs(x=ptr(o), d_out=ptr(t['dy']), d_o_out=ptr(d_o), d_skip=ptr(out['skip']), d_skip_bias=ptr(out['skip_bias']),
                           d_post1=ptr(out['post1']), d_post1_bias=ptr(out['post1_bias']), d_post2=ptr(out['post2']), d_post2_bias=ptr(out['post2_bias']),
                           workspace=ptr(ws), workspace_bytes=ws.numel() * 4, **base, **head)
        _lib.check(lib.pwv_train_head_bwd_f32(ctypes.byref(a), stream), 'head_bwd')
        a = _lib.TrainArgs(form=_lib.TRAIN_LAST, d_o=ptr(d_o), **common)
    else:
        # the gradient for the layer's output as the layer above would leave it: U = g, V = 0 unless given
        gu = _dev(TO.to_tile32((c['g'] if g is None else g).reshape(rows, 64)), device)
        gv = torch.zeros_like(gu) if v_next is None else _dev(TO.to_tile32(v_next.reshape(rows, 64)), device)
        a = _lib.TrainArgs(form=_lib.TRAIN_RESIDUAL, dense=ptr(t['dense']), u_next=ptr(gu), v_next=ptr(gv), d_dense=ptr(out['dense']),
                           d_dense_bias=ptr(out['dense_bias']), **common)
    _lib.check(lib.pwv_train_layer_bwd_f32(ctypes.byref(a), stream), 'layer_bwd')
    torch.cuda.synchronize()
    U = TO.from_tile32(u.cpu().numpy(), rows, 64).reshape(N, T, 64).astype(np.float64)
    V = TO.from_tile32(v.cpu().numpy(), rows, 64).reshape(N, T, 64).astype(np.float64)
    dx = U.copy()
    if d < T:
        dx[:, :T - d] += V[:, d:]
    res = {k: val.cpu().numpy().astype(np.float64) for k, val in out.items()}
    res['x'] = dx
    res['P'] = dP.cpu().numpy().astype(np.float64).reshape(N * frames, kmax, 128).sum(axis=1)
    res['raw'] = (u.cpu(), v.cpu())
    return res


@functools.lru_cache(maxsize=None)
def _layer_reference(d, last):
    c = TO.layer_case(d)
    g64, g32 = TO.layer_grads(c, last, torch.float64), TO.layer_grads(c, last, torch.float32)
    return c, g64, max(TO.rel_err(g32[k], g64[k]) for k in g64 if np.abs(g64[k]).max() > 0)


@pytest.mark.parametrize('last', [False, True], ids=['residual', 'last_head'])
@pytest.mark.parametrize('d', DILATIONS)
def test_layer_backward_matches_float64_autograd(gpu, d, last):
    """416 rows = 13 units with the utterance boundary in the middle of unit 6; every output of the layer backward against float64
    autograd of that one layer, within 8 x the error of float32 autograd of the same layer."""
    c, g64, e32 = _layer_reference(d, last)
    got = _layer_backward(c, last, gpu)
    for k, want in g64.items():
        assert np.isfinite(got[k]).all(), k
        if np.abs(want).max() == 0:
            assert np.abs(got[k]).max() == 0, k
            continue
        err = TO.rel_err(got[k], want)
        print('d=%d %s %s err %.3g (E32 %.3g)' % (d, 'last' if last else 'residual', k, err, e32))
        assert err <= MARGIN * e32, (k, err, e32)
    if d >= TO.T:       # no row has a look-back: the tap at t - d sees zeros only
        assert np.abs(got['filter'][0]).max() == 0 and np.abs(got['gate'][0]).max() == 0
        assert np.abs(g64['filter'][0]).max() == 0


def test_layer_backward_keeps_utterances_apart(gpu):
    """The gradient for the input of utterance 0 does not depend on g of utterance 1, bit for bit -- also in the unit the two share and
    across the look-ahead at t + d."""
    for d in (1, 48):
        c = TO.layer_case(d)
        g2 = c['g'].copy()
        g2[1] = np.random.RandomState(99).randn(TO.T, 64).astype(np.float32)
        a, b = _layer_backward(c, False, gpu), _layer_backward(c, False, gpu, g=g2)
        for i in (0, 1):
            ua, ub = TO.from_tile32(a['raw'][i].numpy(), TO.N * TO.T, 64), TO.from_tile32(b['raw'][i].numpy(), TO.N * TO.T, 64)
            assert np.array_equal(ua[:TO.T], ub[:TO.T])
            assert not np.array_equal(ua[TO.T:], ub[TO.T:])
        assert np.array_equal(a['x'][0], b['x'][0]) and not np.array_equal(a['x'][1], b['x'][1])


# ---- the whole model ------------------------------------------------------------------------------------------------------------------
def _model(device, precision='f32'):
    from pwv_amd.models import IAFVocoder
    from pwv_amd.variables import VariableStore
    cfg, w, mel, z, wav = TO.problem()
    set_hparams(cfg)
    store = VariableStore(device=device)
    store.load_dict(w)
    model = IAFVocoder(batch_size=TO.N, length=TO.T, store=store, precision=precision)
    return model, store, _dev(wav, device), _dev(mel, device), _dev(z, device)


def _check_grads(grads, loss, pred, what=''):
    ref = TO.reference()
    g64, bar = ref['g64'], MARGIN * ref['E32']
    assert sorted(grads) == sorted(g64)
    worst = 0.0
    for k, want in g64.items():
        got = grads[k].detach().cpu().numpy().astype(np.float64)
        assert got.shape == want.shape if want is not None else got.shape == TO.problem()[1][k].shape, k
        if want is None:
            assert np.abs(got).max() == 0, k        # exact zeros for what the model never reads
            continue
        assert np.isfinite(got).all(), k
        err = TO.rel_err(got, want)
        worst = max(worst, err)
        assert err <= bar, (what, k, err, bar)
    print('%s worst gradient err %.3g (E32 %.3g, bar %.3g)' % (what, worst, ref['E32'], bar))
    assert abs(float(loss) - ref['loss']) <= 2e-6 * max(1.0, abs(ref['loss']))
    assert np.abs(pred.detach().cpu().numpy().astype(np.float64) - ref['pred']).max() <= TOL_F32
    return worst


def test_model_gradients_match_float64_autograd(gpu):
    """All 149 gradients and the loss of the small model against float64 autograd, exact zeros for the 32 unused variables, pred within
    the project's fp32 bar."""
    from pwv_amd import train as TR
    model, _, wav, mel, z = _model(gpu)
    loss, pred, grads = TR.loss_and_grad(model, wav, mel, z=z)
    torch.cuda.synchronize()
    assert tuple(pred.shape) == (TO.N, TO.T, 1) and loss.dim() == 0 and loss.is_cuda
    assert sum(v is not None for v in TO.reference()['g64'].values()) == 149
    _check_grads(grads, loss, pred, 'default grid')


@pytest.mark.parametrize('max_workgroups', [1, 3, 0])
def test_partials_and_determinism(gpu, max_workgroups):
    """1, 3 and the default number of partials per weight-gradient reduction: each agrees with float64 under the same bar and is
    bit-identical to its own repetition."""
    from pwv_amd import train as TR
    model, _, wav, mel, z = _model(gpu)
    runs = []
    for _ in range(2):
        loss, pred, grads = TR.loss_and_grad(model, wav, mel, z=z, max_workgroups=max_workgroups)
        torch.cuda.synchronize()
        runs.append((loss, pred, grads))
    _check_grads(runs[0][2], runs[0][0], runs[0][1], 'max_workgroups=%d' % max_workgroups)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    for k in runs[0][2]:
        assert torch.equal(runs[0][2][k], runs[1][2][k]), k


def test_guarded_loss_and_grad(gpu):
    """One loss_and_grad inside poisoned, guard-banded buffers: no store outside a buffer, and no NaN in pred, loss or any gradient -- a
    partial slot, a dP slot or an activation that is read but never written is poisoned."""
    from pwv_amd import engine
    from pwv_amd import train as TR
    with guarded(TR, engine) as g:
        model, _, wav, mel, z = _model(gpu)
        loss, pred, grads = TR.loss_and_grad(model, wav, mel, z=z, max_workgroups=3)
        torch.cuda.synchronize()
        g.check()
        assert any('train.py' in s for s in g.sites())
        assert torch.isfinite(loss).all() and torch.isfinite(pred).all()
        for k, v in grads.items():
            assert torch.isfinite(v).all(), k
        _check_grads(grads, loss, pred, 'guarded')


def test_training_trains(gpu):
    """Ten Trainer.step calls at lr 2e-4 on the fixed batch with a fixed z against ten steps of the float64 restatement (autograd + numpy
    Adam): the loss falls at every step, by at least half of the reference's decrease, and the shadows follow the restatement's.

    The bar of the shadows is built like the gradients': D32 = the largest |shadow - shadow64| of the SAME restatement run in float32
    (float32 autograd, variables, moments and shadows stored in float32), computed at run time, and the GPU must stay within 8 D32 for
    every variable.  The gradient bar times lr, 8 E32 lr = 3e-9, cannot be asked of any float32 implementation: a shadow of size 0.3
    is stored to 3e-8, and Adam's first steps move an entry by lr sign(g), so an entry whose gradient is smaller than its float32 error
    may move the other way by 2 lr per step whatever the implementation.  Both show in D32."""
    from pwv_amd import train as TR
    ref_losses, ref_shadow = TO.trajectory(10)
    _, shadow32 = TO.trajectory(10, single=True)
    d32 = max(float(np.abs(shadow32[k].astype(np.float64) - ref_shadow[k]).max()) for k in ref_shadow)
    model, store, wav, mel, z = _model(gpu)
    tr = TR.Trainer(model, lr=TO.LR, beta2=TO.BETA2, ema_decay=TO.DECAY)
    version = store.version
    losses = [float(tr.step(wav, mel, z=z)) for _ in range(10)]
    assert store.version > version and tr.steps == 10
    loss_after, _, _ = TR.loss_and_grad(model, wav, mel, z=z)
    losses.append(float(loss_after))
    print('gpu  ', ' '.join('%.5f' % v for v in losses))
    print('fp64 ', ' '.join('%.5f' % v for v in ref_losses))
    print('largest difference of the trajectories %.3g' % max(abs(a - b) for a, b in zip(losses, ref_losses)))
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    assert losses[0] - losses[-1] >= 0.5 * (ref_losses[0] - ref_losses[-1])
    shadows = tr.shadows()
    assert sorted(shadows) == sorted(ref_shadow)
    errs = {k: float(np.abs(shadows[k].cpu().numpy().astype(np.float64) - want).max()) for k, want in ref_shadow.items()}
    print('largest shadow difference %.3g (D32 %.3g, bar %.3g; 8 E32 lr = %.3g)' % (max(errs.values()), d32, MARGIN * d32, MARGIN * TO.reference()['E32'] * TO.LR))
    for k, err in errs.items():
        assert err <= MARGIN * d32, (k, err, d32)
    moved = max(float(np.abs(ref_shadow[k] - TO.problem()[1][k]).max()) for k in ref_shadow)
    assert MARGIN * d32 < 0.5 * moved, (d32, moved)      # the bar still tells a shadow that moved from one that did not


def test_train_cli_then_generate(gpu, tmp_path):
    """`python -m pwv_amd.train train/small --steps=3` on seeded stand-in audio writes a checkpoint that `generate` loads with use_ema, and
    the result is finite audio."""
    env = dict(os.environ, PWV_LOGDIR=str(tmp_path), PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = subprocess.run([sys.executable, '-m', 'pwv_amd.train', 'train/small', '--steps=3', '--seed=4'], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:]
    lines = [l for l in out.stdout.splitlines() if 'loss/likelihood' in l]
    assert len(lines) == 3 and all(np.isfinite(float(l.split()[-1])) for l in lines), out.stdout[-2000:]
    ckpt = tmp_path / 'model-3.npz'
    assert ckpt.exists()
    with np.load(str(ckpt)) as z:
        assert any(k.endswith('/ExponentialMovingAverage') for k in z.files) and any(k.endswith('/Adam_1') for k in z.files)
    gen = subprocess.run([sys.executable, '-m', 'pwv_amd.generate', 'train/small'], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         text=True, timeout=300)
    assert gen.returncode == 0, gen.stdout[-3000:]
    assert 'No checkpoint found' not in gen.stdout
    pred = np.load(str(tmp_path / 'pred_wav.npy'))
    assert pred.shape[1] == 1600 and np.isfinite(pred).all() and np.abs(pred).max() > 0
