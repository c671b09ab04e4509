"""GPU: training the skip-connection architecture (pwv_amd/train.py: use_skip_connection=True -> pwv_train_skip_*,
csrc/pwv_train_skip.hip) against float64 autograd on the CPU (tests/train_skip_oracle.py): one layer and the head on S through the C
ABI at ragged shapes, uniform and packed, the whole small skip model, the training forward against the generation forward, five
optimiser steps, guarded buffers and `python -m pwv_amd.train train/small_skip` -> `generate`.

The bars are the project's own (tests/test_gpu_train.py): a gradient within 8 E32 of float64 per variable, E32 = the error of float32
autograd on the CPU of the same function, computed at run time; TOL_F32 for a prediction (times max(1, |value|max) for the O(4) rows of
one layer's x_out and S); 8 D32 for a shadow after five steps."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import train_oracle as TO
from tests import train_skip_oracle as SO
from tests import train_varlen_oracle as VO
from tests.guarded import guarded
from tests.util import TOL_F32, set_hparams

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 8
# (N, T, hop, offset): 19.5 units, 4.5 units with 17 P rows per unit, 9.4 units with one frame boundary, half a unit
SHAPES = [(3, 208, 16, 8), (2, 72, 2, 1), (1, 300, 256, 128), (1, 16, 16, 8)]
LAYER_CASES = [(s, d) for i, s in enumerate(SHAPES) for d in ((1, 48, 256) if i == 0 else (1, 48))]
PACKED_LAYER_CASES = [(tuple(VO.DENSE[0]), VO.DENSE[1], 1), (tuple(VO.DENSE[0]), VO.DENSE[1], 3), (tuple(VO.LENGTHS), VO.HOP, 1),
                      (tuple(VO.LENGTHS), VO.HOP, 48)]
MODEL_SHAPES = [(3, 240, 80), (1, 16, 16), (5, 16, 16)]


@pytest.fixture(autouse=True)
def _default_hparams():
    yield
    from pwv_amd.hparam import hparam as hp
    hp.set_hparam_yaml('default')


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _id(v):
    return 'x'.join(str(x) for x in v) if isinstance(v, (tuple, list)) else str(v)


# ---- one layer and the head through ctypes --------------------------------------------------------------------------------------------
class _Call(object):
    """The device side of a one-layer case: its inputs uploaded once (tile32 inputs with NaN padding rows), and the four entry points."""

    def __init__(self, c, device, packed):
        from pwv_amd import _lib
        self.c, self.device, self.packed, self.lib = c, device, packed, _lib.lib()
        self.rows = c['rows']
        self.kmax = (c['hop'] + 30) // 32 + 1
        self.prows = c['P'].shape[0]
        self.t = {k: _dev(c[k], device) for k in ('P', 'filter', 'gate', 'dense', 'dense_bias', 'skip', 'skip_bias', 'post1', 'post1_bias', 'post2',
                                                  'post2_bias', 'dy')}
        self.x = _dev(SO.to_tile32(c['x']), device)
        self.S_in = _dev(SO.to_tile32(c['S_in']), device)
        self.dS = _dev(SO.to_tile32(c['dS']), device)
        self.g = _dev(SO.to_tile32(c['g']), device)
        if packed:
            self.cu_r = _dev(np.asarray(c['cu_rows'], dtype=np.int32), device)
            self.cu_f = _dev(np.asarray(c['cu_frames'], dtype=np.int32), device)

    def nan(self, *shape):
        return torch.full(shape, float('nan'), dtype=torch.float32, device=self.device)

    def tile(self, C=64):
        return self.nan(((self.rows + 31) // 32) * 32 * C)

    def args(self, max_workgroups, **kw):
        from pwv_amd import _lib
        c = self.c
        base = dict(cond_hop=c['hop'], cond_offset=c['offset'], proj_row_stride=128, d_proj_row_stride=128, max_workgroups=max_workgroups,
                    dilation=c['d'], next_dilation=1)
        if self.packed:
            base.update(cu_rows=self.cu_r.data_ptr(), cu_frames=self.cu_f.data_ptr(), n=len(c['lengths']), rows=self.rows, proj_rows=self.prows)
        else:
            base.update(N=c['N'], T=c['T'], cond_frames=c['frames'])
        base.update({k: (v.data_ptr() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()})
        return _lib.TrainSkipArgs(**base)

    def call(self, name, a):
        from pwv_amd import _lib
        _lib.check(getattr(self.lib, name)(ctypes.byref(a), torch.cuda.current_stream().cuda_stream), name)

    def workspace(self, max_workgroups):
        ws = self.nan(self.lib.pwv_train_skip_workspace_bytes(ctypes.byref(self.args(max_workgroups))) // 4)
        assert ws.numel() > 0
        return ws

    def layer_forward(self, last, accumulate, max_workgroups):
        """(x_out [rows, 64] or None, S_out [rows, 128], the raw S buffer) as float32 numpy."""
        from pwv_amd import _lib
        t = self.t
        S = self.S_in.clone() if accumulate else self.tile(128)
        x_out = None if last else self.tile()
        self.call('pwv_train_skip_layer_fwd_f32', self.args(
            max_workgroups, form=_lib.TRAIN_LAST if last else _lib.TRAIN_RESIDUAL, x=self.x, proj=t['P'], filter=t['filter'], gate=t['gate'],
            dense=None if last else t['dense'], dense_bias=None if last else t['dense_bias'], x_out=x_out, skip=t['skip'],
            skip_bias=t['skip_bias'], skip_sum=S, skip_accumulate=int(accumulate)))
        torch.cuda.synchronize()
        raw = S.cpu().numpy()
        return (None if last else TO.from_tile32(x_out.cpu().numpy(), self.rows, 64)), TO.from_tile32(raw, self.rows, 128), raw

    def layer_backward(self, last, max_workgroups):
        """Every output of the layer backward as float64 numpy, dP with its slots added."""
        from pwv_amd import _lib
        t, c = self.t, self.c
        u, v, ws = self.tile(), self.tile(), self.workspace(max_workgroups)
        dP = torch.zeros((self.prows * self.kmax, 128), dtype=torch.float32, device=self.device)
        names = ('filter', 'gate', 'skip') + (() if last else ('dense', 'dense_bias'))
        out = {k: self.nan(*c[k].shape) for k in names}
        kw = dict(form=_lib.TRAIN_LAST if last else _lib.TRAIN_RESIDUAL, x=self.x, proj=t['P'], filter=t['filter'], gate=t['gate'], skip=t['skip'],
                  d_skip_sum=self.dS, u=u, v=v, d_proj=dP, d_filter=out['filter'], d_gate=out['gate'], d_skip=out['skip'], workspace=ws,
                  workspace_bytes=ws.numel() * 4)
        if not last:
            kw.update(dense=t['dense'], u_next=self.g, v_next=torch.zeros_like(self.g), d_dense=out['dense'], d_dense_bias=out['dense_bias'])
        self.call('pwv_train_skip_layer_bwd_f32', self.args(max_workgroups, **kw))
        torch.cuda.synchronize()
        res = {k: val.cpu().numpy().astype(np.float64) for k, val in out.items()}
        res['U'] = TO.from_tile32(u.cpu().numpy(), self.rows, 64).astype(np.float64)
        res['V'] = TO.from_tile32(v.cpu().numpy(), self.rows, 64).astype(np.float64)
        res['P'] = dP.cpu().numpy().astype(np.float64).reshape(self.prows, self.kmax, 128).sum(axis=1)
        return res

    def head(self, max_workgroups):
        """y [rows] float32 and the head backward's outputs as float64 numpy."""
        t, c = self.t, self.c
        w = dict(post1=t['post1'], post1_bias=t['post1_bias'], post2=t['post2'], post2_bias=t['post2_bias'])
        y = self.nan(self.rows)
        self.call('pwv_train_skip_head_fwd_f32', self.args(max_workgroups, skip_sum=self.S_in, y=y, **w))
        dS, ws = self.tile(128), self.workspace(max_workgroups)
        out = {k: self.nan(*c[k].shape) for k in ('skip_bias', 'post1', 'post1_bias', 'post2', 'post2_bias')}
        self.call('pwv_train_skip_head_bwd_f32', self.args(
            max_workgroups, skip_sum=self.S_in, d_out=t['dy'], d_skip_sum_out=dS, d_skip_bias=out['skip_bias'], d_post1=out['post1'],
            d_post1_bias=out['post1_bias'], d_post2=out['post2'], d_post2_bias=out['post2_bias'], workspace=ws, workspace_bytes=ws.numel() * 4, **w))
        torch.cuda.synchronize()
        res = {k: val.cpu().numpy().astype(np.float64) for k, val in out.items()}
        res['dS'] = TO.from_tile32(dS.cpu().numpy(), self.rows, 128).astype(np.float64)
        return y.cpu().numpy(), res


def _e32(g32, g64, names):
    return max(TO.rel_err(g32[k], g64[k]) for k in names if np.abs(g64[k]).max() > 0)


def _check_outputs(got, g64, e32, names, what):
    for k in names:
        want = g64[k]
        assert np.isfinite(got[k]).all(), (what, k)         # no NaN of a padding row or of an unwritten slot reaches a gradient
        if np.abs(want).max() == 0:
            assert np.abs(got[k]).max() == 0, (what, k)
            continue
        err = TO.rel_err(got[k], want)
        print('%s %s err %.3g (E32 %.3g)' % (what, k, err, e32))
        assert err <= MARGIN * e32, (what, k, err, e32)


def _check_layer(c, device, packed, what):
    call = _Call(c, device, packed)
    S_in32 = c['S_in']
    for last in (False, True):
        names = SO.GRADS_LAST if last else SO.GRADS_RESIDUAL
        r64, r32 = SO.skip_layer(c, last, torch.float64), SO.skip_layer(c, last, torch.float32)
        term64 = SO.skip_layer(c, last, torch.float64, accumulate=False)['S_out']
        e32 = _e32(r32, r64, names)
        form = '%s %s' % (what, 'last' if last else 'residual')
        # forward: accumulate 0 writes the term, 1 adds it to S_in with one rounding; S is the same bits whatever the grid
        x0, S0, raw0 = call.layer_forward(last, 0, 1)
        for mwg in (3, 0):
            xg, Sg, rawg = call.layer_forward(last, 0, mwg)
            assert np.array_equal(S0, Sg) and (last or np.array_equal(x0, xg)), (form, mwg)
        assert np.isfinite(S0).all() and np.abs(S0 - term64).max() <= TOL_F32 * max(1.0, np.abs(term64).max()), form
        if not last:
            assert np.isfinite(x0).all() and np.abs(x0 - r64['x_out']).max() <= TOL_F32 * max(1.0, np.abs(r64['x_out']).max()), form
        for mwg in (1, 3, 0):
            x1, S1, raw1 = call.layer_forward(last, 1, mwg)
            assert np.array_equal(S1, S_in32 + S0), (form, mwg)          # float32 + float32: S_in + (o skip + skip_bias), one rounding
            assert last or np.array_equal(x1, x0)
        assert np.abs(S1 - r64['S_out']).max() <= TOL_F32 * max(1.0, np.abs(r64['S_out']).max()), form
        for mwg in (1, 3, 0):
            _check_outputs(call.layer_backward(last, mwg), r64, e32, names, '%s max_workgroups=%d' % (form, mwg))


def _check_head(c, device, packed, what):
    call = _Call(c, device, packed)
    h64, h32 = SO.skip_head(c, torch.float64), SO.skip_head(c, torch.float32)
    names = ('dS', 'skip_bias', 'post1', 'post1_bias', 'post2', 'post2_bias')
    e32 = _e32(h32, h64, names)
    for mwg in (1, 3, 0):
        y, got = call.head(mwg)
        assert np.isfinite(y).all() and np.abs(y - h64['y']).max() <= TOL_F32 * max(1.0, np.abs(h64['y']).max()), what
        _check_outputs(got, h64, e32, names, '%s head max_workgroups=%d' % (what, mwg))


@pytest.mark.parametrize('shape, d', LAYER_CASES, ids=['%s-d%d' % (_id(s), d) for s, d in LAYER_CASES])
def test_skip_layer_matches_float64_autograd(gpu, shape, d):
    """One skip layer through the C ABI, forward and backward, both forms, skip_accumulate 0 and 1, 1 / 3 / the default number of
    workgroups: x_out and S against float64, S_in + term to one rounding, every gradient within 8 E32; the inputs' padding rows are NaN."""
    N, T, hop, offset = shape
    _check_layer(SO.layer_case(d, N, T, hop, offset), gpu, False, '%s d=%d' % (_id(shape), d))


@pytest.mark.parametrize('shape', SHAPES, ids=_id)
def test_skip_head_matches_float64_autograd(gpu, shape):
    """The head on S, forward and backward: y, dS, the post weights' gradients and the column sums of dS (every layer's d skip_bias)."""
    N, T, hop, offset = shape
    _check_head(SO.layer_case(1, N, T, hop, offset), gpu, False, _id(shape))


@pytest.mark.parametrize('lengths, hop, d', PACKED_LAYER_CASES, ids=['%s-d%d' % (_id(l), d) for l, _, d in PACKED_LAYER_CASES])
def test_packed_skip_layer_matches_float64_autograd(gpu, lengths, hop, d):
    """The same layer on packed rows: four utterances in one unit at hop 8 (DENSE) and the ragged LENGTHS at hop 16; the head on the
    packed rows too."""
    c = SO.packed_layer_case(d, lengths, hop)
    _check_layer(c, gpu, True, 'packed %s d=%d' % (_id(lengths), d))
    if d == 1:
        _check_head(c, gpu, True, 'packed %s' % _id(lengths))


# ---- the whole model ------------------------------------------------------------------------------------------------------------------
def _store(w, device):
    from pwv_amd.variables import VariableStore
    store = VariableStore(device=device)
    store.load_dict(w)
    return store


def _model(device, shape=(TO.N, TO.T, TO.HOP)):
    from pwv_amd.models import IAFVocoder
    N, T, hop = shape
    cfg, w, mel, z, wav = SO.problem(N, T, hop)
    set_hparams(cfg)
    store = _store(w, device)
    return IAFVocoder(batch_size=N, length=T, store=store, precision='f32'), store, _dev(wav, device), _dev(mel, device), _dev(z, device)


def _packed_model(device, lengths=tuple(VO.LENGTHS), hop=VO.HOP):
    from pwv_amd.models import IAFVocoder
    cfg, w, mels, zs, wavs = SO.packed_problem(lengths, hop)
    set_hparams(cfg)
    model = IAFVocoder(batch_size=1, length=max(lengths), store=_store(w, device), precision='f32')
    return model, [_dev(a[0, :, 0], device) for a in wavs], [_dev(a[0], device) for a in mels], [_dev(a[0], device) for a in zs]


def _check_grads(grads, ref, what):
    """All 173 live gradients within 8 E32 of float64 autograd, exact zeros for the 8 the model never reads, and every layer's
    d skip_bias of a net the same bits."""
    g64, bar = ref['g64'], MARGIN * ref['E32']
    assert sorted(grads) == sorted(g64)
    worst, zeros = 0.0, 0
    for k, want in g64.items():
        got = grads[k].detach().cpu().numpy().astype(np.float64)
        if want is None:
            assert got.shape == SO.weights()[k].shape and np.abs(got).max() == 0, (what, k)
            zeros += 1
            continue
        assert got.shape == want.shape and np.isfinite(got).all(), (what, k)
        err = TO.rel_err(got, want)
        worst = max(worst, err)
        assert err <= bar, (what, k, err, bar)
    print('%s worst gradient err %.3g (E32 %.3g, bar %.3g)' % (what, worst, ref['E32'], bar))
    assert zeros == SO.DEAD and len(g64) - zeros == SO.LIVE
    nets = sorted(set(k.split('/dilated_stack/')[0] for k in grads if k.endswith('/skip_bias')))
    assert len(nets) == 4
    for net in nets:
        sb = [grads['%s/dilated_stack/layer%d/skip_bias' % (net, j)] for j in range(4)]
        assert all(torch.equal(sb[0], s) for s in sb[1:]), net
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


@pytest.mark.parametrize('max_workgroups', [1, 3, 0])
def test_skip_model_gradients_match_float64_autograd(gpu, max_workgroups):
    """2 x 208 at hop 16 with 1, 3 and the default number of partials: all 173 gradients, the loss and pred against float64 autograd,
    exact zeros for the 8 unread variables, each run the bits of its repetition."""
    from pwv_amd import train as TR
    from pwv_amd._lib import PwvError
    model, _, wav, mel, z = _model(gpu)
    with pytest.raises(PwvError, match='skip accumulation'):
        TR.loss_and_grad(model, wav, mel, z=z)
    runs = []
    for _ in range(2):
        runs.append(TR.loss_and_grad(model, wav, mel, z=z, max_workgroups=max_workgroups, use_skip_connection=True))
        torch.cuda.synchronize()
    _check_uniform(runs[0], SO.reference(), (TO.N, TO.T), 'skip max_workgroups=%d' % max_workgroups)
    _same(runs[0], runs[1])


@pytest.mark.parametrize('shape', MODEL_SHAPES, ids=_id)
def test_skip_model_gradients_at_ragged_shapes(gpu, shape):
    """3 x 240 at hop 80 (22.5 units, four dP slots), 1 x 16 and 5 x 16 (utterances of half a unit)."""
    from pwv_amd import train as TR
    model, _, wav, mel, z = _model(gpu, shape)
    runs = []
    for _ in range(2):
        runs.append(TR.loss_and_grad(model, wav, mel, z=z, use_skip_connection=True))
        torch.cuda.synchronize()
    _check_uniform(runs[0], SO.reference(*shape), shape, 'skip %s' % _id(shape))
    _same(runs[0], runs[1])


@pytest.mark.parametrize('max_workgroups', [1, 0])
def test_packed_skip_model_gradients_match_float64_autograd(gpu, max_workgroups):
    """The packed batch (208, 16, 48, 144) against float64 autograd of the utterances run one by one; the bits of its repetition."""
    from pwv_amd import train as TR
    model, wavs, mels, zs = _packed_model(gpu)
    runs = []
    for _ in range(2):
        runs.append(TR.loss_and_grad_varlen(model, wavs, mels, z=zs, max_workgroups=max_workgroups, use_skip_connection=True))
        torch.cuda.synchronize()
    _check_packed(runs[0], SO.packed_reference(), VO.LENGTHS, 'packed skip max_workgroups=%d' % max_workgroups)
    _same(runs[0], runs[1])


def test_equal_lengths_give_the_bits_of_the_uniform_batch(gpu):
    """Two utterances of 208 samples packed = the uniform 2 x 208 call, bit for bit: the loss, every pred, every gradient."""
    from pwv_amd import train as TR
    model, _, wav, mel, z = _model(gpu)
    a = TR.loss_and_grad(model, wav, mel, z=z, use_skip_connection=True)
    b = TR.loss_and_grad_varlen(model, [wav[i, :, 0] for i in range(TO.N)], [mel[i] for i in range(TO.N)], z=[z[i] for i in range(TO.N)],
                                use_skip_connection=True)
    torch.cuda.synchronize()
    _same((a[0], [a[1][i] for i in range(TO.N)], a[2]), b)


def test_a_packed_prediction_is_the_utterance_alone(gpu):
    """preds[i] of the packed batch = the prediction of utterance i trained alone with the same z, bit for bit."""
    from pwv_amd import train as TR
    model, wavs, mels, zs = _packed_model(gpu)
    _, preds, _ = TR.loss_and_grad_varlen(model, wavs, mels, z=zs, use_skip_connection=True)
    for i in range(len(wavs)):
        _, alone, _ = TR.loss_and_grad_varlen(model, [wavs[i]], [mels[i]], z=[zs[i]], use_skip_connection=True)
        torch.cuda.synchronize()
        assert torch.equal(preds[i], alone[0]), i


def test_training_forward_agrees_with_the_generation_forward(gpu):
    """pred of loss_and_grad against model(mel, z) at precision 'f32' under the same hparams: the SKIP variants of the per-layer
    generation kernels are an independent implementation of the same forward."""
    from pwv_amd import train as TR
    model, _, wav, mel, z = _model(gpu)
    _, pred, _ = TR.loss_and_grad(model, wav, mel, z=z, use_skip_connection=True)
    out = model(None, mel, is_training=False, z=z, verify=False)
    model.verify()
    assert out.shape == pred.shape
    err, scale = float((out - pred).abs().max()), max(1.0, float(out.abs().max()))
    print('largest |training forward - generation forward| %.3g (|y|max %.3g)' % (err, float(out.abs().max())))
    assert torch.isfinite(out).all() and err <= TOL_F32 * scale


@pytest.mark.parametrize('fused', [False, True], ids=['foreach', 'fused'])
def test_skip_training_trains(gpu, fused):
    """Five Trainer.step calls (use_skip_connection=True) at lr 2e-4 on the fixed batch against five steps of the float64 restatement:
    the loss falls at every step, by at least half of the reference's decrease, and the shadows stay within 8 D32, D32 = the largest
    |shadow - shadow64| of the same restatement run in float32 (tests/test_gpu_train.py, test_training_trains)."""
    from pwv_amd import train as TR
    ref_losses, ref_shadow = SO.trajectory(5)
    _, shadow32 = SO.trajectory(5, single=True)
    d32 = max(float(np.abs(shadow32[k].astype(np.float64) - ref_shadow[k]).max()) for k in ref_shadow)
    model, store, wav, mel, z = _model(gpu)
    tr = TR.Trainer(model, lr=TO.LR, beta2=TO.BETA2, ema_decay=TO.DECAY, fused=fused, use_skip_connection=True)
    losses = [float(tr.step(wav, mel, z=z)) for _ in range(5)]
    assert tr.steps == 5
    losses.append(float(TR.loss_and_grad(model, wav, mel, z=z, use_skip_connection=True)[0]))
    print('gpu  ', ' '.join('%.5f' % v for v in losses))
    print('fp64 ', ' '.join('%.5f' % v for v in ref_losses))
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    assert losses[0] - losses[-1] >= 0.5 * (ref_losses[0] - ref_losses[-1])
    shadows = tr.shadows()
    assert sorted(shadows) == sorted(ref_shadow) and len(shadows) == 181
    errs = {k: float(np.abs(shadows[k].cpu().numpy().astype(np.float64) - want).max()) for k, want in ref_shadow.items()}
    print('largest shadow difference %.3g (D32 %.3g, bar %.3g)' % (max(errs.values()), d32, MARGIN * d32))
    for k, err in errs.items():
        assert err <= MARGIN * d32, (k, err, d32)
    moved = max(float(np.abs(ref_shadow[k] - SO.weights()[k]).max()) for k in ref_shadow)
    assert MARGIN * d32 < 0.5 * moved, (d32, moved)      # the bar still tells a shadow that moved from one that did not


def test_guarded_skip_loss_and_grad(gpu):
    """One uniform and one packed run with three partials inside poisoned, guard-banded buffers: no band is touched, no NaN -- of a
    padding row of S or dS, of an unwritten partial -- is left in the loss, a prediction or a gradient, and the results are the bits
    of the plain runs."""
    from pwv_amd import engine
    from pwv_amd import train as TR
    model, _, wav, mel, z = _model(gpu)
    plain = TR.loss_and_grad(model, wav, mel, z=z, max_workgroups=3, use_skip_connection=True)
    model, wavs, mels, zs = _packed_model(gpu)
    plain_packed = TR.loss_and_grad_varlen(model, wavs, mels, z=zs, max_workgroups=3, use_skip_connection=True)
    torch.cuda.synchronize()
    with guarded(TR, engine) as g:
        model, _, wav, mel, z = _model(gpu)
        run = TR.loss_and_grad(model, wav, mel, z=z, max_workgroups=3, use_skip_connection=True)
        model, wavs, mels, zs = _packed_model(gpu)
        run_packed = TR.loss_and_grad_varlen(model, wavs, mels, z=zs, max_workgroups=3, use_skip_connection=True)
        torch.cuda.synchronize()
        g.check()
        assert any('train.py' in s for s in g.sites())
        for loss, preds, grads in (run, run_packed):
            assert torch.isfinite(loss).all() and all(torch.isfinite(p).all() for p in (preds if isinstance(preds, list) else [preds]))
            for k, v in grads.items():
                assert torch.isfinite(v).all(), k
        _same(plain, run)
        _same(plain_packed, run_packed)


def test_train_cli_skip_packed_data_parallel(gpu, tmp_path):
    """`python -m pwv_amd.train train/small_skip --varlen --gpus 2 --steps 2`: two ranks (on a machine with one GPU both on it, over
    gloo: the dry run of tests/test_gpu_train_opt.py), each a DataParallelTrainer that was handed the request, on packed batches."""
    env = dict(os.environ, PWV_LOGDIR=str(tmp_path), PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT', 'MASTER_ADDR', 'PWV_TRAIN_DRYRUN_ONE_GPU'):
        env.pop(k, None)
    if torch.cuda.device_count() < 2:
        env['PWV_TRAIN_DRYRUN_ONE_GPU'] = '1'
    out = subprocess.run([sys.executable, '-m', 'pwv_amd.train', 'train/small_skip', '--varlen', '--gpus', '2', '--steps', '2'], cwd=ROOT, env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith('step ')]
    assert len(lines) == 2 and all('loss/likelihood' in l and np.isfinite(float(l.split()[-1])) for l in lines), out.stdout[-2000:]
    assert (tmp_path / 'model-2.npz').exists()


def test_train_cli_skip_then_generate(gpu, tmp_path):
    """`python -m pwv_amd.train train/small_skip --steps=3` in a fresh process opts in by itself, writes a checkpoint that `generate`
    loads with use_ema, and the result is finite audio of the asked length."""
    env = dict(os.environ, PWV_LOGDIR=str(tmp_path), PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = subprocess.run([sys.executable, '-m', 'pwv_amd.train', 'train/small_skip', '--steps=3', '--seed=4'], cwd=ROOT, env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:]
    lines = [l for l in out.stdout.splitlines() if 'loss/likelihood' in l]
    assert len(lines) == 3 and all(np.isfinite(float(l.split()[-1])) for l in lines), out.stdout[-2000:]
    ckpt = tmp_path / 'model-3.npz'
    assert ckpt.exists()
    with np.load(str(ckpt)) as z:
        assert any(k.endswith('/ExponentialMovingAverage') for k in z.files) and any(k.endswith('/Adam_1') for k in z.files)
        assert any(k.endswith('layer0/skip') for k in z.files)
    gen = subprocess.run([sys.executable, '-m', 'pwv_amd.generate', 'train/small_skip'], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, text=True, timeout=300)
    assert gen.returncode == 0, gen.stdout[-3000:]
    assert 'No checkpoint found' not in gen.stdout
    pred = np.load(str(tmp_path / 'pred_wav.npy'))
    assert pred.shape[1] == 1600 and np.isfinite(pred).all() and np.abs(pred).max() > 0
