"""GPU: training on packed batches of mixed-length utterances (pwv_amd/train.py: loss_and_grad_varlen -> pwv_train_varlen_* and
pwv_train_loss_varlen_f32, csrc/pwv_train_varlen.hip, csrc/pwv_train_loss.hip) against float64 autograd on the CPU
(tests/train_varlen_oracle.py): one layer through the C ABI, the whole small model, the loss head, five optimiser steps, guarded
buffers and `python -m pwv_amd.train --varlen`.

The bars are the project's own: a gradient within 8 E32 of float64 per variable (E32 = the error of float32 autograd on the CPU of the
same function, computed at run time; tests/test_gpu_train.py), TOL_F32 for a prediction, 1e-10 for the score table.  The packed batch is
tests.train_varlen_oracle.LENGTHS = [208, 16, 48, 144]: 416 rows = 13 units."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import train_oracle as TO
from tests import train_power_oracle as PO
from tests import train_varlen_oracle as VO
from tests.guarded import guarded
from tests.util import TOL_F32, set_hparams

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 8
DILATIONS = (1, 32, 48, 256)
WIN = PO.WIN


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


# ---- one layer through ctypes ---------------------------------------------------------------------------------------------------------
def _layer_backward(c, last, device, g=None, max_workgroups=0, next_dilation=1, v_next=None):
    """The packed layer backward (and, in the last form, the head backward in front of it); returns float64 numpy: the input gradient
    assembled with its look-ahead per utterance, dP with its slots added, every weight and bias gradient, and the raw U, V.  The residual
    form takes U = g (default: c['g']) and V = v_next [rows, 64] (default: zeros), gathered with next_dilation."""
    from pwv_amd import _lib
    lib = _lib.lib()
    d, hop, lengths, cu_rows, cu_frames = c['d'], c['hop'], c['lengths'], c['cu_rows'], c['cu_frames']
    rows, prows, n = cu_rows[-1], cu_frames[-1], len(lengths)
    kmax = (hop + 30) // 32 + 1
    t = {k: _dev(c[k], device) for k in ('P', 'filter', 'gate', 'dense', 'dense_bias', 'skip', 'skip_bias', 'post1', 'post1_bias', 'post2', 'post2_bias', 'dy')}
    x = _dev(TO.to_tile32(c['x']), device)
    cu_r, cu_f = _dev(np.asarray(cu_rows, dtype=np.int32), device), _dev(np.asarray(cu_frames, dtype=np.int32), device)
    nan = lambda *shape: torch.full(shape, float('nan'), dtype=torch.float32, device=device)
    tile = lambda: nan(((rows + 31) // 32) * 32 * 64)
    u, v = tile(), tile()
    dP = torch.zeros((prows * kmax, 128), dtype=torch.float32, device=device)
    ptr = lambda a: a.data_ptr()
    flat = dict(N=1, T=rows, max_workgroups=max_workgroups)
    base = dict(cond_hop=hop, cond_offset=hop // 2, proj_row_stride=128, d_proj_row_stride=128, max_workgroups=max_workgroups, dilation=d,
                next_dilation=next_dilation, cu_rows=ptr(cu_r), cu_frames=ptr(cu_f), n=n, rows=rows, proj_rows=prows)
    ws = nan(lib.pwv_train_workspace_bytes(ctypes.byref(_lib.TrainArgs(**flat))) // 4)
    assert ws.numel() > 0
    out = {k: nan(*c[k].shape) for k in (TO.LAYER_LAST if last else TO.LAYER_RESIDUAL) if k not in ('x', 'P')}
    stream = torch.cuda.current_stream().cuda_stream
    common = dict(base, x=ptr(x), proj=ptr(t['P']), filter=ptr(t['filter']), gate=ptr(t['gate']), u=ptr(u), v=ptr(v), d_proj=ptr(dP),
                  d_filter=ptr(out['filter']), d_gate=ptr(out['gate']), workspace=ptr(ws), workspace_bytes=ws.numel() * 4)
    if last:
        o, d_o = tile(), tile()
        a = _lib.TrainVarlenArgs(form=_lib.TRAIN_LAST, x_out=ptr(o), **{k: val for k, val in common.items() if k in base or k in ('x', 'proj', 'filter', 'gate')})
        _lib.check(lib.pwv_train_varlen_layer_fwd_f32(ctypes.byref(a), stream), 'varlen layer_fwd')
        head = dict(skip=ptr(t['skip']), skip_bias=ptr(t['skip_bias']), post1=ptr(t['post1']), post1_bias=ptr(t['post1_bias']), post2=ptr(t['post2']),
                    post2_bias=ptr(t['post2_bias']))
        a = _lib.TrainArgs(x=ptr(o), d_out=ptr(t['dy']), d_o_out=ptr(d_o), d_skip=ptr(out['skip']), d_skip_bias=ptr(out['skip_bias']),
                           d_post1=ptr(out['post1']), d_post1_bias=ptr(out['post1_bias']), d_post2=ptr(out['post2']), d_post2_bias=ptr(out['post2_bias']),
                           workspace=ptr(ws), workspace_bytes=ws.numel() * 4, **flat, **head)
        _lib.check(lib.pwv_train_head_bwd_f32(ctypes.byref(a), stream), 'head_bwd')
        a = _lib.TrainVarlenArgs(form=_lib.TRAIN_LAST, d_o=ptr(d_o), **common)
    else:
        # the gradient for the layer's output as the layer above would leave it: U = g, V = 0 unless given
        gu = _dev(TO.to_tile32(c['g'] if g is None else g), device)
        gv = torch.zeros_like(gu) if v_next is None else _dev(TO.to_tile32(v_next), device)
        a = _lib.TrainVarlenArgs(form=_lib.TRAIN_RESIDUAL, dense=ptr(t['dense']), u_next=ptr(gu), v_next=ptr(gv), d_dense=ptr(out['dense']),
                                 d_dense_bias=ptr(out['dense_bias']), **common)
    _lib.check(lib.pwv_train_varlen_layer_bwd_f32(ctypes.byref(a), stream), 'varlen layer_bwd')
    torch.cuda.synchronize()
    U = TO.from_tile32(u.cpu().numpy(), rows, 64)
    V = TO.from_tile32(v.cpu().numpy(), rows, 64)
    dx = U.astype(np.float64)
    for r0, T in zip(cu_rows, lengths):
        if d < T:
            dx[r0:r0 + T - d] += V[r0 + d:r0 + T]
    res = {k: val.cpu().numpy().astype(np.float64) for k, val in out.items()}
    res['x'] = dx
    res['P'] = dP.cpu().numpy().astype(np.float64).reshape(prows, kmax, 128).sum(axis=1)
    res['raw'] = (U, V)
    return res


@functools.lru_cache(maxsize=None)
def _layer_reference(d, last, dense=False):
    c = VO.layer_case(d, lengths=tuple(VO.DENSE[0]), hop=VO.DENSE[1]) if dense else VO.layer_case(d)
    g64, g32 = VO.layer_grads(c, last, torch.float64), VO.layer_grads(c, last, torch.float32)
    return c, g64, max(TO.rel_err(g32[k], g64[k]) for k in g64 if np.abs(g64[k]).max() > 0)


def _check_layer(got, g64, e32, what):
    for k, want in g64.items():
        assert np.isfinite(got[k]).all(), k
        if np.abs(want).max() == 0:
            assert np.abs(got[k]).max() == 0, k
            continue
        err = TO.rel_err(got[k], want)
        print('%s %s err %.3g (E32 %.3g)' % (what, k, err, e32))
        assert err <= MARGIN * e32, (what, k, err, e32)


@pytest.mark.parametrize('last', [False, True], ids=['residual', 'last_head'])
@pytest.mark.parametrize('d', DILATIONS)
def test_packed_layer_backward_matches_float64_autograd(gpu, d, last):
    """Every output of the packed layer backward -- the input gradient assembled from U and V, dP with its slots added, every weight
    and bias gradient -- against float64 autograd of that layer run utterance by utterance, within 8 x the error of float32 autograd."""
    c, g64, e32 = _layer_reference(d, last)
    got = _layer_backward(c, last, gpu)
    _check_layer(got, g64, e32, 'd=%d %s' % (d, 'last' if last else 'residual'))
    if d >= max(VO.LENGTHS):       # no row has a look-back: the tap at t - d sees zeros only
        assert np.abs(got['filter'][0]).max() == 0 and np.abs(got['gate'][0]).max() == 0


@pytest.mark.parametrize('last', [False, True], ids=['residual', 'last_head'])
def test_packed_layer_backward_with_four_utterances_in_a_unit(gpu, last):
    """Utterances of 40, 8, 8, 24 and 16 samples at hop 8: rows 32 .. 63 -- one unit -- hold parts of four of them (the frames, 8 rows from
    t = 8 f - 4 on, straddle the unit edges: both dP slots are in use)."""
    for d in (1, 3):
        c, g64, e32 = _layer_reference(d, last, dense=True)
        _check_layer(_layer_backward(c, last, gpu), g64, e32, 'dense d=%d' % d)


def test_packed_layer_backward_keeps_utterances_apart(gpu):
    """Another g for utterance 1 -- the 16 samples that share unit 6 with the end of utterance 0 -- leaves U and V of every other
    utterance the same bits, and changes its own."""
    for d in (1, 48):
        c = VO.layer_case(d)
        g2 = c['g'].copy()
        a0, a1 = VO.CU_ROWS[1], VO.CU_ROWS[2]
        g2[a0:a1] = np.random.RandomState(99).randn(a1 - a0, 64).astype(np.float32)
        a, b = _layer_backward(c, False, gpu), _layer_backward(c, False, gpu, g=g2)
        others = np.r_[0:a0, a1:VO.ROWS]
        for i in (0, 1):
            assert np.array_equal(a['raw'][i][others], b['raw'][i][others])
        assert not np.array_equal(a['raw'][0][a0:a1], b['raw'][0][a0:a1])
        assert np.array_equal(a['x'][others], b['x'][others]) and not np.array_equal(a['x'][a0:a1], b['x'][a0:a1])


# ---- the whole model ------------------------------------------------------------------------------------------------------------------
def _model(device, lengths=tuple(VO.LENGTHS)):
    from pwv_amd.models import IAFVocoder
    from pwv_amd.variables import VariableStore
    cfg, w, mels, zs, wavs = VO.problem(lengths)
    set_hparams(cfg)
    store = VariableStore(device=device)
    store.load_dict(w)
    model = IAFVocoder(batch_size=1, length=max(lengths), store=store, precision='f32')
    return (model, store, [_dev(a[0, :, 0], device) for a in wavs], [_dev(a[0], device) for a in mels], [_dev(a[0], device) for a in zs])


def _check_grads(grads, ref, what=''):
    g64, bar = ref['g64'], MARGIN * ref['E32']
    assert sorted(grads) == sorted(g64)
    worst, zeros = 0.0, 0
    for k, want in g64.items():
        got = grads[k].detach().cpu().numpy().astype(np.float64)
        if want is None:
            assert got.shape == TO.problem()[1][k].shape and np.abs(got).max() == 0, k        # exact zeros for what the model never reads
            zeros += 1
            continue
        assert got.shape == want.shape and np.isfinite(got).all(), k
        err = TO.rel_err(got, want)
        worst = max(worst, err)
        assert err <= bar, (what, k, err, bar)
    print('%s worst gradient err %.3g (E32 %.3g, bar %.3g)' % (what, worst, ref['E32'], bar))
    assert zeros == 32 and len(g64) - zeros == 149


def _check_preds(preds, ref):
    assert [tuple(p.shape) for p in preds] == [(T, 1) for T in VO.LENGTHS]
    for p, want in zip(preds, ref['preds']):
        assert np.abs(p.detach().cpu().numpy().astype(np.float64).reshape(-1) - want).max() <= TOL_F32


def _same(a, b):
    assert torch.equal(a[0], b[0]) and all(torch.equal(p, q) for p, q in zip(a[1], b[1]))
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k


@pytest.mark.parametrize('max_workgroups', [1, 3, 0])
def test_packed_model_gradients_match_float64_autograd(gpu, max_workgroups):
    """All 149 gradients, the loss and the predictions of the small model on the packed batch against float64 autograd of the utterances
    run one by one; exact zeros for the 32 unread variables; 1, 3 and the default number of partials, each bit-identical to its
    repetition."""
    from pwv_amd import train as TR
    model, _, wavs, mels, zs = _model(gpu)
    ref = VO.reference()
    runs = []
    for _ in range(2):
        runs.append(TR.loss_and_grad_varlen(model, wavs, mels, z=zs, max_workgroups=max_workgroups))
        torch.cuda.synchronize()
    loss, preds, grads = runs[0]
    assert loss.dim() == 0 and loss.is_cuda
    _check_grads(grads, ref, 'max_workgroups=%d' % max_workgroups)
    _check_preds(preds, ref)
    assert abs(float(loss) - ref['terms']['total']) <= 2e-6 * max(1.0, abs(ref['terms']['total']))
    _same(runs[0], runs[1])


def test_equal_lengths_give_the_bits_of_the_uniform_batch(gpu):
    """Two utterances of 208 samples with the z of tests.train_oracle: loss_and_grad_varlen returns the bits of loss_and_grad for the
    prediction and every gradient."""
    from pwv_amd import train as TR
    from pwv_amd.models import IAFVocoder
    from pwv_amd.variables import VariableStore
    cfg, w, mel, z, wav = TO.problem()
    set_hparams(cfg)
    store = VariableStore(device=gpu)
    store.load_dict(w)
    model = IAFVocoder(batch_size=TO.N, length=TO.T, store=store, precision='f32')
    wav, mel, z = _dev(wav, gpu), _dev(mel, gpu), _dev(z, gpu)
    loss, pred, grads = TR.loss_and_grad(model, wav, mel, z=z)
    vloss, vpreds, vgrads = TR.loss_and_grad_varlen(model, [wav[i, :, 0] for i in range(TO.N)], [mel[i] for i in range(TO.N)],
                                                    z=[z[i] for i in range(TO.N)])
    torch.cuda.synchronize()
    assert torch.equal(loss, vloss)
    for i in range(TO.N):
        assert torch.equal(pred[i], vpreds[i])
    assert sorted(grads) == sorted(vgrads)
    for k in grads:
        assert torch.equal(grads[k], vgrads[k]), k


def test_a_packed_prediction_is_the_utterance_alone(gpu):
    """preds[i] of the packed batch = the prediction of utterance i trained alone with the same z, bit for bit: the kernels are
    row-local, and so is the frame rate -- P comes from the project's own GEMM, whose sum over K has one order whatever the number of
    rows (with torch.matmul it differed by one or two float32 ulps: the BLAS picks its kernel by the row count)."""
    from pwv_amd import train as TR
    model, _, wavs, mels, zs = _model(gpu)
    _, preds, _ = TR.loss_and_grad_varlen(model, wavs, mels, z=zs)
    worst = []
    for i in range(len(wavs)):
        _, alone, _ = TR.loss_and_grad_varlen(model, [wavs[i]], [mels[i]], z=[zs[i]])
        torch.cuda.synchronize()
        worst.append(float((preds[i] - alone[0]).abs().max()))
    print('largest |packed - alone| per utterance', ' '.join('%.3g' % v for v in worst))
    assert worst == [0.0] * len(wavs), worst


def test_a_packed_prediction_does_not_depend_on_its_companions(gpu):
    """Other noise, mels and wavs in utterances 0, 1 and 3 (the same lengths) leave the prediction of utterance 2 the same bits: no
    kernel reads across a boundary, in the unit utterance 2 shares with utterance 3 either."""
    from pwv_amd import train as TR
    model, _, wavs, mels, zs = _model(gpu)
    _, preds, _ = TR.loss_and_grad_varlen(model, wavs, mels, z=zs)
    g = torch.Generator(device='cpu').manual_seed(5)
    other = lambda t: torch.randn(t.shape, generator=g).to(t.device) * 0.5
    keep = 2
    wavs2, mels2, zs2 = ([t if i == keep else other(t) for i, t in enumerate(ts)] for ts in (wavs, mels, zs))
    _, preds2, _ = TR.loss_and_grad_varlen(model, wavs2, mels2, z=zs2)
    torch.cuda.synchronize()
    assert torch.equal(preds[keep], preds2[keep])
    assert all(not torch.equal(preds[i], preds2[i]) for i in range(len(wavs)) if i != keep)


def test_seeds_give_every_utterance_its_own_stream(gpu):
    """seeds=: utterance i's prediction does not depend on its companions, and equals what z = the stream of IAFVocoder(1, T_i) with
    noise_seed = seeds[i] gives."""
    from pwv_amd import engine
    from pwv_amd import train as TR
    model, _, wavs, mels, _ = _model(gpu)
    seeds = [11, 12, 13, 14]
    _, preds, _ = TR.loss_and_grad_varlen(model, wavs, mels, seeds=seeds)
    zs = [engine.logistic_noise_op((T, 1), gpu, seed=s, offset=0) for T, s in zip(VO.LENGTHS, seeds)]
    _, want, _ = TR.loss_and_grad_varlen(model, wavs, mels, z=zs)
    torch.cuda.synchronize()
    for p, q in zip(preds, want):
        assert torch.equal(p, q)
    with pytest.raises(ValueError, match='exclude'):
        TR.loss_and_grad_varlen(model, wavs, mels, seeds=seeds, z=zs)


# ---- the loss head through ctypes -----------------------------------------------------------------------------------------------------
def _loss_head(preds, ys, win, hop, wl1, wp, device):
    """One pwv_train_loss_varlen_f32 on lists of float32 numpy [T_i]; d_out, result and workspace start as NaN.  Returns (d_out float32
    [rows], result float64 [n, 4]) as CPU tensors."""
    from pwv_amd import _lib
    lib = _lib.lib()
    n, rows = len(preds), sum(len(p) for p in preds)
    cu = _dev(np.asarray([0] + list(np.cumsum([len(p) for p in preds])), dtype=np.int32), device)
    a = _lib.TrainLossVarlenArgs(n=n, rows=rows, win_length=win, hop_length=hop, weight_l1=wl1, weight_power=wp)
    need = int(lib.pwv_train_loss_varlen_workspace_bytes(ctypes.byref(a)))
    assert need > 0 and need % 8 == 0, lib.pwv_last_error()
    nan = lambda shape, dtype: torch.full(shape, float('nan'), dtype=dtype, device=device)
    p, t_y = _dev(np.concatenate(preds), device), _dev(np.concatenate(ys), device)
    d_out, table, work = nan((rows,), torch.float32), nan((n, 4), torch.float64), nan((need // 8,), torch.float64)
    a.out, a.y, a.cu_rows, a.d_out, a.result, a.workspace, a.workspace_bytes = (p.data_ptr(), t_y.data_ptr(), cu.data_ptr(), d_out.data_ptr(),
                                                                               table.data_ptr(), work.data_ptr(), need)
    _lib.check(lib.pwv_train_loss_varlen_f32(ctypes.byref(a), torch.cuda.current_stream().cuda_stream), 'pwv_train_loss_varlen_f32')
    torch.cuda.synchronize()
    return d_out.cpu(), table.cpu()


def test_packed_loss_head_matches_float64(gpu):
    """(win, hop) = (48, 16) on the packed batch -- the 16-sample utterance has no frame: d_out against float64 within 8 E32 of float32
    autograd, the table within 1e-10 of score.score_reference per utterance, weight 0 = the L1 alone within one float32 ulp of
    sign / sum T_i, every run bit-identical to its repetition."""
    from pwv_amd.score import score_reference
    win, hop = WIN, VO.HOP
    preds, ys = VO.head_case()
    assert [PO.frame_count(T, win, hop) for T in VO.LENGTHS] == [11, 0, 1, 7]
    table64 = score_reference(preds, ys, win, hop)
    assert table64[1, 3] == 0 and table64[0, 3] == 11 * 33
    for wl1, wp in ((0.0, 1.0), (1.0, 1.0)):
        g64, g32 = (VO.head_grad(preds, ys, win, hop, wl1, wp, dt) for dt in (torch.float64, torch.float32))
        e32 = TO.rel_err(g32, g64)
        d, table = _loss_head(preds, ys, win, hop, wl1, wp, gpu)
        assert torch.isfinite(d).all() and torch.isfinite(table).all()
        err = TO.rel_err(d.numpy(), g64)
        print('weights (%g, %g) d_out err %.3g (E32 %.3g)' % (wl1, wp, err, e32))
        assert err <= MARGIN * e32, (err, e32)
        assert (np.abs(table.numpy() - table64) <= 1e-10 * np.abs(table64)).all()
        if wl1 == 0:            # the utterance without a frame, and the tail no frame covers: written, and zero
            assert (d.numpy()[VO.CU_ROWS[1]:VO.CU_ROWS[2]] == 0).all()
        d2, table2 = _loss_head(preds, ys, win, hop, wl1, wp, gpu)
        assert torch.equal(d, d2) and torch.equal(table, table2)
    d, table = _loss_head(preds, ys, win, hop, 1.0, 0.0, gpu)
    want = np.sign(np.concatenate(preds).astype(np.float64) - np.concatenate(ys)) / VO.ROWS
    assert np.abs(d.numpy().astype(np.float64) - want).max() <= np.spacing(np.float32(1.0 / VO.ROWS))
    assert (np.sign(d.numpy()) == np.sign(want)).all()
    l1_table = table64 * [1, 1, 0, 0]
    assert (np.abs(table.numpy() - l1_table) <= 1e-10 * np.abs(l1_table)).all() and (table.numpy()[:, 2:] == 0).all()


def test_packed_loss_head_keeps_utterances_apart(gpu):
    """Other contents in utterances 0, 1 and 3 leave the table row of utterance 2 the same bits, and change theirs."""
    preds, ys = VO.head_case()
    other_p, other_y = VO.head_case(seed=7)
    p2, y2 = [other_p[0], other_p[1], preds[2], other_p[3]], [other_y[0], other_y[1], ys[2], other_y[3]]
    _, ta = _loss_head(preds, ys, WIN, VO.HOP, 1.0, 1.0, gpu)
    _, tb = _loss_head(p2, y2, WIN, VO.HOP, 1.0, 1.0, gpu)
    assert torch.equal(ta[2], tb[2])
    for i in (0, 1, 3):
        assert not torch.equal(ta[i, 0], tb[i, 0])


@pytest.mark.parametrize('weights', [(1.0, 1.0), (0.0, 1.0), (1.0, 0.0)], ids=['both', 'power', 'l1'])
@pytest.mark.parametrize('T,win,hop', [(208, 48, 16), (100, 16, 24), (210, 48, 20), (4400, 48, 16)])
def test_equal_lengths_give_the_bits_of_the_uniform_loss_head(gpu, T, win, hop, weights):
    """Two utterances of equal length T through pwv_train_loss_varlen_f32 with cu_rows = [0, T, 2 T] and through pwv_train_loss_f32: d_out
    and the [n, 4] table are the same bits.  Both forms divide 4 w by the same integer n F B and weight_l1 by the same n T, add a
    sample's frames in ascending f and an utterance's partials in the same order.  The shapes: nfft above win; hop above win (gaps and a
    tail); a tail behind the last frame; 273 frames and 5 tiles per utterance (the strided partial sums make a second pass, the gather
    crosses tile boundaries).  The data: train_power_oracle.case(T, 2); at T = 4400 with seed 1, since none of the 50 draws of seed 0
    keeps all 8800 samples clear of a zero difference, which case() insists on."""
    from tests.test_gpu_train_power import _loss_head as _uniform_loss_head
    pred, y = PO.case(T, 2, seed=1 if T == 4400 else 0)
    wl1, wp = weights
    d_u, table_u = _uniform_loss_head(pred, y, win, hop, wl1, wp, gpu)
    d_p, table_p = _loss_head(list(pred), list(y), win, hop, wl1, wp, gpu)
    assert torch.isfinite(d_u).all() and torch.isfinite(table_u).all()
    assert torch.equal(d_p, d_u.reshape(-1)) and torch.equal(table_p, table_u)


@pytest.fixture()
def small_power(gpu):
    from pwv_amd.hparam import hparam as hp
    out = _model(gpu)
    hp.signal.win_length = WIN
    yield out
    hp.set_hparam_yaml('default')


def test_packed_model_gradients_with_the_power_loss(small_power):
    """All 149 gradients of L1 + w * power on the packed batch at the weight of tests/test_gpu_train_power.py (the balanced weight of
    tests.train_power_oracle), likelihood, power and total against float64."""
    from pwv_amd import train as TR
    model, _, wavs, mels, zs = small_power
    w = PO.balanced_weight()
    ref = VO.reference(w, WIN)
    terms = {}
    loss, preds, grads = TR.loss_and_grad_varlen(model, wavs, mels, z=zs, power_weight=w, terms=terms)
    torch.cuda.synchronize()
    _check_grads(grads, ref, 'L1 + %.4g power' % w)
    _check_preds(preds, ref)
    for k in ('likelihood', 'power', 'total'):
        print('%s %.9g (float64 %.9g)' % (k, float(terms[k]), ref['terms'][k]))
        assert abs(float(terms[k]) - ref['terms'][k]) <= 2e-6 * abs(ref['terms'][k]), k
    assert torch.equal(loss, terms['total'])


def test_packed_training_trains(gpu):
    """Five Trainer.step_varlen calls at lr 2e-4 on the fixed packed batch: the loss falls at every step and follows the float64
    trajectory; the shadows within 8 D32, D32 = the largest |shadow - shadow64| of the same restatement run in float32
    (tests/test_gpu_train.py, test_training_trains)."""
    from pwv_amd import train as TR
    ref_losses, ref_shadow = VO.trajectory(5)
    losses32, shadow32 = VO.trajectory(5, single=True)
    d32 = max(float(np.abs(shadow32[k].astype(np.float64) - ref_shadow[k]).max()) for k in ref_shadow)
    # the bar of "follows": built like D32 -- L32 = the largest distance of the float32 restatement's losses from the float64 ones, and
    # never below one float32 ulp of the loss, which any float32 mean is rounded to
    l32 = max(max(abs(a - b) for a, b in zip(losses32, ref_losses)), float(np.spacing(np.float32(ref_losses[0]))))
    model, store, wavs, mels, zs = _model(gpu)
    tr = TR.Trainer(model, lr=TO.LR, beta2=TO.BETA2, ema_decay=TO.DECAY)
    losses = [float(tr.step_varlen(wavs, mels, z=zs)) for _ in range(5)]
    assert tr.steps == 5
    losses.append(float(TR.loss_and_grad_varlen(model, wavs, mels, z=zs)[0]))
    print('gpu  ', ' '.join('%.6f' % v for v in losses))
    print('fp64 ', ' '.join('%.6f' % v for v in ref_losses))
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    print('largest difference of the trajectories %.3g (L32 %.3g, bar %.3g)' % (max(abs(a - b) for a, b in zip(losses, ref_losses)), l32, MARGIN * l32))
    for a, b in zip(losses, ref_losses):
        assert abs(a - b) <= MARGIN * l32, (losses, ref_losses, l32)
    assert losses[0] - losses[-1] >= 0.5 * (ref_losses[0] - ref_losses[-1])
    shadows = tr.shadows()
    assert sorted(shadows) == sorted(ref_shadow)
    errs = {k: float(np.abs(shadows[k].cpu().numpy().astype(np.float64) - want).max()) for k, want in ref_shadow.items()}
    print('largest shadow difference %.3g (D32 %.3g, bar %.3g)' % (max(errs.values()), d32, MARGIN * d32))
    for k, err in errs.items():
        assert err <= MARGIN * d32, (k, err, d32)


def test_guarded_packed_loss_and_grad(gpu):
    """One loss_and_grad_varlen with three partials inside poisoned, guard-banded buffers: no mark in a band, no NaN in loss, preds or
    any gradient."""
    from pwv_amd import engine
    from pwv_amd import train as TR
    with guarded(TR, engine) as g:
        model, _, wavs, mels, zs = _model(gpu)
        loss, preds, grads = TR.loss_and_grad_varlen(model, wavs, mels, z=zs, max_workgroups=3)
        torch.cuda.synchronize()
        g.check()
        assert any('train.py' in s for s in g.sites())
        assert torch.isfinite(loss).all() and all(torch.isfinite(p).all() for p in preds)
        for k, v in grads.items():
            assert torch.isfinite(v).all(), k
        _check_grads(grads, VO.reference(), 'guarded')


def test_train_cli_varlen_then_generate(gpu, tmp_path):
    """`python -m pwv_amd.train train/small_varlen --varlen --steps=3` writes model-3.npz and prints three finite losses; `generate`
    loads the checkpoint."""
    env = dict(os.environ, PWV_LOGDIR=str(tmp_path), PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = subprocess.run([sys.executable, '-m', 'pwv_amd.train', 'train/small_varlen', '--varlen', '--steps=3', '--seed=4'], cwd=ROOT, env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:]
    lines = [l for l in out.stdout.splitlines() if 'loss/likelihood' in l]
    assert len(lines) == 3 and all(np.isfinite(float(l.split()[-1])) for l in lines), out.stdout[-2000:]
    assert (tmp_path / 'model-3.npz').exists()
    gen = subprocess.run([sys.executable, '-m', 'pwv_amd.generate', 'train/small_varlen'], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, text=True, timeout=300)
    assert gen.returncode == 0, gen.stdout[-3000:]
    assert 'No checkpoint found' not in gen.stdout
    pred = np.load(str(tmp_path / 'pred_wav.npy'))
    assert pred.shape[1] == 1600 and np.isfinite(pred).all() and np.abs(pred).max() > 0
