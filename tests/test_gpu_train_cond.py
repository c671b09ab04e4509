"""GPU: training the transposed-conv conditioning (pwv_amd/train.py -> pwv_train_cond_*, csrc/pwv_train_cond.hip) against float64
autograd on the CPU (tests/train_cond_oracle.py): one layer with a per-sample condition through the C ABI at every kind of dilation,
both forms, two channel counts and both condition layouts; the whole small model at hop 80; the partials of the weight-gradient
reductions; guarded buffers; five optimiser steps; `python -m pwv_amd.train train/small_tran` -> `generate`.

The bars are built as in tests/test_gpu_train.py: err(v) = max|g - g64| / max|g64| per variable, E32 = the largest err of float32
autograd on the CPU of the same function, computed at run time, and the kernels must stay within 8 E32.  A forward output is held to the
project's fp32 bar, TOL_F32."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import train_cond_oracle as CO
from tests import train_oracle as TO
from tests.guarded import Guard, guarded
from tests.util import TOL_F32, set_hparams

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 8
DILATIONS = (1, 3, 64, 256)             # within a tile, odd, across tiles, larger than T
CHANNELS = (80, 34)                     # the reference's; two whole 32-blocks and two channels of a third are no multiple of anything
HOP = CO.HOP


# ---- one layer through ctypes ---------------------------------------------------------------------------------------------------------
def _layer_run(c, last, device, margin=0, max_workgroups=0, alloc=None, accumulate_twice=False):
    """The layer forward and backward of include/pwv_hip_train_cond.h (in the last form with the head backward between them) on one net.
    `margin`: 0 = the condition rows of an utterance follow each other (cond_utt_rows = T); HOP = cond and d_cond are [N, T + HOP, C]
    tensors with NaN margins of HOP / 2 rows, entered through a pointer to sample 0 (cond_utt_rows = T + HOP).  `alloc(shape)` makes an
    uninitialised float32 device buffer (default: NaN-filled).  Returns float64 numpy gradients (x assembled with its look-ahead), the
    forward output, and the raw u, v, d_cond."""
    from pwv_amd import _lib
    lib = _lib.lib()
    N, T, d, C = c['x'].shape[0], c['x'].shape[1], c['d'], c['C']
    rows = N * T
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    nan = alloc or (lambda *shape: torch.full(shape, float('nan'), dtype=torch.float32, device=device))
    tile = lambda: nan(((rows + 31) // 32) * 32 * 64)
    names = CO.LAYER_LAST if last else CO.LAYER_RESIDUAL
    t = {k: dev(c[k]) for k in names if k not in ('x', 'cond')}
    t['dy'] = dev(c['dy'])
    x = dev(TO.to_tile32(c['x'].reshape(rows, 64)))
    utt = T + margin
    cond_full = np.full((N, utt, C), np.nan, dtype=np.float32)
    cond_full[:, margin // 2: margin // 2 + T] = c['cond']
    cond, d_cond = dev(cond_full), nan(N, utt, C)
    skip = (margin // 2) * C * 4
    out = {k: nan(*c[k].shape) for k in names if k not in ('x', 'cond')}
    ptr = lambda a: a.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    base = dict(N=N, T=T, max_workgroups=max_workgroups, dilation=d, next_dilation=1)
    cbase = dict(base, cond=ptr(cond) + skip, cond_channels=C, cond_row_stride=C, cond_utt_rows=utt, x=ptr(x), filter=ptr(t['filter']),
                 gate=ptr(t['gate']), gc_filter=ptr(t['gc_filter']), gc_gate=ptr(t['gc_gate']), filter_bias=ptr(t['filter_bias']),
                 gate_bias=ptr(t['gate_bias']))
    ws = nan(lib.pwv_train_cond_workspace_bytes(ctypes.byref(_lib.TrainCondArgs(**cbase))) // 4)
    assert ws.numel() > 0
    u, v, fwd = tile(), tile(), tile()
    bwd = dict(cbase, u=ptr(u), v=ptr(v), d_cond=ptr(d_cond) + skip, d_filter=ptr(out['filter']), d_gate=ptr(out['gate']),
               d_gc_filter=ptr(out['gc_filter']), d_gc_gate=ptr(out['gc_gate']), d_filter_bias=ptr(out['filter_bias']),
               d_gate_bias=ptr(out['gate_bias']), workspace=ptr(ws), workspace_bytes=ws.numel() * 4)
    if last:
        d_o = tile()
        a = _lib.TrainCondArgs(form=_lib.TRAIN_LAST, x_out=ptr(fwd), **cbase)
        _lib.check(lib.pwv_train_cond_layer_fwd_f32(ctypes.byref(a), stream), 'cond_layer_fwd')
        head = dict(skip=ptr(t['skip']), skip_bias=ptr(t['skip_bias']), post1=ptr(t['post1']), post1_bias=ptr(t['post1_bias']), post2=ptr(t['post2']),
                    post2_bias=ptr(t['post2_bias']))
        a = _lib.TrainArgs(x=ptr(fwd), d_out=ptr(t['dy']), d_o_out=ptr(d_o), d_skip=ptr(out['skip']), d_skip_bias=ptr(out['skip_bias']),
                           d_post1=ptr(out['post1']), d_post1_bias=ptr(out['post1_bias']), d_post2=ptr(out['post2']), d_post2_bias=ptr(out['post2_bias']),
                           workspace=ptr(ws), workspace_bytes=ws.numel() * 4, **base, **head)
        _lib.check(lib.pwv_train_head_bwd_f32(ctypes.byref(a), stream), 'head_bwd')
        a = _lib.TrainCondArgs(form=_lib.TRAIN_LAST, d_o=ptr(d_o), **bwd)
    else:
        a = _lib.TrainCondArgs(form=_lib.TRAIN_RESIDUAL, x_out=ptr(fwd), dense=ptr(t['dense']), dense_bias=ptr(t['dense_bias']), **cbase)
        _lib.check(lib.pwv_train_cond_layer_fwd_f32(ctypes.byref(a), stream), 'cond_layer_fwd')
        # the gradient for the layer's output as the layer above would leave it: U = g, V = 0, taken with next_dilation 1
        gu = dev(TO.to_tile32(c['g'].reshape(rows, 64)))
        gv = torch.zeros_like(gu)
        a = _lib.TrainCondArgs(form=_lib.TRAIN_RESIDUAL, dense=ptr(t['dense']), u_next=ptr(gu), v_next=ptr(gv), d_dense=ptr(out['dense']),
                               d_dense_bias=ptr(out['dense_bias']), **bwd)
    _lib.check(lib.pwv_train_cond_layer_bwd_f32(ctypes.byref(a), stream), 'cond_layer_bwd')
    first = None
    if accumulate_twice:
        torch.cuda.synchronize()
        first = d_cond.cpu()
        a.d_cond_accumulate = 1
        _lib.check(lib.pwv_train_cond_layer_bwd_f32(ctypes.byref(a), stream), 'cond_layer_bwd')
    torch.cuda.synchronize()
    U = TO.from_tile32(u.cpu().numpy(), rows, 64).reshape(N, T, 64).astype(np.float64)
    V = TO.from_tile32(v.cpu().numpy(), rows, 64).reshape(N, T, 64).astype(np.float64)
    dx = U.copy()
    if d < T:
        dx[:, :T - d] += V[:, d:]
    res = {k: val.cpu().numpy().astype(np.float64) for k, val in out.items()}
    res['x'] = dx
    dc = d_cond.cpu()
    lo = margin // 2
    if margin:          # the margins belong to nobody: still the NaN they were filled with
        assert torch.isnan(dc[:, :lo]).all() and torch.isnan(dc[:, lo + T:]).all()
    res['cond'] = dc[:, lo:lo + T].numpy().astype(np.float64)
    res['fwd'] = TO.from_tile32(fwd.cpu().numpy(), rows, 64).reshape(N, T, 64).astype(np.float64)
    res['raw'] = (TO.from_tile32(u.cpu().numpy(), rows, 64).reshape(N, T, 64), TO.from_tile32(v.cpu().numpy(), rows, 64).reshape(N, T, 64),
                  dc[:, lo:lo + T].numpy())
    res['first'] = first
    return res


def _check_layer(got, g64, fwd64, e32, what):
    for k, want in g64.items():
        assert np.isfinite(got[k]).all(), (what, k)
        if np.abs(want).max() == 0:
            assert np.abs(got[k]).max() == 0, (what, k)
            continue
        err = TO.rel_err(got[k], want)
        print('%s %s err %.3g (E32 %.3g)' % (what, k, err, e32))
        assert err <= MARGIN * e32, (what, k, err, e32)
    assert np.abs(got['fwd'] - fwd64).max() <= TOL_F32, what


@pytest.mark.parametrize('margin', [0, HOP], ids=['cropped', 'uncropped'])
@pytest.mark.parametrize('C', CHANNELS)
@pytest.mark.parametrize('last', [False, True], ids=['residual', 'last_head'])
@pytest.mark.parametrize('d', DILATIONS)
def test_cond_layer_matches_float64_autograd(gpu, d, last, C, margin):
    """400 rows = 12.5 units, the last one half full, the utterance boundary inside unit 6: the forward output and every output of the
    backward -- the input gradient, d_cond, the gradients of filter, gate, gc_filter, gc_gate, both biases and dense (or the head) --
    against float64 autograd of that one layer, within 8 x the error of float32 autograd of the same layer.  `uncropped`: cond and d_cond
    are entered through a pointer into a [N, T + 80, C] tensor whose margins are NaN and stay NaN."""
    c, g64, fwd64, e32 = CO.layer_reference(d, C, last)
    got = _layer_run(c, last, gpu, margin=margin)
    _check_layer(got, g64, fwd64, e32, 'd=%d %s C=%d margin=%d' % (d, 'last' if last else 'residual', C, margin))
    if d >= CO.LT:      # no row has a look-back: the tap at t - d sees zeros only
        assert np.abs(got['filter'][0]).max() == 0 and np.abs(got['gate'][0]).max() == 0


@pytest.mark.parametrize('C', CHANNELS)
@pytest.mark.parametrize('last', [False, True], ids=['residual', 'last_head'])
def test_d_cond_accumulates(gpu, last, C):
    """d_cond_accumulate = 1 after d_cond_accumulate = 0 on the same buffer: bit for bit twice the first result (x + x is exact)."""
    c = CO.layer_case(3, C)
    got = _layer_run(c, last, gpu, margin=HOP, accumulate_twice=True)
    lo = HOP // 2
    first = got['first'][:, lo:lo + CO.LT].numpy()
    assert np.isfinite(first).all() and np.abs(first).max() > 0
    assert np.array_equal(got['raw'][2], 2 * first)


@pytest.mark.parametrize('last', [False, True], ids=['residual', 'last_head'])
def test_cond_layer_grid_and_determinism(gpu, last):
    """max_workgroups 1, 3 and the default: u, v and d_cond are the same bits at every grid (a row belongs to one unit); the weight
    gradients -- sums of 1, 3 or 13 partials -- agree with float64 under the bar at each and are bit-identical run to run."""
    d, C = 64, 34
    c, g64, fwd64, e32 = CO.layer_reference(d, C, last)
    runs = {}
    for mw in (1, 3, 0):
        a, b = _layer_run(c, last, gpu, max_workgroups=mw), _layer_run(c, last, gpu, max_workgroups=mw)
        _check_layer(a, g64, fwd64, e32, 'max_workgroups=%d' % mw)
        for k in g64:
            assert np.array_equal(a[k], b[k]), (mw, k)
        runs[mw] = a
    for mw in (3, 0):
        for i in range(3):
            assert np.array_equal(runs[1]['raw'][i], runs[mw]['raw'][i]), (mw, i)
        assert np.array_equal(runs[1]['fwd'], runs[mw]['fwd'])


def test_cond_layer_in_guarded_buffers(gpu):
    """One forward and backward of either form with every output and the workspace inside poisoned, guard-banded allocations: no NaN is
    left in an output (every element the header promises is written) and no band is touched."""
    for last in (False, True):
        for C in CHANNELS:
            g = Guard()
            alloc = lambda *shape: g.allocate(shape, torch.float32, gpu, None)
            c, g64, fwd64, e32 = CO.layer_reference(3, C, last)
            got = _layer_run(c, last, gpu, max_workgroups=3, alloc=alloc)
            g.check()
            assert len(g.allocations) >= 12
            _check_layer(got, g64, fwd64, e32, 'guarded C=%d' % C)
            assert np.isfinite(got['cond']).all() and all(np.isfinite(r).all() for r in got['raw'])


def test_cond_layer_keeps_utterances_apart(gpu):
    """u, v, d_cond and the forward output of utterance 1 -- rows 200 .. 399, which begin at row 8 of unit 6 -- are the same bits when
    the utterance is run alone, where it begins at row 0 of unit 0."""
    for d in (1, 64):
        c = CO.layer_case(d, 80)
        alone = dict(c, **{k: c[k][1:2] for k in ('x', 'cond', 'g', 'dy')})
        for last in (False, True):
            a, b = _layer_run(c, last, gpu), _layer_run(alone, last, gpu)
            for i in range(3):
                assert np.array_equal(a['raw'][i][1], b['raw'][i][0]), (d, last, i)
            assert np.array_equal(a['fwd'][1], b['fwd'][0])


# ---- the whole model ------------------------------------------------------------------------------------------------------------------
def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


@pytest.fixture()
def small(gpu):
    """Sets the hparams of tests.train_cond_oracle's problem (hop 80, transposed-conv conditioning, win_length 160) and yields a factory
    of (model, store, wav, mel, z) on the device."""
    from pwv_amd.hparam import hparam as hp
    from pwv_amd.models import IAFVocoder
    from pwv_amd.variables import VariableStore
    cfg, w, mel, z, wav = CO.problem()

    def make(n=CO.N, first=0):
        set_hparams(cfg)
        hp.signal.win_length = CO.WIN
        store = VariableStore(device=gpu)
        store.load_dict(w)
        sl = slice(first, first + n)
        return IAFVocoder(batch_size=n, length=CO.T, store=store, precision='f32'), store, _dev(wav[sl], gpu), _dev(mel[sl], gpu), _dev(z[sl], gpu)

    yield make
    hp.set_hparam_yaml('default')


def _check_grads(grads, ref, what):
    g64, bar = ref['g64'], MARGIN * ref['E32']
    assert sorted(grads) == sorted(g64)
    worst, zeros = 0.0, 0
    for k, want in g64.items():
        got = grads[k].detach().cpu().numpy().astype(np.float64)
        if want is None:
            assert got.shape == CO.problem()[1][k].shape and np.abs(got).max() == 0, k       # exact zeros for what the model never reads
            zeros += 1
            continue
        assert got.shape == want.shape and np.isfinite(got).all(), k
        err = TO.rel_err(got, want)
        worst = max(worst, err)
        assert err <= bar, (what, k, err, bar)
    print('%s worst gradient err %.3g (E32 %.3g, bar %.3g)' % (what, worst, ref['E32'], bar))
    assert zeros == 32 and len(g64) - zeros == 151          # the 148 of the nets and the three transposed-conv weights
    return worst


def test_model_gradients_match_float64_autograd(small):
    """All 151 gradients -- the three transposed_conv_*_weights among them -- and the loss of the small model (480 rows = 15 units, the
    boundary at 7.5) against float64 autograd, exact zeros for the 32 unused variables, pred within the project's fp32 bar; 1 and 3
    partials per reduction hold the same bar, and a run is bit-identical to its repetition."""
    from pwv_amd import train as TR
    model, _, wav, mel, z = small()
    ref = CO.reference()
    names = ['iaf_vocoder/cond/transposed_conv_%d_weights' % i for i in range(3)]
    assert all(ref['g64'][n] is not None and np.abs(ref['g64'][n]).max() > 0 for n in names) and 'iaf_vocoder/cond/dense' not in ref['g64']
    for mw in (0, 1, 3):
        runs = []
        for _ in range(2):
            loss, pred, grads = TR.loss_and_grad(model, wav, mel, z=z, max_workgroups=mw)
            torch.cuda.synchronize()
            runs.append((loss, pred, grads))
        loss, pred, grads = runs[0]
        assert tuple(pred.shape) == (CO.N, CO.T, 1) and loss.dim() == 0 and loss.is_cuda
        _check_grads(grads, ref, 'max_workgroups=%d' % mw)
        assert abs(float(loss) - ref['loss']) <= 2e-6 * max(1.0, abs(ref['loss']))
        assert np.abs(pred.cpu().numpy().astype(np.float64) - ref['pred']).max() <= TOL_F32
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
        for k in grads:
            assert torch.equal(grads[k], runs[1][2][k]), (mw, k)


def test_pred_of_an_utterance_alone_and_in_the_batch(small):
    """pred of utterance 1 is the same bits alone and as the second of the batch: the conditioning GEMMs and the layer kernels work row
    by row."""
    from pwv_amd import train as TR
    model, _, wav, mel, z = small()
    _, pred, _ = TR.loss_and_grad(model, wav, mel, z=z)
    for i in (0, 1):
        m1, _, w1, mel1, z1 = small(1, i)
        _, alone, _ = TR.loss_and_grad(m1, w1, mel1, z=z1)
        torch.cuda.synchronize()
        assert torch.equal(pred[i], alone[0]), i


def test_model_gradients_with_the_power_loss(small):
    """The same under L1 + w * power at win_length 160 <= T (2 frames of hop 80 per utterance; tests/train_power_oracle.py's
    restatement), w such that both terms' gradients for pred have the same maximum in the float64 reference."""
    from pwv_amd import train as TR
    model, _, wav, mel, z = small()
    ref = CO.reference(True)
    terms = {}
    loss, pred, grads = TR.loss_and_grad(model, wav, mel, z=z, power_weight=ref['w'], terms=terms)
    torch.cuda.synchronize()
    _check_grads(grads, ref, 'L1 + %.4g power' % ref['w'])
    assert np.abs(pred.cpu().numpy().astype(np.float64) - ref['pred']).max() <= TOL_F32
    for k in ('likelihood', 'power', 'total'):
        print('%s %.9g (float64 %.9g)' % (k, float(terms[k]), ref['terms'][k]))
        assert abs(float(terms[k]) - ref['terms'][k]) <= 2e-6 * abs(ref['terms'][k]), k
    assert torch.equal(loss, terms['total'])


def test_guarded_loss_and_grad(gpu, small):
    """One loss_and_grad inside poisoned, guard-banded buffers: no store outside a buffer -- d_cond is entered through a pointer past its
    front margin --, no NaN in pred, loss or any gradient, and the gradients hold the bar."""
    from pwv_amd import engine
    from pwv_amd import train as TR
    with guarded(TR, engine) as g:
        model, _, wav, mel, z = small()
        loss, pred, grads = TR.loss_and_grad(model, wav, mel, z=z, max_workgroups=3)
        torch.cuda.synchronize()
        g.check()
        assert any('train.py' in s for s in g.sites())
        assert torch.isfinite(loss).all() and torch.isfinite(pred).all()
        for k, v in grads.items():
            assert torch.isfinite(v).all(), k
        _check_grads(grads, CO.reference(), 'guarded')


def test_training_trains(small):
    """Five Trainer.step calls at lr 2e-4 on the fixed batch with a fixed z against five steps of the float64 restatement (autograd +
    numpy Adam / EMA).  The bar of the shadows is D32 x 8, D32 = the largest |shadow - shadow64| of the same restatement run in float32
    (tests/test_gpu_train.py, test_training_trains), and the shadows of the three transposed-conv weights must have moved by more than
    twice that bar: a conditioning that is not trained would stand still."""
    from pwv_amd import train as TR
    steps = 5
    ref_losses, ref_shadow = CO.trajectory(steps)
    _, shadow32 = CO.trajectory(steps, single=True)
    d32 = max(float(np.abs(shadow32[k].astype(np.float64) - ref_shadow[k]).max()) for k in ref_shadow)
    bar = MARGIN * d32
    model, store, wav, mel, z = small()
    tr = TR.Trainer(model, lr=TO.LR, beta2=TO.BETA2, ema_decay=TO.DECAY)
    losses = [float(tr.step(wav, mel, z=z)) for _ in range(steps)]
    assert tr.steps == steps
    print('gpu  ', ' '.join('%.6f' % v for v in losses))
    print('fp64 ', ' '.join('%.6f' % v for v in ref_losses))
    assert all(abs(a - b) <= TOL_F32 for a, b in zip(losses, ref_losses))      # (a mean of |pred - wav|, pred within TOL_F32)
    shadows = tr.shadows()
    assert sorted(shadows) == sorted(ref_shadow)
    errs = {k: float(np.abs(shadows[k].cpu().numpy().astype(np.float64) - want).max()) for k, want in ref_shadow.items()}
    print('largest shadow difference %.3g (D32 %.3g, bar %.3g)' % (max(errs.values()), d32, bar))
    for k, err in errs.items():
        assert err <= bar, (k, err, d32)
    w0 = CO.problem()[1]
    for i in range(3):
        k = 'iaf_vocoder/cond/transposed_conv_%d_weights' % i
        moved = float(np.abs(shadows[k].cpu().numpy().astype(np.float64) - w0[k]).max())
        assert moved > 2 * bar, (k, moved, bar)


def test_train_cli_then_generate(gpu, tmp_path):
    """`python -m pwv_amd.train train/small_tran --steps=2` on seeded stand-in audio writes a checkpoint with the transposed-conv weights,
    their shadows and moments, that `generate` loads, and the result is finite audio."""
    env = dict(os.environ, PWV_LOGDIR=str(tmp_path), PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = subprocess.run([sys.executable, '-m', 'pwv_amd.train', 'train/small_tran', '--steps=2', '--seed=4'], cwd=ROOT, env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:]
    lines = [l for l in out.stdout.splitlines() if 'loss/likelihood' in l]
    assert len(lines) == 2 and all(np.isfinite(float(l.split()[-1])) for l in lines), out.stdout[-2000:]
    ckpt = tmp_path / 'model-2.npz'
    assert ckpt.exists()
    with np.load(str(ckpt)) as f:
        for i in range(3):
            k = 'iaf_vocoder/cond/transposed_conv_%d_weights' % i
            assert k in f.files and k + '/ExponentialMovingAverage' in f.files and k + '/Adam_1' in f.files
            assert np.abs(f[k + '/Adam']).max() > 0
        assert 'iaf_vocoder/cond/dense' not in f.files
    gen = subprocess.run([sys.executable, '-m', 'pwv_amd.generate', 'train/small_tran'], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, text=True, timeout=300)
    assert gen.returncode == 0, gen.stdout[-3000:]
    assert 'No checkpoint found' not in gen.stdout
    pred = np.load(str(tmp_path / 'pred_wav.npy'))
    assert pred.shape[1] == 1600 and np.isfinite(pred).all() and np.abs(pred).max() > 0
