"""GPU: training the shared-net architecture (pwv_amd/train.py: shared_nets=True -> pwv_train_shared_*, csrc/pwv_train_shared.hip)
against float64 autograd on the CPU (tests/train_shared_oracle.py): the two-output head through the C ABI in both input modes at
ragged shapes, the whole small shared model (uniform, packed, with skip connections, with transposed-conv conditioning), the training
forward against the generation forward, the default architecture as it was, five optimiser steps with save / load / generate, and the
command line.

The bars are the project's own (tests/test_gpu_train.py): err(v) = max|g - g64| / max|g64| within 8 E32 per output, E32 = the largest
err of float32 autograd on the CPU of the same restatement, computed at run time; 2e-5 for a prediction; 8 D32 for a shadow after five
steps.

Measured on an MI355X (E32 in brackets): see DESIGN.md section 9, "Training the shared-net architecture"."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import train_oracle as TO
from tests import train_shared_oracle as SO
from tests import train_varlen_oracle as VO
from tests.guarded import Guard
from tests.util import TOL_F32, set_hparams

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 8
HEAD_SHAPES = [(2, 208), (3, 80), (5, 16), (1, 16)]            # 13 whole units, 7.5 units, 2.5 units, half a unit
MODEL_SHAPES = [(3, 240, 80), (5, 16, 16), (1, 16, 16)]
assert TOL_F32 == 2e-5


@pytest.fixture(autouse=True)
def _default_hparams():
    yield
    from pwv_amd.hparam import hparam as hp
    hp.set_hparam_yaml('default')


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _id(v):
    return 'x'.join(str(x) for x in v) if isinstance(v, (tuple, list)) else str(v)


# ---- the head through ctypes ------------------------------------------------------------------------------------------------------------
def _head_run(c, mode, biased, max_workgroups, device, guard=None):
    """(y0, y1 float32 numpy, {output: float64 numpy}) of one forward and one backward call.  Tile32 inputs have NaN padding rows; every
    output and the workspace start as NaN.  With a tests.guarded.Guard every buffer the calls see -- inputs too -- lies between poisoned
    bands."""
    from pwv_amd import _lib
    lib, rows = _lib.lib(), c['rows']

    def nan(*shape):
        if guard is not None:
            return guard.allocate(shape, torch.float32, device, None)          # 0xFF..: NaN
        return torch.full(shape, float('nan'), dtype=torch.float32, device=device)

    def up(a):
        t = nan(*np.asarray(a).shape)
        t.copy_(_dev(a, device))
        return t

    t = {k: up(c[k]) for k in SO.HEAD_WEIGHTS + ('d_out', 'd_mul') if biased or k not in SO.HEAD_BIASES}
    o, S = up(TO.to_tile32(c['o'])), up(TO.to_tile32(c['S']))
    blocks = (rows + 31) // 32
    w = dict(post1=t['post1'], post1_bias=t.get('post1_bias'), post2=t['post2'], post2_bias=t.get('post2_bias'))
    if mode == SO.GATED:
        w.update(x=o, skip=t['skip'], skip_bias=t.get('skip_bias'))
    else:
        w.update(skip_sum=S)

    def args(**kw):
        kw = dict(w, **kw)
        return _lib.TrainSharedArgs(N=c['N'], T=c['T'], max_workgroups=max_workgroups, head_in=mode,
                                    **{k: (v.data_ptr() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()})

    def call(name, a):
        _lib.check(getattr(lib, name)(ctypes.byref(a), torch.cuda.current_stream().cuda_stream), name)

    need = lib.pwv_train_shared_workspace_bytes(ctypes.byref(args()))
    assert need > 0 and need % 4 == 0
    ws, y = nan(need // 4), nan(2, rows)
    call('pwv_train_shared_head_fwd_f32', args(y=y[0], y_shift=y[1]))
    names = [k for k in SO.HEAD_WEIGHTS if k in t and (mode == SO.GATED or not k.startswith('skip'))]
    out = {k: nan(*c[k].shape) for k in names}
    kw = dict(d_out=t['d_out'], d_mul=t['d_mul'], d_post1=out['post1'], d_post1_bias=out.get('post1_bias'), d_post2=out['post2'],
              d_post2_bias=out.get('post2_bias'), workspace=ws, workspace_bytes=need)
    if mode == SO.GATED:
        d_x = nan(blocks * 32 * 64)
        kw.update(d_o_out=d_x, d_skip=out['skip'], d_skip_bias=out.get('skip_bias'))
    else:
        d_x = nan(blocks * 32 * 128)
        out['skip_bias'] = nan(128)             # the column sums of dS leave with or without biases in the head
        kw.update(d_skip_sum_out=d_x, d_skip_bias=out['skip_bias'])
    call('pwv_train_shared_head_bwd_f32', args(**kw))
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy().astype(np.float64) for k, v in out.items()}
    raw = d_x.cpu().numpy()
    C = 64 if mode == SO.GATED else 128
    res['d_o' if mode == SO.GATED else 'dS'] = TO.from_tile32(raw, rows, C).astype(np.float64)
    pad = raw.reshape(blocks, C // 4, 32, 4).transpose(0, 2, 1, 3).reshape(blocks * 32, C)[rows:]
    assert np.isnan(pad).all()                  # rows beyond the batch are not written
    yy = y.cpu().numpy()
    return yy[0], yy[1], res


def _same_outputs(a, b):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and sorted(a[2]) == sorted(b[2])
    for k in a[2]:
        assert np.array_equal(a[2][k], b[2][k]), k


@pytest.mark.parametrize('mode', [SO.GATED, SO.SKIPSUM], ids=['gated', 'skipsum'])
@pytest.mark.parametrize('shape', HEAD_SHAPES, ids=_id)
def test_shared_head_matches_float64_autograd(gpu, shape, mode):
    """The two-output head through the C ABI, forward and backward, with every bias and with none, at 1, 3 and the default number of
    workgroups: y0, y1, d o / dS and every weight gradient within 8 E32 of float64 autograd; y0, y1 the same bits at every grid; every
    output the bits of its repetition; one run inside guard bands, none touched, the bits of the plain run."""
    c = SO.head_case(*shape)
    for biased in (True, False):
        h64, h32 = SO.shared_head(c, mode, torch.float64, biased), SO.shared_head(c, mode, torch.float32, biased)
        names = sorted(h64)
        assert 'y0' in names and 'y1' in names and 'post2' in names and ('d_o' if mode == SO.GATED else 'dS') in names
        assert ('post2_bias' in names) == biased
        e32 = max(TO.rel_err(h32[k], h64[k]) for k in names)
        runs = {}
        for mwg in (1, 3, 0):
            y0, y1, got = _head_run(c, mode, biased, mwg, gpu)
            runs[mwg] = (y0, y1, got)
            got = dict(got, y0=y0.astype(np.float64), y1=y1.astype(np.float64))
            assert sorted(got) == names
            for k in names:
                assert np.isfinite(got[k]).all(), (k, mwg)          # no NaN of a padding row or of an unwritten partial arrives
                err = TO.rel_err(got[k], h64[k])
                print('%s %s biased=%d max_workgroups=%d %s err %.3g (E32 %.3g)' % (_id(shape), mode, biased, mwg, k, err, e32))
                assert err <= MARGIN * e32, (k, mwg, err, e32)
            assert np.array_equal(y0, runs[1][0]) and np.array_equal(y1, runs[1][1]), mwg
            xk = 'd_o' if mode == SO.GATED else 'dS'
            assert np.array_equal(got[xk], runs[1][2][xk]), mwg          # row-local as well: no grid in it
        _same_outputs(runs[3], _head_run(c, mode, biased, 3, gpu))
        guard = Guard()
        inside = _head_run(c, mode, biased, 3, gpu, guard)
        guard.check()
        assert len(guard.allocations) >= 10
        _same_outputs(runs[3], inside)


# ---- the whole model ------------------------------------------------------------------------------------------------------------------
def _store(w, device):
    from pwv_amd.variables import VariableStore
    store = VariableStore(device=device)
    store.load_dict(w)
    return store


def _model(device, shape=(TO.N, TO.T, TO.HOP), skip=False, tran=False):
    from pwv_amd.models import IAFVocoder
    N, T, hop = shape
    cfg, w, mel, z, wav = SO.problem(N, T, hop, skip, tran)
    set_hparams(cfg)
    store = _store(w, device)
    return IAFVocoder(batch_size=N, length=T, store=store, precision='f32'), store, _dev(wav, device), _dev(mel, device), _dev(z, device)


def _packed_model(device, skip=False):
    from pwv_amd.models import IAFVocoder
    cfg, w, mels, zs, wavs = SO.packed_problem(skip=skip)
    set_hparams(cfg)
    model = IAFVocoder(batch_size=1, length=max(VO.LENGTHS), store=_store(w, device), precision='f32')
    return model, [_dev(a[0, :, 0], device) for a in wavs], [_dev(a[0], device) for a in mels], [_dev(a[0], device) for a in zs]


def _kw(skip):
    return dict(shared_nets=True, use_skip_connection=True) if skip else dict(shared_nets=True)


def _check_grads(grads, ref, dead, what):
    """Every live gradient within 8 E32 of float64 autograd, exact zeros for the variables the model never reads."""
    g64, bar = ref['g64'], MARGIN * ref['E32']
    assert sorted(grads) == sorted(g64)
    worst, zeros = 0.0, 0
    for k, want in g64.items():
        got = grads[k].detach().cpu().numpy().astype(np.float64)
        if want is None:
            assert np.abs(got).max() == 0, (what, k)
            zeros += 1
            continue
        assert got.shape == want.shape and np.isfinite(got).all(), (what, k)
        err = TO.rel_err(got, want)
        worst = max(worst, err)
        assert err <= bar, (what, k, err, bar)
    print('%s worst gradient err %.3g (E32 %.3g, bar %.3g)' % (what, worst, ref['E32'], bar))
    assert zeros == dead and sorted(grads.unread) == sorted(k for k, v in g64.items() if v is None)


def _check_uniform(run, ref, shape, dead, what):
    loss, pred, grads = run
    assert tuple(pred.shape) == (shape[0], shape[1], 1) and loss.dim() == 0 and loss.is_cuda
    _check_grads(grads, ref, dead, what)
    assert abs(float(loss) - ref['loss']) <= 2e-6 * max(1.0, abs(ref['loss']))
    err = np.abs(pred.detach().cpu().numpy().astype(np.float64) - ref['pred']).max()
    print('%s pred err %.3g' % (what, err))
    assert err <= 2e-5


def _check_packed(run, ref, dead, what):
    loss, preds, grads = run
    assert loss.dim() == 0 and loss.is_cuda and [tuple(p.shape) for p in preds] == [(T, 1) for T in VO.LENGTHS]
    _check_grads(grads, ref, dead, what)
    assert abs(float(loss) - ref['loss']) <= 2e-6 * max(1.0, abs(ref['loss']))
    for p, want in zip(preds, ref['preds']):
        assert np.abs(p.detach().cpu().numpy().astype(np.float64).reshape(-1) - want).max() <= 2e-5


def _same(a, b):
    preds = lambda r: r[1] if isinstance(r[1], (list, tuple)) else [r[1]]
    assert torch.equal(a[0], b[0]) and all(torch.equal(p, q) for p, q in zip(preds(a), preds(b)))
    assert sorted(a[2]) == sorted(b[2])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k


def _twice(fn):
    runs = []
    for _ in range(2):
        runs.append(fn())
        torch.cuda.synchronize()
    _same(runs[0], runs[1])
    return runs[0]


@pytest.mark.parametrize('max_workgroups', [1, 3, 0])
def test_shared_model_gradients_match_float64_autograd(gpu, max_workgroups):
    """2 x 208 at hop 16 with 1, 3 and the default number of partials: all 75 gradients, the loss and pred against float64 autograd,
    exact zeros for the 16 unread variables, each run the bits of its repetition; a bare call is refused."""
    from pwv_amd import train as TR
    from pwv_amd._lib import PwvError
    model, _, wav, mel, z = _model(gpu)
    with pytest.raises(PwvError, match='shared'):
        TR.loss_and_grad(model, wav, mel, z=z)
    run = _twice(lambda: TR.loss_and_grad(model, wav, mel, z=z, max_workgroups=max_workgroups, shared_nets=True))
    _check_uniform(run, SO.reference(), (TO.N, TO.T), SO.DEAD, 'shared max_workgroups=%d' % max_workgroups)


@pytest.mark.parametrize('shape', MODEL_SHAPES, ids=_id)
def test_shared_model_gradients_at_ragged_shapes(gpu, shape):
    """3 x 240 at hop 80 (22.5 units, four dP slots), 5 x 16 and 1 x 16 (utterances of half a unit)."""
    from pwv_amd import train as TR
    model, _, wav, mel, z = _model(gpu, shape)
    run = _twice(lambda: TR.loss_and_grad(model, wav, mel, z=z, shared_nets=True))
    _check_uniform(run, SO.reference(*shape), shape, SO.DEAD, 'shared %s' % _id(shape))


@pytest.mark.parametrize('skip', [False, True], ids=['plain', 'skip'])
def test_packed_shared_model_gradients_match_float64_autograd(gpu, skip):
    """The packed batch (208, 16, 48, 144), without and with skip connections, against float64 autograd of the utterances run one by
    one; the bits of its repetition; every utterance alone has the prediction it has in the batch."""
    from pwv_amd import train as TR
    model, wavs, mels, zs = _packed_model(gpu, skip)
    run = _twice(lambda: TR.loss_and_grad_varlen(model, wavs, mels, z=zs, **_kw(skip)))
    _check_packed(run, SO.packed_reference(skip=skip), SO.DEAD_SKIP if skip else SO.DEAD, 'packed shared skip=%d' % skip)
    for i in range(len(wavs)):
        _, alone, _ = TR.loss_and_grad_varlen(model, [wavs[i]], [mels[i]], z=[zs[i]], **_kw(skip))
        torch.cuda.synchronize()
        assert torch.equal(run[1][i], alone[0]), i


def test_shared_skip_model_gradients_match_float64_autograd(gpu):
    """With skip connections (both requests), 2 x 208: 87 gradients, 4 exact zeros; one request alone is refused."""
    from pwv_amd import train as TR
    from pwv_amd._lib import PwvError
    model, _, wav, mel, z = _model(gpu, skip=True)
    with pytest.raises(PwvError, match='skip accumulation'):
        TR.loss_and_grad(model, wav, mel, z=z, shared_nets=True)
    with pytest.raises(PwvError, match='shared'):
        TR.loss_and_grad(model, wav, mel, z=z, use_skip_connection=True)
    run = _twice(lambda: TR.loss_and_grad(model, wav, mel, z=z, max_workgroups=3, **_kw(True)))
    _check_uniform(run, SO.reference(skip=True), (TO.N, TO.T), SO.DEAD_SKIP, 'shared + skip')


def test_shared_transposed_conv_model_gradients_match_float64_autograd(gpu):
    """With transposed-conv conditioning, 2 x 160 at hop 80: the per-sample layer kernels, the same head call."""
    from pwv_amd import train as TR
    shape = (2, 160, 80)
    model, _, wav, mel, z = _model(gpu, shape, tran=True)
    run = _twice(lambda: TR.loss_and_grad(model, wav, mel, z=z, shared_nets=True))
    ref = SO.reference(*shape, tran=True)
    assert len(ref['g64']) == SO.TOTAL + 2
    _check_uniform(run, ref, shape, SO.DEAD, 'shared + transposed_conv')


@pytest.mark.parametrize('skip', [False, True], ids=['plain', 'skip'])
def test_equal_lengths_give_the_bits_of_the_uniform_batch(gpu, skip):
    """Two utterances of 208 samples packed = the uniform 2 x 208 call, bit for bit: the loss, every pred, every gradient."""
    from pwv_amd import train as TR
    model, _, wav, mel, z = _model(gpu, skip=skip)
    a = TR.loss_and_grad(model, wav, mel, z=z, **_kw(skip))
    b = TR.loss_and_grad_varlen(model, [wav[i, :, 0] for i in range(TO.N)], [mel[i] for i in range(TO.N)], z=[z[i] for i in range(TO.N)],
                                **_kw(skip))
    torch.cuda.synchronize()
    _same((a[0], [a[1][i] for i in range(TO.N)], a[2]), b)


def test_training_forward_agrees_with_the_generation_forward(gpu):
    """pred of loss_and_grad against model(mel, z) at precision 'f32' (SharedIAFLayer on the generation kernels) on the same weights and
    noise: both within 2e-5 of the float64 oracle; their difference is printed, not barred."""
    from pwv_amd import train as TR
    from pwv_amd.modules import SharedIAFLayer
    model, store, wav, mel, z = _model(gpu)
    _, pred, _ = TR.loss_and_grad(model, wav, mel, z=z, shared_nets=True)
    out = model(None, mel, is_training=False, z=z, verify=False)
    model.verify()
    with TR.variable_scope(TR.SCOPE, absolute=True):
        assert all(isinstance(f, SharedIAFLayer) for f in model._flows(store, True, 'f32'))
    want = SO.reference()['pred']
    assert out.shape == pred.shape == want.shape
    e_train = np.abs(pred.cpu().numpy().astype(np.float64) - want).max()
    e_gen = np.abs(out.cpu().numpy().astype(np.float64) - want).max()
    print('training forward err %.3g, generation forward err %.3g, |training - generation| %.3g (|y|max %.3g)'
          % (e_train, e_gen, float((out - pred).abs().max()), np.abs(want).max()))
    assert e_train <= 2e-5 and e_gen <= 2e-5


def test_the_default_architecture_is_untouched(gpu):
    """loss_and_grad without the request under the default small model runs as before: its 181 gradients within its own bar, and
    shared_nets=None the bits of the bare call."""
    from pwv_amd import train as TR
    from pwv_amd.models import IAFVocoder
    cfg, w, mel, z, wav = TO.problem()
    set_hparams(cfg)
    model = IAFVocoder(batch_size=TO.N, length=TO.T, store=_store(w, gpu), precision='f32')
    wav, mel, z = _dev(wav, gpu), _dev(mel, gpu), _dev(z, gpu)
    assert TR.refusal(model, wav, mel) is None
    a = TR.loss_and_grad(model, wav, mel, z=z)
    b = TR.loss_and_grad(model, wav, mel, z=z, shared_nets=None)
    torch.cuda.synchronize()
    _same(a, b)
    ref = TO.reference()
    assert len(a[2]) == 181
    for k, want in ref['g64'].items():
        got = a[2][k].cpu().numpy().astype(np.float64)
        assert (np.abs(got).max() == 0) if want is None else (TO.rel_err(got, want) <= MARGIN * ref['E32']), k
    assert np.abs(a[1].cpu().numpy().astype(np.float64) - ref['pred']).max() <= 2e-5


@pytest.mark.parametrize('fused', [False, True], ids=['foreach', 'fused'])
def test_shared_training_trains(gpu, fused, tmp_path):
    """Five Trainer.step calls (shared_nets=True) at lr 2e-4 on the fixed batch against five steps of the float64 restatement: the loss
    falls at every step and follows the float64 trajectory, the shadows stay within 8 D32 (D32 = the largest |shadow - shadow64| of
    the same restatement run in float32, as tests/test_gpu_train.py has it); save -> load resumes bit for bit; a fresh model that loads
    the .npz with use_ema generates within 2e-5 of the oracle on the shadows."""
    from pwv_amd import train as TR
    from pwv_amd.models import IAFVocoder
    from pwv_amd.variables import EMA_SUFFIX, VariableStore
    ref_losses, ref_shadow = SO.trajectory(5)
    _, shadow32 = SO.trajectory(5, single=True)
    d32 = max(float(np.abs(shadow32[k].astype(np.float64) - ref_shadow[k]).max()) for k in ref_shadow)
    model, store, wav, mel, z = _model(gpu)
    make = lambda m: TR.Trainer(m, lr=TO.LR, beta2=TO.BETA2, ema_decay=TO.DECAY, fused=fused, shared_nets=True)
    tr = make(model)
    losses = [float(tr.step(wav, mel, z=z)) for _ in range(5)]
    assert tr.steps == 5
    path = str(tmp_path / 'model-5.npz')
    tr.save(path)
    losses.append(float(TR.loss_and_grad(model, wav, mel, z=z, shared_nets=True)[0]))
    print('gpu  ', ' '.join('%.5f' % v for v in losses))
    print('fp64 ', ' '.join('%.5f' % v for v in ref_losses))
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    assert max(abs(a - b) for a, b in zip(losses, ref_losses)) <= 2e-5          # the loss is a mean of |pred - wav|: the prediction's bar
    shadows = tr.shadows()
    assert sorted(shadows) == sorted(ref_shadow) and len(shadows) == SO.TOTAL
    errs = {k: float(np.abs(shadows[k].cpu().numpy().astype(np.float64) - want).max()) for k, want in ref_shadow.items()}
    print('largest shadow difference %.3g (D32 %.3g, bar %.3g)' % (max(errs.values()), d32, MARGIN * d32))
    for k, err in errs.items():
        assert err <= MARGIN * d32, (k, err, d32)
    # save -> load resumes bit for bit: a sixth step of the trainer that went on and of one that loaded
    model2, store2, _, _, _ = _model(gpu)
    tr2 = make(model2)
    assert tr2.load(path) == 5
    l6, l6b = tr.step(wav, mel, z=z), tr2.step(wav, mel, z=z)
    torch.cuda.synchronize()
    assert torch.equal(l6, l6b)
    for n in tr.names:
        assert torch.equal(store.vars[n], store2.vars[n]), n
    a, b = tr.shadows(), tr2.shadows()
    assert all(torch.equal(a[n], b[n]) for n in tr.names)
    # a fresh model on the shadows of the file
    with np.load(path) as zf:
        ema = {k[:-len(EMA_SUFFIX)]: zf[k] for k in zf.files if k.endswith(EMA_SUFFIX)}
    assert sorted(ema) == sorted(ref_shadow) and all('/shared/' in k or '/cond/' in k for k in ema)
    cfg, _, mel_np, z_np, _ = SO.problem()
    set_hparams(cfg)
    fresh = VariableStore(device=gpu)
    fresh.load_npz(path, use_ema=True)
    gen = IAFVocoder(batch_size=TO.N, length=TO.T, store=fresh, precision='f32')
    out = gen(None, mel, is_training=False, z=z, verify=False)
    gen.verify()
    want = SO.pred64(ema, mel_np, z_np, cfg)
    err = np.abs(out.cpu().numpy().astype(np.float64) - want).max()
    print('generation on the shadows err %.3g' % err)
    assert err <= 2e-5


def test_train_cli_shared_packed_data_parallel(gpu, tmp_path):
    """`python -m pwv_amd.train train/small_shared --varlen --gpus 2 --steps 2`: two ranks (on a machine with one GPU both on it, over
    gloo: the dry run of tests/test_gpu_train_opt.py), each a DataParallelTrainer that was handed the request, on packed batches."""
    env = dict(os.environ, PWV_LOGDIR=str(tmp_path), PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT', 'MASTER_ADDR', 'PWV_TRAIN_DRYRUN_ONE_GPU'):
        env.pop(k, None)
    if torch.cuda.device_count() < 2:
        env['PWV_TRAIN_DRYRUN_ONE_GPU'] = '1'
    out = subprocess.run([sys.executable, '-m', 'pwv_amd.train', 'train/small_shared', '--varlen', '--gpus', '2', '--steps', '2'], cwd=ROOT,
                         env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith('step ')]
    assert len(lines) == 2 and all('loss/likelihood' in l and np.isfinite(float(l.split()[-1])) for l in lines), out.stdout[-2000:]
    assert (tmp_path / 'model-2.npz').exists()


def test_train_cli_shared_then_generate(gpu, tmp_path):
    """`python -m pwv_amd.train train/small_shared --steps=3` in a fresh process opts in by itself and writes a checkpoint under the
    shared names; `generate` loads it with use_ema and writes finite audio of the asked length."""
    env = dict(os.environ, PWV_LOGDIR=str(tmp_path), PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = subprocess.run([sys.executable, '-m', 'pwv_amd.train', 'train/small_shared', '--steps=3', '--seed=4'], cwd=ROOT, env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:]
    lines = [l for l in out.stdout.splitlines() if 'loss/likelihood' in l]
    assert len(lines) == 3 and all(np.isfinite(float(l.split()[-1])) for l in lines), out.stdout[-2000:]
    ckpt = tmp_path / 'model-3.npz'
    assert ckpt.exists()
    with np.load(str(ckpt)) as z:
        assert any(k.endswith('/ExponentialMovingAverage') for k in z.files) and any(k.endswith('/Adam_1') for k in z.files)
        assert z['iaf_vocoder/iaf0/shared/postprocessing/postprocess2'].shape == (1, 128, 2)
        assert not any('/scalar/' in k or '/shifter/' in k for k in z.files)
    gen = subprocess.run([sys.executable, '-m', 'pwv_amd.generate', 'train/small_shared'], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, text=True, timeout=300)
    assert gen.returncode == 0, gen.stdout[-3000:]
    assert 'No checkpoint found' not in gen.stdout
    pred = np.load(str(tmp_path / 'pred_wav.npy'))
    assert pred.shape[1] == 1600 and np.isfinite(pred).all() and np.abs(pred).max() > 0
