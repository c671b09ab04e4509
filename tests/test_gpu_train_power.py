"""GPU: training with the STFT power loss (pwv_amd/train.py: power_weight -> pwv_train_loss_f32, csrc/pwv_train_loss.hip) against float64
on the CPU (tests/train_power_oracle.py): the loss head through the C ABI at every kind of framing, the whole small model under
L1 + w * power, five optimiser steps, and `python -m pwv_amd.train train/small_power`.

The bar of a gradient is the one of tests/test_gpu_train.py: err = max|g - g64| / max|g64|, E32 = that error of float32 autograd on the
CPU of the same function, computed at run time, and the device must stay within 8 E32.  The loss head itself works in float64 and rounds
once, so it sits far inside; measured maxima are in DESIGN.md section 9, "Training"."""
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
from tests.guarded import Guard
from tests.util import TOL_F32, set_hparams

pytestmark = pytest.mark.gpu
SHAPES, case = PO.SHAPES, PO.case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 8
N = 2


# ---- the loss head through ctypes -----------------------------------------------------------------------------------------------------
def _loss_head(pred, y, win, hop, wl1, wp, device, guard=None):
    """One pwv_train_loss_f32 on float32 numpy [n, T] inputs; d_out, result and workspace start as NaN.  Returns (d_out float32 [n, T],
    result float64 [n, 4]) as CPU tensors.  `guard`: a tests.guarded.Guard whose banded, poisoned buffers hold everything."""
    from pwv_amd import _lib
    lib = _lib.lib()
    n, T = pred.shape
    a = _lib.TrainLossArgs(n=n, T=T, win_length=win, hop_length=hop, weight_l1=wl1, weight_power=wp)
    need = int(lib.pwv_train_loss_workspace_bytes(ctypes.byref(a)))
    assert need > 0 and need % 8 == 0, lib.pwv_last_error()

    def buf(shape, dtype, src=None):
        if guard is not None:
            t = guard.allocate(shape, dtype, device, None)
            assert torch.isnan(t).all()                     # (poisoned: 0xFF.. is a NaN)
        else:
            t = torch.full(shape, float('nan'), dtype=dtype, device=device)
        if src is not None:
            t.copy_(torch.from_numpy(src))
        return t

    p, t_y = buf((n, T), torch.float32, pred), buf((n, T), torch.float32, y)
    d_out, table, work = buf((n, T), torch.float32), buf((n, 4), torch.float64), buf((need // 8,), torch.float64)
    a.out, a.y, a.d_out, a.result, a.workspace, a.workspace_bytes = p.data_ptr(), t_y.data_ptr(), d_out.data_ptr(), table.data_ptr(), work.data_ptr(), need
    _lib.check(lib.pwv_train_loss_f32(ctypes.byref(a), torch.cuda.current_stream().cuda_stream), 'pwv_train_loss_f32')
    torch.cuda.synchronize()
    return d_out.cpu(), table.cpu()


@functools.lru_cache(maxsize=None)
def _kernel_reference(T, win, hop):
    """The case of a shape and its float64 / float32 CPU references (computed once, never written to): the power gradient at weight 1, the
    L1 gradient, their E32s, and the table of score.score_reference."""
    from pwv_amd.score import score_reference
    pred, y = case(T, N)
    gp = PO.power_grad_numpy(pred, y, win, hop)
    gp32 = PO.power_grad_autograd(pred, y, win, hop, torch.float32)
    diff = torch.from_numpy(pred) - torch.from_numpy(y)
    l1_32 = torch.sign(diff) / float(N * T)                             # what train.py forms in float32 at power_weight None
    l1_64 = np.sign(pred.astype(np.float64) - y) / (N * T)

    def both(dtype):
        p = torch.from_numpy(pred).to(dtype).requires_grad_(True)
        t = torch.from_numpy(y).to(dtype)
        ((p - t).abs().mean() + PO.power_loss_torch(p, t, win, hop, dtype)).backward()
        return p.grad.double().numpy()

    b64 = both(torch.float64)
    assert np.abs(b64 - (l1_64 + gp)).max() <= 1e-12 * np.abs(b64).max()
    return {'pred': pred, 'y': y, 'gp': gp, 'e32_power': TO.rel_err(gp32, gp), 'l1_32': l1_32, 'both': b64,
            'e32_both': TO.rel_err(both(torch.float32), b64), 'table': score_reference(pred, y, win, hop)}


@pytest.mark.parametrize('T, win, hop', SHAPES)
def test_loss_head_matches_float64(gpu, T, win, hop):
    """The power gradient alone, the L1 alone and both, each against its reference; the table against score.score_reference; a second run
    of each is bit-identical."""
    r = _kernel_reference(T, win, hop)
    pred, y = r['pred'], r['y']
    # the power gradient alone
    d, table = _loss_head(pred, y, win, hop, 0.0, 1.0, gpu)
    assert torch.isfinite(d).all() and torch.isfinite(table).all()
    err = TO.rel_err(d.numpy(), r['gp'])
    print('(%d, %d, %d) power gradient err %.3g (E32 %.3g)' % (T, win, hop, err, r['e32_power']))
    assert err <= MARGIN * r['e32_power'], (err, r['e32_power'])
    covered = np.zeros(T, dtype=bool)
    for f in range(PO.frame_count(T, win, hop)):
        covered[f * hop:f * hop + win] = True
    assert (d.numpy()[:, ~covered] == 0).all()                          # written, and the power term is 0 where no frame is
    assert (np.abs(table.numpy() - r['table']) <= 1e-10 * np.abs(r['table'])).all()
    d2, table2 = _loss_head(pred, y, win, hop, 0.0, 1.0, gpu)
    assert torch.equal(d, d2) and torch.equal(table, table2)
    # the L1 alone: one float32 ulp of sign / (n T); no frame is formed
    d, table = _loss_head(pred, y, win, hop, 1.0, 0.0, gpu)
    want = r['l1_32'].numpy()
    ulp = np.spacing(np.float32(1.0 / (N * T)))
    assert np.abs(d.numpy().astype(np.float64) - want.astype(np.float64)).max() <= ulp
    assert (np.sign(d.numpy()) == np.sign(want)).all()
    l1_table = r['table'] * [1, 1, 0, 0]
    assert (np.abs(table.numpy() - l1_table) <= 1e-10 * np.abs(l1_table)).all() and (table.numpy()[:, 2:] == 0).all()
    dw, tablew = _loss_head(pred, y, 0, hop, 1.0, 1.0, gpu)             # win_length 0 is the same mode
    assert torch.equal(d, dw) and torch.equal(table, tablew)
    # both on
    d, table = _loss_head(pred, y, win, hop, 1.0, 1.0, gpu)
    err = TO.rel_err(d.numpy(), r['both'])
    print('(%d, %d, %d) L1 + power gradient err %.3g (E32 %.3g)' % (T, win, hop, err, r['e32_both']))
    assert err <= MARGIN * r['e32_both'], (err, r['e32_both'])
    assert (np.abs(table.numpy() - r['table']) <= 1e-10 * np.abs(r['table'])).all()
    d2, table2 = _loss_head(pred, y, win, hop, 1.0, 1.0, gpu)
    assert torch.equal(d, d2) and torch.equal(table, table2)


@pytest.mark.parametrize('T, win, hop', SHAPES)
def test_loss_head_keeps_utterances_apart(gpu, T, win, hop):
    """Other contents in utterance 1 leave utterance 0's d_out and row of the table bit-identical, and change utterance 1's: no frame
    crosses the boundary, no partial is shared."""
    r = _kernel_reference(T, win, hop)
    other_pred, other_y = case(T, N, seed=7)
    pred2, y2 = r['pred'].copy(), r['y'].copy()
    pred2[1], y2[1] = other_pred[0], other_y[0]
    a, ta = _loss_head(r['pred'], r['y'], win, hop, 1.0, 1.0, gpu)
    b, tb = _loss_head(pred2, y2, win, hop, 1.0, 1.0, gpu)
    assert torch.equal(a[0], b[0]) and torch.equal(ta[0], tb[0])
    assert not torch.equal(a[1], b[1]) and not torch.equal(ta[1, 0], tb[1, 0]) and not torch.equal(ta[1, 2], tb[1, 2])


@pytest.mark.parametrize('T, win, hop', SHAPES)
def test_loss_head_in_guarded_buffers(gpu, T, win, hop):
    """One call inside guard-banded buffers with d_out, result and the workspace poisoned: no band is touched, and d_out and result are
    finite everywhere -- a sample that is never written, or a workspace slot that is read and never written, is a NaN."""
    r = _kernel_reference(T, win, hop)
    g = Guard()
    d, table = _loss_head(r['pred'], r['y'], win, hop, 1.0, 1.0, gpu, guard=g)
    g.check()
    assert len(g.allocations) == 5
    assert torch.isfinite(d).all() and torch.isfinite(table).all()
    assert TO.rel_err(d.numpy(), r['both']) <= MARGIN * r['e32_both']


# ---- the whole model ------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def small(gpu):
    """(model, store, wav, mel, z) of tests.train_oracle's problem on the device with hp.signal.win_length = 48: 11 frames at hop 16."""
    from pwv_amd.hparam import hparam as hp
    from pwv_amd.models import IAFVocoder
    from pwv_amd.variables import VariableStore
    cfg, w, mel, z, wav = TO.problem()
    set_hparams(cfg)
    hp.signal.win_length = PO.WIN
    assert PO.frame_count(TO.T, PO.WIN, cfg.hop_length) == 11
    store = VariableStore(device=gpu)
    store.load_dict(w)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    yield IAFVocoder(batch_size=TO.N, length=TO.T, store=store, precision='f32'), store, dev(wav), dev(mel), dev(z)
    hp.set_hparam_yaml('default')


def _check_grads(grads, g64, e32, what):
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
        assert err <= MARGIN * e32, (what, k, err, e32)
    print('%s worst gradient err %.3g (E32 %.3g, bar %.3g)' % (what, worst, e32, MARGIN * e32))
    assert zeros == 32 and len(g64) - zeros == 149


def test_model_gradients_with_the_power_loss(small):
    """All 149 gradients of L1 + w * power against float64 autograd, w from the float64 reference so that both terms' gradients for pred
    have the same maximum (at 0.0005 a wrong power term would hide under the L1's); exact zeros for the 32 unused variables; the terms
    within 2e-6 relative; `loss` their combination; a second run bit-identical."""
    from pwv_amd import train as TR
    model, _, wav, mel, z = small
    ref = PO.reference()
    w = ref['w']
    gp = PO.power_grad_numpy(ref['pred'], TO.problem()[4], PO.WIN, 16)
    assert abs(w * np.abs(gp).max() * TO.N * TO.T - 1) < 1e-12
    runs = []
    for _ in range(2):
        terms = {}
        loss, pred, grads = TR.loss_and_grad(model, wav, mel, z=z, power_weight=w, terms=terms)
        torch.cuda.synchronize()
        runs.append((loss, pred, grads, terms))
    loss, pred, grads, terms = runs[0]
    assert tuple(pred.shape) == (TO.N, TO.T, 1) and sorted(terms) == ['likelihood', 'power', 'total']
    for t in [loss] + list(terms.values()):
        assert t.dim() == 0 and t.is_cuda and t.dtype == torch.float32
    _check_grads(grads, ref['g64'], ref['E32'], 'L1 + %.4g power' % w)
    assert np.abs(pred.cpu().numpy().astype(np.float64) - ref['pred']).max() <= TOL_F32
    for k in ('likelihood', 'power', 'total'):
        print('%s %.9g (float64 %.9g)' % (k, float(terms[k]), ref['terms'][k]))
        assert abs(float(terms[k]) - ref['terms'][k]) <= 2e-6 * abs(ref['terms'][k]), k
    assert torch.equal(loss, terms['total'])
    # three float32 roundings (likelihood, power, total) of 6e-8 relative each
    combined = float(terms['likelihood']) + w * float(terms['power'])
    assert abs(float(loss) - combined) <= 3e-7 * abs(combined)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    for k in grads:
        assert torch.equal(grads[k], runs[1][2][k]), k
    for k in terms:
        assert torch.equal(terms[k], runs[1][3][k]), k


def test_power_weight_zero_and_none(small):
    """power_weight = 0.0 goes through the new loss head and gives the L1's gradients within the bar of the L1-only reference;
    power_weight = None is the path of before: bit-identical to its own repetition, and no new symbol is called."""
    from pwv_amd import train as TR
    model, _, wav, mel, z = small
    ref = TO.reference()
    called = []
    real = TR._call

    def spy(name, args):
        called.append(name)
        return real(name, args)

    TR._call = spy
    try:
        terms = {}
        loss0, pred0, grads0 = TR.loss_and_grad(model, wav, mel, z=z, power_weight=0.0, terms=terms)
        torch.cuda.synchronize()
        assert called.count('pwv_train_loss_f32') == 1
        del called[:]
        none = [TR.loss_and_grad(model, wav, mel, z=z) for _ in range(2)]
        torch.cuda.synchronize()
        assert called and not [c for c in called if 'loss' in c] and set(called) <= set(TR._lib.TRAIN_SYMBOLS)
    finally:
        TR._call = real
    _check_grads(grads0, ref['g64'], ref['E32'], 'power_weight 0')
    assert abs(float(loss0) - ref['loss']) <= 2e-6 * abs(ref['loss']) and float(terms['power']) == 0 and torch.equal(terms['likelihood'], loss0)
    _check_grads(none[0][2], ref['g64'], ref['E32'], 'power_weight None')
    assert torch.equal(none[0][0], none[1][0]) and torch.equal(none[0][1], none[1][1]) and torch.equal(none[0][1], pred0)
    for k in none[0][2]:
        assert torch.equal(none[0][2][k], none[1][2][k]), k


def test_training_with_the_power_loss_trains(small):
    """Five Trainer(power_weight=w).step calls on the fixed batch against five steps of the float64 restatement with the same loss: the
    total falls at every step, by at least half of the reference's decrease, and both terms end below where they started."""
    from pwv_amd import train as TR
    model, store, wav, mel, z = small
    w = PO.balanced_weight()
    ref = PO.trajectory(5)
    tr = TR.Trainer(model, lr=TO.LR, beta2=TO.BETA2, ema_decay=TO.DECAY, power_weight=w)
    seen = []
    for _ in range(5):
        loss = tr.step(wav, mel, z=z)
        assert torch.equal(loss, tr.terms['total'])
        seen.append({k: float(v) for k, v in tr.terms.items()})
    after = {}
    TR.loss_and_grad(model, wav, mel, z=z, power_weight=w, terms=after)
    seen.append({k: float(v) for k, v in after.items()})
    assert tr.steps == 5
    for k in ('likelihood', 'power', 'total'):
        print('gpu  %-10s' % k, ' '.join('%.6f' % s[k] for s in seen))
        print('fp64 %-10s' % k, ' '.join('%.6f' % s[k] for s in ref))
    totals = [s['total'] for s in seen]
    assert all(b < a for a, b in zip(totals, totals[1:])), totals
    assert ref[0]['total'] > ref[-1]['total']
    assert totals[0] - totals[-1] >= 0.5 * (ref[0]['total'] - ref[-1]['total'])
    assert seen[-1]['likelihood'] < seen[0]['likelihood'] and seen[-1]['power'] < seen[0]['power']


def test_train_cli_with_the_power_loss(gpu, tmp_path):
    """`python -m pwv_amd.train train/small_power --steps=2 --seed=4` in a fresh process: two step lines with finite loss/likelihood,
    loss/power and loss/total, and model-2.npz."""
    env = dict(os.environ, PWV_LOGDIR=str(tmp_path), PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = subprocess.run([sys.executable, '-m', 'pwv_amd.train', 'train/small_power', '--steps=2', '--seed=4'], cwd=ROOT, env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:]
    lines = [l.split() for l in out.stdout.splitlines() if l.startswith('step ')]
    assert len(lines) == 2, out.stdout[-2000:]
    for i, l in enumerate(lines):
        assert l[:2] == ['step', str(i + 1)] and l[2::2] == ['loss/likelihood', 'loss/power', 'loss/total'], l
        lik, power, total = (float(v) for v in l[3::2])
        assert np.isfinite([lik, power, total]).all() and lik > 0 and power > 0
        assert abs(total - (lik + 0.0005 * power)) <= 2e-6 + 1e-5 * total          # (six printed decimals)
    assert (tmp_path / 'model-2.npz').exists()
