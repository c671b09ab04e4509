"""GPU: the gradient arena and the fused optimiser (include/pwv_hip_train_opt.h, csrc/pwv_train_opt.hip) and the trainers on top of them
(train.Trainer(fused=True), train.DataParallelTrainer): pack / unpack against numpy bit for bit, one Adam + EMA launch against the float64
restatement of tests/train_oracle.py, ten fused steps against its trajectory, checkpoints across the two paths, a replicated trainer at
world size 1 over nccl and at world size 2, and `python -m pwv_amd.train train/small_dp`.

The bars are the ones of tests/test_gpu_train.py, formed the same way at run time: 8 x the error of the same computation in float32 on
the CPU.  Measured values are in DESIGN.md section 9, "Data-parallel training"."""
import json
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import train_oracle as TO
from tests.guarded import guarded
from tests.util import set_hparams

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 8
SIZES = (1, 3, 4, 5, 64, 8192, 4097)
UNALIGNED = 5                           # SIZES[5] = 8192 floats live one float behind a 16-byte line


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


# ---- pack / unpack -------------------------------------------------------------------------------------------------------------------------
def _tensors(TR, device, fill):
    """The seven tensors, allocated through TR.torch (the guard's proxy inside a guarded run); `fill(i, count)` -> float32 numpy."""
    out = []
    for i, c in enumerate(SIZES):
        if i == UNALIGNED:
            t = TR.torch.empty(c + 4, dtype=torch.float32, device=device)[1:1 + c]
            assert t.data_ptr() % 16 == 4 and t.is_contiguous()
        else:
            t = TR.torch.empty(c, dtype=torch.float32, device=device)
            assert t.data_ptr() % 16 == 0
        t.copy_(torch.from_numpy(fill(i, c)))
        out.append(t)
    return out


def _pack_unpack(TR, device):
    names = ['t%d' % i for i in range(len(SIZES))]
    lay = TR.arena_layout(names, [(c,) for c in SIZES])
    rng = np.random.RandomState(1)
    data = [rng.randn(c).astype(np.float32) for c in SIZES]
    data[2][:] = (np.nan, -0.0, np.inf, 1e-42)          # bits travel: a NaN, a signed zero, an infinity, a denormal
    src = _tensors(TR, device, lambda i, c: data[i])
    arena = TR.torch.zeros(lay.total, dtype=torch.float32, device=device)
    TR.arena_pack(src, lay, arena)
    want = np.zeros(lay.total, dtype=np.float32)
    for o, d in zip(lay.offsets, data):
        want[o:o + len(d)] = d
    got = arena.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    pad = np.ones(lay.total, dtype=bool)
    for o, c in zip(lay.offsets, lay.counts):
        pad[o:o + c] = False
    assert pad.sum() == sum(-c % 4 for c in SIZES) == 10 and (got.view(np.uint32)[pad] == 0).all()
    dst = _tensors(TR, device, lambda i, c: np.full(c, np.nan, dtype=np.float32))
    TR.arena_unpack(dst, lay, arena)
    for t, d in zip(dst, data):
        assert np.array_equal(t.cpu().numpy().view(np.uint32), d.view(np.uint32))
    return lay


def test_pack_unpack_bit_for_bit(gpu):
    """Seven tensors of 1, 3, 4, 5, 64, 8192 and 4097 floats (several chunks, tails of 1, 3, 1 and 1 floats, one tensor whose address is
    only 4-byte aligned) into an arena and back: the arena is numpy's bit for bit, its 10 padding floats are still zero, unpack into
    NaN-filled tensors gives the originals back."""
    from pwv_amd import train as TR
    lay = _pack_unpack(TR, gpu)
    assert lay.total == sum((c + 3) // 4 * 4 for c in SIZES)


def test_pack_unpack_guarded(gpu):
    """The same inside poisoned, guard-banded buffers: no store outside a tensor or the arena."""
    from pwv_amd import train as TR
    with guarded(TR) as g:
        _pack_unpack(TR, gpu)
        torch.cuda.synchronize()
        g.check()
        assert len(g.allocations) >= 2 * len(SIZES) + 1 and any('train.py' in s or 'test_gpu_train_opt.py' in s for s in g.sites())


# ---- one Adam + EMA launch -----------------------------------------------------------------------------------------------------------------
def _adam_inputs():
    rng = np.random.RandomState(2)
    names = ['v%d' % i for i in range(len(SIZES))]
    f32 = lambda a: a.astype(np.float32)
    var = {n: f32(0.3 * rng.randn(c)) for n, c in zip(names, SIZES)}
    m = {n: f32(1e-2 * rng.randn(c)) for n, c in zip(names, SIZES)}
    v = {n: f32(1e-4 * rng.rand(c)) for n, c in zip(names, SIZES)}
    shadow = {n: f32(var[n] + 1e-3 * rng.randn(c)) for n, c in zip(names, SIZES)}
    g = {n: f32(np.sign(rng.randn(c)) * 10.0 ** rng.uniform(-12, 3, c)) for n, c in zip(names, SIZES)}       # |g| from 1e-12 to 1e3
    big = names[5]
    g[big][:64] = 0.0                   # g = 0
    v[big][32:128] = 0.0                # v = 0, with and without a gradient
    m[big][32:48] = 0.0                 # ... and m = v = g = 0: 0 / (0 + eps)
    g[names[6]][-1], g[names[6]][-2] = 1e3, 1e-12
    return names, var, m, v, shadow, g


@pytest.mark.parametrize('decay', [TO.DECAY, None], ids=['ema', 'no_ema'])
@pytest.mark.parametrize('scale', [1.0, 0.5])
@pytest.mark.parametrize('t', [1, 1000])
def test_adam_ema_matches_float64(gpu, t, scale, decay):
    """One pwv_train_opt_adam_ema_f32 launch from random var, m, v, shadow, g against train_oracle.adam_ema_numpy in float64 on the same
    float32 inputs: per array (var, m, v, shadow) the largest absolute error is at most 8 x D32, the error of the same restatement run in
    float32, computed here -- and the result IS that float32 restatement, bit for bit (numpy's float32 operations are the IEEE ones the
    header lists).  Twice the same inputs: the same bits.  With the EMA off the shadow arena is not touched."""
    from pwv_amd import train as TR
    names, var, m, v, shadow, g = _adam_inputs()
    lr_t = TO.LR * math.sqrt(1.0 - TO.BETA2 ** t) / (1.0 - TO.BETA1 ** t)
    sg = {n: (np.float32(scale) * a).astype(np.float32) for n, a in g.items()}           # (exact: scale is 1 or 0.5)

    def restated(dt):
        W, M, V, S = ({n: a.astype(dt) for n, a in d.items()} for d in (var, m, v, shadow))
        TO.adam_ema_numpy(W, M, V, S, {n: a.astype(dt) for n, a in sg.items()}, t)
        assert all(a.dtype == dt for d in (W, M, V, S) for a in d.values())
        return {'var': W, 'm': M, 'v': V, 'shadow': S}

    r64, r32 = restated(np.float64), restated(np.float32)

    def run():
        fill = {i: var[n] for i, n in enumerate(names)}
        tensors = _tensors(TR, gpu, lambda i, c: fill[i])
        ar = TR._Arenas(names, tensors, ema=True)
        assert ar.layout.names == names
        for arena, d in ((ar.grad, g), (ar.m, m), (ar.v, v), (ar.shadow, shadow)):
            for view, n in zip(ar.layout.views(arena), names):
                view.copy_(torch.from_numpy(d[n]))
        ar.adam_ema(lr_t, TO.BETA1, TO.BETA2, TO.EPS, decay, scale)
        torch.cuda.synchronize()
        out = {'var': {n: x.cpu().numpy() for n, x in zip(names, tensors)}}
        for key, arena in (('m', ar.m), ('v', ar.v), ('shadow', ar.shadow), ('grad', ar.grad)):
            out[key] = {n: x.cpu().numpy() for n, x in zip(names, ar.layout.views(arena))}
        out['raw'] = [a.cpu().numpy() for a in (ar.grad, ar.m, ar.v, ar.shadow)]
        return out

    got, again = run(), run()
    for key in ('var', 'm', 'v', 'shadow', 'grad'):
        for n in names:
            assert np.array_equal(got[key][n].view(np.uint32), again[key][n].view(np.uint32)), (key, n)
            assert np.array_equal(got['grad'][n], g[n])                                     # the gradients are only read
    pad = np.ones(got['raw'][0].size, dtype=bool)
    lay = TR.arena_layout(names, [(c,) for c in SIZES])
    for o, c in zip(lay.offsets, lay.counts):
        pad[o:o + c] = False
    assert all((a.view(np.uint32)[pad] == 0).all() for a in got['raw'])                   # padding is never written
    for key in ('var', 'm', 'v') + (('shadow',) if decay is not None else ()):
        err = max(float(np.abs(got[key][n].astype(np.float64) - r64[key][n]).max()) for n in names)
        d32 = max(float(np.abs(r32[key][n].astype(np.float64) - r64[key][n]).max()) for n in names)
        same = sum(int((got[key][n].view(np.uint32) != r32[key][n].view(np.uint32)).sum()) for n in names)
        print('t=%d scale=%g decay=%s %s: err %.3g, D32 %.3g, bar %.3g; %d of %d elements differ from the float32 restatement'
              % (t, scale, decay, key, err, d32, MARGIN * d32, same, sum(SIZES)))
        assert all(np.isfinite(got[key][n]).all() for n in names), key
        assert d32 > 0 and err <= MARGIN * d32, (key, err, d32)
        assert same == 0, (key, same)          # the header's promise: the float32 statements, one rounding each, nothing fused
    if decay is None:
        for n in names:
            assert np.array_equal(got['shadow'][n].view(np.uint32), shadow[n].view(np.uint32)), n


# ---- the fused trainer ---------------------------------------------------------------------------------------------------------------------
def _model(device, n=TO.N):
    from pwv_amd.models import IAFVocoder
    from pwv_amd.variables import VariableStore
    cfg, w, mel, z, wav = TO.problem()
    set_hparams(cfg)
    store = VariableStore(device=device)
    store.load_dict(w)
    model = IAFVocoder(batch_size=n, length=TO.T, store=store, precision='f32')
    return model, store, _dev(wav, device), _dev(mel, device), _dev(z, device)


def test_fused_training_follows_the_trajectory(gpu):
    """Ten Trainer(fused=True).step calls on the fixed batch against ten steps of the float64 restatement, with the bars of
    tests/test_gpu_train.py::test_training_trains formed the same way: the loss falls at every step, by at least half of the
    reference's decrease, and every shadow stays within 8 D32 of the restatement's, D32 = the largest |shadow - shadow64| of the same
    restatement run in float32."""
    from pwv_amd import train as TR
    ref_losses, ref_shadow = TO.trajectory(10)
    _, shadow32 = TO.trajectory(10, single=True)
    d32 = max(float(np.abs(shadow32[k].astype(np.float64) - ref_shadow[k]).max()) for k in ref_shadow)
    model, store, wav, mel, z = _model(gpu)
    tr = TR.Trainer(model, lr=TO.LR, beta2=TO.BETA2, ema_decay=TO.DECAY, fused=True)
    version = store.version
    losses = [float(tr.step(wav, mel, z=z)) for _ in range(10)]
    assert store.version > version and tr.steps == 10 and tr.fused
    loss_after, _, _ = TR.loss_and_grad(model, wav, mel, z=z)
    losses.append(float(loss_after))
    print('fused', ' '.join('%.5f' % v for v in losses))
    print('fp64 ', ' '.join('%.5f' % v for v in ref_losses))
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    assert losses[0] - losses[-1] >= 0.5 * (ref_losses[0] - ref_losses[-1])
    shadows = tr.shadows()
    assert sorted(shadows) == sorted(ref_shadow)
    errs = {k: float(np.abs(shadows[k].cpu().numpy().astype(np.float64) - want).max()) for k, want in ref_shadow.items()}
    print('largest shadow difference %.3g (D32 %.3g, bar %.3g)' % (max(errs.values()), d32, MARGIN * d32))
    for k, err in errs.items():
        assert err <= MARGIN * d32, (k, err, d32)
    moved = max(float(np.abs(ref_shadow[k] - TO.problem()[1][k]).max()) for k in ref_shadow)
    assert MARGIN * d32 < 0.5 * moved, (d32, moved)
    # the state is views into the arenas, and the unread variables' gradient slots are the zeros they started as
    ar = tr.arenas
    assert all(s.data_ptr() >= ar.shadow.data_ptr() and s.data_ptr() < ar.shadow.data_ptr() + 4 * ar.shadow.numel() for s in tr.state['shadow'])
    unread = [k for k, v in TO.reference()['g64'].items() if v is None]
    grads = tr.gradients()
    assert len(unread) == 32 and all(float(grads[k].abs().max()) == 0 for k in unread)


def _everything(tr):
    out = {'var/' + n: tr.store.vars[n] for n in tr.names}
    for key in ('m', 'v', 'shadow'):
        out.update({key + '/' + n: t for n, t in zip(tr.names, tr.state[key])})
    return {k: t.detach().cpu().numpy().copy() for k, t in out.items()}


@pytest.mark.parametrize('writer', [True, False], ids=['fused_to_unfused', 'unfused_to_fused'])
def test_checkpoints_cross_the_two_paths(gpu, tmp_path, writer):
    """save from a fused trainer, load into an unfused one, and the reverse: variables, m, v and shadows are bit-equal and the step
    count is kept; the loaded trainer then takes a step."""
    from pwv_amd import train as TR
    kw = dict(lr=TO.LR, beta2=TO.BETA2, ema_decay=TO.DECAY)
    model, _, wav, mel, z = _model(gpu)
    a = TR.Trainer(model, fused=writer, **kw)
    for _ in range(2):
        a.step(wav, mel, z=z)
    path = str(tmp_path / 'ckpt.npz')
    a.save(path)
    model_b, _, _, _, _ = _model(gpu)
    b = TR.Trainer(model_b, fused=not writer, **kw)
    assert b.load(path) == 2 and b.steps == 2
    ea, eb = _everything(a), _everything(b)
    assert sorted(ea) == sorted(eb) and len(ea) == 4 * len(a.names)
    for k in ea:
        assert np.array_equal(ea[k].view(np.uint32), eb[k].view(np.uint32)), k
    assert np.isfinite(float(b.step(wav, mel, z=z))) and b.steps == 3


def test_step_varlen_runs_fused(gpu):
    """Two packed steps of utterances of 208 and 96 samples with per-utterance seeds (the same noise at both steps) on the fused path:
    a finite, falling loss, and the first loss has the bits of the unfused trainer's (the same call, before any update)."""
    from pwv_amd import train as TR
    losses = {}
    for fused in (True, False):
        model, _, wav, mel, _ = _model(gpu)
        tr = TR.Trainer(model, lr=TO.LR, beta2=TO.BETA2, ema_decay=TO.DECAY, fused=fused)
        wavs = [wav[0, :, 0].contiguous(), wav[1, :96, 0].contiguous()]
        mels = [mel[0].contiguous(), mel[1, :1 + 96 // TO.HOP].contiguous()]
        losses[fused] = [float(tr.step_varlen(wavs, mels, seeds=[11, 12])) for _ in range(2)]
        assert tr.steps == 2
    assert np.isfinite(losses[True]).all() and losses[True][1] < losses[True][0]
    assert losses[True][0] == losses[False][0]
    assert np.isfinite(losses[False]).all()


# ---- replicas ------------------------------------------------------------------------------------------------------------------------------
def _child_env():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT', 'MASTER_ADDR', 'PWV_TRAIN_DRYRUN_ONE_GPU'):
        env.pop(k, None)
    return env


def test_world_size_one_over_nccl_gives_the_fused_bits(gpu, tmp_path):
    """In a child process: DataParallelTrainer at world size 1 over nccl (RCCL) -- the broadcast and the all-reduce on the device arena
    -- leaves, after 3 steps with drawn noise, the bits of Trainer(fused=True): every variable, m, v and shadow."""
    out = str(tmp_path / 'nccl1.json')
    res = subprocess.run([sys.executable, '-m', 'tests.train_opt_worker', 'nccl1', out], cwd=ROOT, env=_child_env(), stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-3000:]
    j = json.load(open(out))
    assert j['backend'] == 'nccl' and j['world'] == 1 and j['steps'] == 3
    assert j['differ'] == [] and j['arrays'] > 0 and j['arrays'] % 4 == 0
    assert j['losses_dp'] == j['losses_one'] and j['mean_loss'] == j['losses_dp'][-1]
    assert j['offsets'] == [3 * TO.N * TO.T] * 2          # both drew the counters 0 .. 3 N T - 1


@pytest.fixture(scope='module')
def two_ranks(tmp_path_factory):
    """Two fresh child processes under one timeout, one utterance of the N = 2 problem each, 3 steps; a child that fails or times out
    fails the test, nothing is retried.  Returns the directory the ranks wrote into."""
    out = str(tmp_path_factory.mktemp('two_ranks'))
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(2):
        env = dict(_child_env(), RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE='2', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, '-m', 'tests.train_opt_worker', 'rank', out], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    logs, failed = [], False
    for p in procs:
        try:
            log, _ = p.communicate(timeout=300 if not failed else 5)
        except subprocess.TimeoutExpired:
            p.kill()
            log, _ = p.communicate()
            log += '\n(timed out)'
            failed = True
        failed = failed or p.returncode != 0
        logs.append(log)
    assert not failed and all(p.returncode == 0 for p in procs), '\n----\n'.join(l[-3000:] for l in logs)
    return out


def test_two_ranks_average_the_gradients_of_the_whole_batch(gpu, two_ranks):
    """After the first all-reduce the gradient arena, times 1 / world, is the gradient of the whole N = 2 batch: per variable rel_err
    against float64 autograd of that batch <= 8 E32, the criterion of tests/test_gpu_train.py; the unread variables are exact zeros;
    both ranks hold the same bits."""
    ref = TO.reference()
    g64, bar = ref['g64'], MARGIN * ref['E32']
    with np.load(os.path.join(two_ranks, 'grads_rank0.npz')) as z0, np.load(os.path.join(two_ranks, 'grads_rank1.npz')) as z1:
        g0, g1 = {k: z0[k] for k in z0.files}, {k: z1[k] for k in z1.files}
    assert sorted(g0) == sorted(g1) == sorted(g64)
    worst = 0.0
    for k, want in g64.items():
        assert np.array_equal(g0[k].view(np.uint32), g1[k].view(np.uint32)), k
        got = g0[k].astype(np.float64) * 0.5
        if want is None:
            assert np.abs(got).max() == 0, k
            continue
        assert got.shape == want.shape and np.isfinite(got).all(), k
        err = TO.rel_err(got, want)
        worst = max(worst, err)
        assert err <= bar, (k, err, bar)
    print('two ranks: worst gradient err %.3g (E32 %.3g, bar %.3g)' % (worst, ref['E32'], bar))
    info = [json.load(open(os.path.join(two_ranks, 'info_rank%d.json' % r))) for r in range(2)]
    assert [i['rank'] for i in info] == [0, 1] and all(i['world'] == 2 and i['steps'] == 3 for i in info)
    assert info[0]['backend'] == info[1]['backend'] == ('nccl' if torch.cuda.device_count() >= 2 else 'gloo')
    # the mean of the local losses of the first step is the loss of the whole batch
    assert abs(0.5 * (info[0]['losses'][0] + info[1]['losses'][0]) - ref['loss']) <= 2e-6 * max(1.0, abs(ref['loss']))
    assert info[0]['mean_loss'] == info[1]['mean_loss']


def test_two_ranks_stay_bit_identical(gpu, two_ranks):
    """After 3 steps every variable, m, v and shadow is bit-identical on the two ranks, they have moved, and rank 0 alone wrote a
    checkpoint."""
    with np.load(os.path.join(two_ranks, 'state_rank0.npz')) as z0, np.load(os.path.join(two_ranks, 'state_rank1.npz')) as z1:
        s0, s1 = {k: z0[k] for k in z0.files}, {k: z1[k] for k in z1.files}
    assert sorted(s0) == sorted(s1) and len(s0) == 4 * len(TO.problem()[1])
    for k in s0:
        assert np.array_equal(s0[k].view(np.uint32), s1[k].view(np.uint32)), k
    w = TO.problem()[1]
    assert max(float(np.abs(s0['var/' + k] - w[k]).max()) for k in w) > 0.5 * TO.LR
    assert os.path.exists(os.path.join(two_ranks, 'ckpt_rank0.npz')) and not os.path.exists(os.path.join(two_ranks, 'ckpt_rank1.npz'))
    with np.load(os.path.join(two_ranks, 'ckpt_rank0.npz')) as z:
        assert int(z['global_step']) == 3
        for k in w:
            assert np.array_equal(z[k], s0['var/' + k]) and np.array_equal(z[k + '/Adam_1'], s0['v/' + k])


def test_train_cli_data_parallel(gpu, tmp_path):
    """`python -m pwv_amd.train train/small_dp --steps 2` starts two ranks (on one GPU: both on it, over gloo -- the dry run), exits 0
    and prints two step lines and one `saved`; the checkpoint is there."""
    env = dict(_child_env(), PWV_LOGDIR=str(tmp_path))
    if torch.cuda.device_count() < 2:
        env['PWV_TRAIN_DRYRUN_ONE_GPU'] = '1'
    out = subprocess.run([sys.executable, '-m', 'pwv_amd.train', 'train/small_dp', '--steps', '2'], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith('step ')]
    assert len(lines) == 2 and all('loss/likelihood' in l and np.isfinite(float(l.split()[-1])) for l in lines), out.stdout[-2000:]
    assert len([l for l in out.stdout.splitlines() if l.startswith('saved ')]) == 1, out.stdout[-2000:]
    assert (tmp_path / 'model-2.npz').exists()
