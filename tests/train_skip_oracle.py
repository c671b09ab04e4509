"""The yardstick of the tests of training the skip-connection architecture (model.use_skip_connection True): the small model of
tests/train_oracle.py with the switch set, its problems and float64 / float32 autograd references for uniform and packed batches -- all
through tests.train_oracle.forward / loss_and_grads / draw_wav / relu_margin and tests.train_varlen_oracle.loss_and_grads, whose
oracle.torch_cpu._wavenet takes use_skip --, the Adam / EMA trajectory, and a float64-autograd restatement of ONE skip layer and of the
head on the skip sum S for the kernel-level tests.  Nothing here runs on a GPU or calls the package's training code."""
import functools

import numpy as np
import torch

from oracle import iaf_oracle as O
from tests import train_oracle as TO
from tests import train_varlen_oracle as VO

LIVE, DEAD = 173, 8                     # variables of the small skip model with / without a gradient (the last layer's dense, dense_bias)


def small_cfg(hop=TO.HOP):
    return O.ModelConfig(dilations=[[1, 2, 32, 64], [4, 48, 256, 3]], n_iaf=2, hop_length=hop, use_skip_connection=True)


@functools.lru_cache(maxsize=None)
def weights():
    return O.init_weights(small_cfg(), seed=3)


# ---- the whole model, uniform batches --------------------------------------------------------------------------------------------------
def problem(N=TO.N, T=TO.T, hop=TO.HOP):
    """(cfg, weights, mel, z, wav) of the small skip model on N x T samples at hop length `hop`; asserts the two input margins of
    tests.train_oracle."""
    return _problem(int(N), int(T), int(hop))


@functools.lru_cache(maxsize=None)
def _problem(N, T, hop):
    cfg, w = small_cfg(hop), weights()
    mel, z = O.synthetic_inputs(N, T, cfg)
    assert TO.relu_margin(w, mel) >= TO.RELU_MARGIN, 'a conditioning pre-activation sits on the ReLU: draw another seed'
    wav, = TO.draw_wav([TO.pred64(w, mel, z, cfg)], TO.WAV_SEED, [(N, T, 1)])
    assert float(np.abs(TO.pred64(w, mel, z, cfg) - wav).min()) >= TO.SIGN_MARGIN
    return cfg, w, mel, z, wav


def reference(N=TO.N, T=TO.T, hop=TO.HOP):
    """{'loss', 'pred', 'g64', 'g32', 'E32'} as tests.train_oracle.reference, of the skip model."""
    return _reference(int(N), int(T), int(hop))


@functools.lru_cache(maxsize=None)
def _reference(N, T, hop):
    cfg, w, mel, z, wav = problem(N, T, hop)
    l64, p64, g64 = TO.loss_and_grads(w, mel, z, wav, cfg, torch.float64)
    _, _, g32 = TO.loss_and_grads(w, mel, z, wav, cfg, torch.float32)
    return {'loss': l64, 'pred': p64, 'g64': g64, 'g32': g32, 'E32': max(TO.rel_err(g32[k], v) for k, v in g64.items() if v is not None)}


# ---- packed batches ---------------------------------------------------------------------------------------------------------------------
def packed_problem(lengths=tuple(VO.LENGTHS), hop=VO.HOP):
    """(cfg, weights, mels, zs, wavs) as tests.train_varlen_oracle.problem (the same seeds per utterance), of the skip model."""
    return _packed_problem(tuple(int(T) for T in lengths), int(hop))


@functools.lru_cache(maxsize=None)
def _packed_problem(lengths, hop):
    cfg, w = small_cfg(hop), weights()
    mels, zs = [], []
    for i, T in enumerate(lengths):
        mel, z = O.synthetic_inputs(1, T, cfg, mel_seed=20 + i, z_seed=40 + i)
        mels.append(mel)
        zs.append(z)
    assert min(TO.relu_margin(w, mel) for mel in mels) >= TO.RELU_MARGIN, 'a conditioning pre-activation sits on the ReLU: draw another seed'
    preds = [TO.pred64(w, mel, z, cfg) for mel, z in zip(mels, zs)]
    wavs = TO.draw_wav(preds, VO.WAV_SEED, [(1, T, 1) for T in lengths])
    assert min(float(np.abs(p - y).min()) for p, y in zip(preds, wavs)) >= TO.SIGN_MARGIN
    return cfg, w, mels, zs, wavs


def packed_reference(lengths=tuple(VO.LENGTHS), hop=VO.HOP):
    """{'terms', 'preds', 'g64', 'g32', 'E32'} as tests.train_varlen_oracle.reference (the L1 alone), of the skip model."""
    return _packed_reference(tuple(int(T) for T in lengths), int(hop))


@functools.lru_cache(maxsize=None)
def _packed_reference(lengths, hop):
    cfg, w, mels, zs, wavs = packed_problem(lengths, hop)
    t64, p64, g64 = VO.loss_and_grads(w, mels, zs, wavs, cfg, torch.float64)
    _, _, g32 = VO.loss_and_grads(w, mels, zs, wavs, cfg, torch.float32)
    return {'terms': t64, 'preds': p64, 'g64': g64, 'g32': g32, 'E32': max(TO.rel_err(g32[k], v) for k, v in g64.items() if v is not None)}


# ---- the optimiser's trajectory ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def trajectory(steps=5, single=False):
    """tests.train_oracle.trajectory on the skip model's fixed batch: (losses before each update + the loss after the last, shadows)."""
    cfg, w, mel, z, wav = problem()
    dt, tdt = (np.float32, torch.float32) if single else (np.float64, torch.float64)
    W = {k: a.astype(dt) for k, a in w.items()}
    m = {k: np.zeros_like(a) for k, a in W.items()}
    v = {k: np.zeros_like(a) for k, a in W.items()}
    shadow = {k: a.copy() for k, a in W.items()}
    losses = []
    for t in range(1, steps + 1):
        l, _, g = TO.loss_and_grads(W, mel, z, wav, cfg, tdt)
        losses.append(l)
        TO.adam_ema_numpy(W, m, v, shadow, {k: (a.astype(dt) if a is not None else None) for k, a in g.items()}, t)
        assert all(a.dtype == dt for a in list(W.values()) + list(shadow.values()))
    losses.append(TO.loss_only(W, mel, z, wav, cfg))
    return losses, shadow


# ---- one skip layer and the head on S ----------------------------------------------------------------------------------------------------
def to_tile32(a):
    """tests.train_oracle.to_tile32 (NaN padding rows) for any channel count that is a multiple of 4."""
    return TO.to_tile32(a)


def layer_case(d, N, T, hop, offset, seed=11):
    """A uniform one-layer case in the flat form both geometries share: tests.train_oracle.layer_case (x, P, the weights, g, dy) on the
    rows one after the other, + S_in and dS [rows, 128], cu_rows and, per row, its P row `fidx`."""
    c = dict(TO.layer_case(d, seed=seed, hop=hop, N=N, T=T, offset=offset))
    rows = N * T
    rng = np.random.RandomState(seed + d + 2000)
    t = np.arange(rows) % T
    c.update(x=c['x'].reshape(rows, 64), g=c['g'].reshape(rows, 64), dy=c['dy'].reshape(rows), rows=rows,
             cu_rows=[n * T for n in range(N + 1)], fidx=(np.arange(rows) // T) * c['frames'] + (t + offset) // hop,
             S_in=rng.randn(rows, 128).astype(np.float32), dS=rng.randn(rows, 128).astype(np.float32))
    return c


def packed_layer_case(d, lengths, hop, seed=11):
    """The same on a packed batch: tests.train_varlen_oracle.layer_case + S_in, dS, fidx."""
    c = dict(VO.layer_case(d, seed=seed, lengths=tuple(lengths), hop=hop))
    rows = c['cu_rows'][-1]
    rng = np.random.RandomState(seed + d + 3000)
    fidx = np.concatenate([c['cu_frames'][i] + (np.arange(T) + hop // 2) // hop for i, T in enumerate(lengths)])
    c.update(rows=rows, offset=hop // 2, fidx=fidx, S_in=rng.randn(rows, 128).astype(np.float32), dS=rng.randn(rows, 128).astype(np.float32))
    return c


def skip_layer(c, last, dtype, accumulate=True):
    """One skip layer by autograd in `dtype` (include/pwv_hip_train_skip.h): x, P, S_in, g, dS ->
        x_out = x + o dense + dense_bias (not `last`),  S_out = S_in + (o skip + skip_bias)  (S_in = 0 unless `accumulate`)
    and, under sum(x_out g) + sum(S_out dS): U (the gradient of the tap at t), V (of the tap at t - d, at the row that READ it), P,
    filter, gate, dense, dense_bias, skip, skip_bias.  The look-back stops at an utterance's first row.  float64 numpy."""
    d, rows, cu = c['d'], c['rows'], c['cu_rows']
    names = ('P', 'filter', 'gate', 'skip', 'skip_bias') + (() if last else ('dense', 'dense_bias'))
    v = {k: torch.from_numpy(c[k]).to(dtype).requires_grad_(True) for k in names}
    x = torch.from_numpy(c['x']).to(dtype).requires_grad_(True)
    back = np.zeros((rows, 64), dtype=np.float32)
    for a, b in zip(cu, cu[1:]):
        if d < b - a:
            back[a + d:b] = c['x'][a:b - d]
    xd = torch.from_numpy(back).to(dtype).requires_grad_(True)
    p = v['P'][torch.from_numpy(np.asarray(c['fidx'], dtype=np.int64))]
    F = xd @ v['filter'][0] + x @ v['filter'][1] + p[:, :64]
    G = xd @ v['gate'][0] + x @ v['gate'][1] + p[:, 64:]
    o = torch.tanh(F) * torch.sigmoid(G)
    term = o @ v['skip'][0] + v['skip_bias']
    S_out = torch.from_numpy(c['S_in']).to(dtype) + term if accumulate else term
    loss = (S_out * torch.from_numpy(c['dS']).to(dtype)).sum()
    out = {}
    if not last:
        x_out = x + o @ v['dense'][0] + v['dense_bias']
        loss = loss + (x_out * torch.from_numpy(c['g']).to(dtype)).sum()
        out['x_out'] = x_out.detach().double().numpy()
    loss.backward()
    out.update({k: t.grad.double().numpy() for k, t in v.items()})
    out.update(S_out=S_out.detach().double().numpy(), U=x.grad.double().numpy(), V=xd.grad.double().numpy())
    return out


GRADS_RESIDUAL = ('U', 'V', 'P', 'filter', 'gate', 'dense', 'dense_bias', 'skip')
GRADS_LAST = ('U', 'V', 'P', 'filter', 'gate', 'skip')


def skip_head(c, dtype):
    """The head on S = c['S_in'] by autograd in `dtype` under sum(y dy): y [rows], dS [rows, 128], post1, post1_bias, post2, post2_bias and
    skip_bias = the column sums of dS (every layer's d skip_bias).  float64 numpy."""
    S = torch.from_numpy(c['S_in']).to(dtype).requires_grad_(True)
    v = {k: torch.from_numpy(c[k]).to(dtype).requires_grad_(True) for k in ('post1', 'post1_bias', 'post2', 'post2_bias')}
    y = torch.relu(torch.relu(S) @ v['post1'][0] + v['post1_bias']) @ v['post2'][0] + v['post2_bias']
    (y[:, 0] * torch.from_numpy(c['dy']).to(dtype)).sum().backward()
    out = {k: t.grad.double().numpy() for k, t in v.items()}
    out.update(y=y.detach().double().numpy()[:, 0], dS=S.grad.double().numpy(), skip_bias=S.grad.double().numpy().sum(axis=0))
    return out
