"""The yardstick of the training tests: the L1 loss of the student restated on top of oracle.torch_cpu._wavenet (differentiable torch
ops on the CPU), its gradients by autograd in float64 / float32, TensorFlow's Adam and the reference's EMA in numpy float64, and one
gated layer (+ head) for the kernel-level test.  Nothing here runs on a GPU or calls the package's training code."""
import functools

import numpy as np
import torch

from oracle import iaf_oracle as O
from oracle import torch_cpu as TC

N, T = 2, 208
LR, BETA1, BETA2, EPS, DECAY = 2e-4, 0.9, 0.999, 1e-8, 0.998


def small_cfg():
    return O.ModelConfig(dilations=[[1, 2, 32, 64], [4, 48, 256, 3]], n_iaf=2, hop_length=16)


@functools.lru_cache(maxsize=None)
def problem():
    """(cfg, weights, mel, z, wav) of the small model: 2 x 208 samples, hop 16."""
    cfg = small_cfg()
    w = O.init_weights(cfg, seed=3)
    mel, z = O.synthetic_inputs(N, T, cfg)
    wav = (0.3 * np.random.RandomState(5).randn(N, T, 1)).astype(np.float32)
    return cfg, w, mel, z, wav


def forward(W, melt, x, cfg):
    hop = cfg.hop_length
    c = torch.relu(melt @ W['iaf_vocoder/cond/dense'][0])
    cond = c.repeat_interleave(hop, dim=1)[:, hop // 2: -(hop // 2), :]
    for i in range(cfg.n_iaf):
        outs = [TC._wavenet(W, 'iaf_vocoder/iaf%d/%s' % (i, net), x, cond, cfg.dilations[i], cfg.use_biases, cfg.use_skip_connection)
                for net in O.net_names(cfg)]
        x = x * outs[0] + outs[1]
    return x


def loss_and_grads(weights, mel, z, wav, cfg, dtype):
    """(loss, pred [N, T, 1] float64 numpy, {name: float64 numpy gradient, or None for a variable the loss does not depend on})."""
    W = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype).requires_grad_(True) for k, v in weights.items()}
    pred = forward(W, torch.from_numpy(mel).to(dtype), torch.from_numpy(z).to(dtype), cfg)
    loss = (pred - torch.from_numpy(wav).to(dtype)).abs().mean()
    loss.backward()
    return float(loss.detach()), pred.detach().double().numpy(), {k: (v.grad.double().numpy() if v.grad is not None else None) for k, v in W.items()}


def loss_only(weights, mel, z, wav, cfg):
    with torch.no_grad():
        W = {k: torch.from_numpy(np.ascontiguousarray(v)).double() for k, v in weights.items()}
        pred = forward(W, torch.from_numpy(mel).double(), torch.from_numpy(z).double(), cfg)
        return float((pred - torch.from_numpy(wav).double()).abs().mean())


@functools.lru_cache(maxsize=None)
def reference():
    """{'loss', 'pred', 'g64', 'g32', 'E32'}: float64 and float32 autograd of the small problem; E32 = max over the variables of
    max|g32 - g64| / max|g64|."""
    cfg, w, mel, z, wav = problem()
    l64, p64, g64 = loss_and_grads(w, mel, z, wav, cfg, torch.float64)
    _, _, g32 = loss_and_grads(w, mel, z, wav, cfg, torch.float32)
    return {'loss': l64, 'pred': p64, 'g64': g64, 'g32': g32, 'E32': max(rel_err(g32[k], v) for k, v in g64.items() if v is not None)}


def rel_err(got, want):
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / np.abs(want).max())


def adam_ema_numpy(W, m, v, shadow, grads, t, lr=LR, beta1=BETA1, beta2=BETA2, eps=EPS, decay=DECAY):
    """Step t (1-based) of tf.train.AdamOptimizer, then the EMA, in place on dicts of float64 arrays; a gradient of None leaves its
    variable alone apart from the EMA (which then moves nothing)."""
    lr_t = float(lr * np.sqrt(1 - beta2 ** t) / (1 - beta1 ** t))       # (a Python float: float32 arrays stay float32)
    for k in W:
        g = grads[k] if grads[k] is not None else np.zeros_like(W[k])
        m[k] = beta1 * m[k] + (1 - beta1) * g
        v[k] = beta2 * v[k] + (1 - beta2) * g * g
        W[k] = W[k] - lr_t * m[k] / (np.sqrt(v[k]) + eps)
        shadow[k] = shadow[k] - (1 - decay) * (shadow[k] - W[k])


@functools.lru_cache(maxsize=None)
def trajectory(steps=10, single=False):
    """(losses before each of `steps` updates + the loss after the last, the shadows after the last) of training on the fixed batch with
    the restatement: float64 throughout, or -- `single` -- with everything a float32 implementation rounds: variables, moments and shadows
    kept in float32, gradients from float32 autograd."""
    cfg, w, mel, z, wav = problem()
    dt, tdt = (np.float32, torch.float32) if single else (np.float64, torch.float64)
    W = {k: a.astype(dt) for k, a in w.items()}
    m = {k: np.zeros_like(a) for k, a in W.items()}
    v = {k: np.zeros_like(a) for k, a in W.items()}
    shadow = {k: a.copy() for k, a in W.items()}
    losses = []
    for t in range(1, steps + 1):
        l, _, g = loss_and_grads(W, mel, z, wav, cfg, tdt)
        losses.append(l)
        adam_ema_numpy(W, m, v, shadow, {k: (a.astype(dt) if a is not None else None) for k, a in g.items()}, t)
        assert all(a.dtype == dt for a in list(W.values()) + list(shadow.values()))
    losses.append(loss_only(W, mel, z, wav, cfg))
    return losses, shadow


# ---- one layer ----------------------------------------------------------------------------------------------------------------------
def to_tile32(a):
    """[rows, C] -> the flat tile32 buffer (include/pwv_hip.h): whole blocks of 32 rows, [C/4][32][4] each; padding rows are NaN."""
    rows, C = a.shape
    blocks = (rows + 31) // 32
    pad = np.full((blocks * 32, C), np.nan, dtype=np.float32)
    pad[:rows] = a
    return np.ascontiguousarray(pad.reshape(blocks, 32, C // 4, 4).transpose(0, 2, 1, 3)).reshape(-1)


def from_tile32(buf, rows, C):
    blocks = (rows + 31) // 32
    return np.asarray(buf).reshape(blocks, C // 4, 32, 4).transpose(0, 2, 1, 3).reshape(blocks * 32, C)[:rows]


def layer_case(d, seed=11, hop=16):
    """Inputs of one gated layer on 2 x 208 rows: x [N, T, 64], P [N * frames, 128] (natural column order), the weights in TF
    layouts, g [N, T, 64] for the residual form and dy [N, T] for the last-layer + head form."""
    rng = np.random.RandomState(seed + d)
    frames = 1 + T // hop
    f32 = lambda a: a.astype(np.float32)
    c = {'d': d, 'hop': hop, 'frames': frames,
         'x': f32(rng.randn(N, T, 64)), 'P': f32(0.5 * rng.randn(N * frames, 128)),
         'filter': f32(0.15 * rng.randn(2, 64, 64)), 'gate': f32(0.15 * rng.randn(2, 64, 64)),
         'dense': f32(0.15 * rng.randn(1, 64, 64)), 'dense_bias': f32(0.1 * rng.randn(64)),
         'skip': f32(0.15 * rng.randn(1, 64, 128)), 'skip_bias': f32(0.1 * rng.randn(128)),
         'post1': f32(0.12 * rng.randn(1, 128, 128)), 'post1_bias': f32(0.1 * rng.randn(128)),
         'post2': f32(0.12 * rng.randn(1, 128, 1)), 'post2_bias': f32(0.1 * rng.randn(1)),
         'g': f32(rng.randn(N, T, 64)), 'dy': f32(0.5 + rng.randn(N, T))}       # (a mean: sum dy = d post2_bias is no cancellation)
    return c


LAYER_RESIDUAL = ('x', 'P', 'filter', 'gate', 'dense', 'dense_bias')
LAYER_LAST = ('x', 'P', 'filter', 'gate', 'skip', 'skip_bias', 'post1', 'post1_bias', 'post2', 'post2_bias')


def layer_grads(c, last, dtype, g=None):
    """Autograd of sum(out * g) (residual form: out = x + o dense + dense_bias) or sum(y * dy) (last form: y = head(o)) for the
    variables named in LAYER_RESIDUAL / LAYER_LAST; float64 numpy."""
    names = LAYER_LAST if last else LAYER_RESIDUAL
    v = {k: torch.from_numpy(c[k]).to(dtype).requires_grad_(True) for k in names}
    d, hop = c['d'], c['hop']
    x = v['x']
    fg = TC.causal_conv_torch(x, torch.cat([v['filter'], v['gate']], dim=2), d)
    idx = (torch.arange(T) + hop // 2) // hop
    fg = fg + v['P'].reshape(N, c['frames'], 128)[:, idx, :]
    o = torch.tanh(fg[..., :64]) * torch.sigmoid(fg[..., 64:])
    if last:
        h1 = torch.relu(o @ v['skip'][0] + v['skip_bias'])
        y = torch.relu(h1 @ v['post1'][0] + v['post1_bias']) @ v['post2'][0] + v['post2_bias']
        loss = (y[..., 0] * torch.from_numpy(c['dy']).to(dtype)).sum()
    else:
        out = x + o @ v['dense'][0] + v['dense_bias']
        loss = (out * torch.from_numpy(c['g'] if g is None else g).to(dtype)).sum()
    loss.backward()
    return {k: t.grad.double().numpy() for k, t in v.items()}
