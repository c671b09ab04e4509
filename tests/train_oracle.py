"""The yardstick of the training tests: the L1 loss of the student restated on top of oracle.torch_cpu._wavenet (differentiable torch
ops on the CPU), its gradients by autograd in float64 / float32, TensorFlow's Adam and the reference's EMA in numpy float64, and one
gated layer (+ head) for the kernel-level test.  Nothing here runs on a GPU or calls the package's training code."""
import functools

import numpy as np
import torch

from oracle import iaf_oracle as O
from oracle import torch_cpu as TC

N, T, HOP = 2, 208, 16
LR, BETA1, BETA2, EPS, DECAY = 2e-4, 0.9, 0.999, 1e-8, 0.998
# Conditions on the INPUTS of a model-level problem (not bars): a conditioning pre-activation closer to zero than RELU_MARGIN may fall
# on either side of the ReLU in a float32 evaluation (tests/train_cond_oracle.py), and a prediction closer to its target than
# SIGN_MARGIN = 5 x tests.util.TOL_F32 may legitimately give the L1's sign(pred - wav) either value; one flipped ReLU or sign would
# then decide a comparison of gradients.
RELU_MARGIN = 1e-6
SIGN_MARGIN = 1e-4
WAV_SEED = 5                            # the first wav seed tried; problem() takes the first from here upward that keeps SIGN_MARGIN


def small_cfg(hop=HOP):
    return O.ModelConfig(dilations=[[1, 2, 32, 64], [4, 48, 256, 3]], n_iaf=2, hop_length=hop)


def relu_margin(weights, mel):
    """The smallest |pre-activation| of the conditioning dense + ReLU in float64."""
    return float(np.abs(np.asarray(mel, dtype=np.float64) @ weights['iaf_vocoder/cond/dense'][0].astype(np.float64)).min())


def pred64(weights, mel, z, cfg):
    """The model's output in float64, [N, T, 1] numpy."""
    with torch.no_grad():
        W = {k: torch.from_numpy(np.ascontiguousarray(v)).double() for k, v in weights.items()}
        return forward(W, torch.from_numpy(mel).double(), torch.from_numpy(z).double(), cfg).numpy()


def draw_wav(pred, first_seed, shapes):
    """[0.3 randn(shape) float32 from seed first_seed + k + i for the i-th shape] at the first k >= 0 for which every sample keeps
    |pred - wav| >= SIGN_MARGIN (`pred`: the float64 predictions, one array per shape); asserts the margin it returns with."""
    for k in range(64):
        wavs = [(0.3 * np.random.RandomState(first_seed + k + i).randn(*shape)).astype(np.float32) for i, shape in enumerate(shapes)]
        if min(float(np.abs(p - w).min()) for p, w in zip(pred, wavs)) >= SIGN_MARGIN:
            break
    assert min(float(np.abs(p - w).min()) for p, w in zip(pred, wavs)) >= SIGN_MARGIN, 'no wav seed keeps the predictions off their targets'
    return wavs


def problem(N=N, T=T, hop=HOP):
    """(cfg, weights, mel, z, wav) of the small model on N x T samples at hop length `hop` (the default: 2 x 208 samples, hop 16).  The
    weights do not depend on the shape.  Asserts RELU_MARGIN and SIGN_MARGIN of the inputs."""
    return _problem(int(N), int(T), int(hop))


@functools.lru_cache(maxsize=None)
def _problem(N, T, hop):
    cfg = small_cfg(hop)
    w = O.init_weights(cfg, seed=3)
    mel, z = O.synthetic_inputs(N, T, cfg)
    assert relu_margin(w, mel) >= RELU_MARGIN, 'a conditioning pre-activation sits on the ReLU: draw another seed'
    wav, = draw_wav([pred64(w, mel, z, cfg)], WAV_SEED, [(N, T, 1)])
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


def reference(N=N, T=T, hop=HOP):
    """{'loss', 'pred', 'g64', 'g32', 'E32'}: float64 and float32 autograd of problem(N, T, hop); E32 = max over the variables of
    max|g32 - g64| / max|g64|."""
    return _reference(int(N), int(T), int(hop))


@functools.lru_cache(maxsize=None)
def _reference(N, T, hop):
    cfg, w, mel, z, wav = problem(N, T, hop)
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


def layer_case(d, seed=11, hop=HOP, N=N, T=T, offset=None):
    """Inputs of one gated layer on N x T rows (the default: 2 x 208): x [N, T, 64], P [N * frames, 128] (natural column order; sample t
    reads frame (t + offset) // hop, offset = hop // 2 unless given), the weights in TF layouts, g [N, T, 64] for the residual form and
    dy [N, T] for the last-layer + head form."""
    rng = np.random.RandomState(seed + d)
    offset = hop // 2 if offset is None else offset
    frames = (T - 1 + offset) // hop + 1
    f32 = lambda a: a.astype(np.float32)
    c = {'d': d, 'hop': hop, 'frames': frames, 'N': N, 'T': T, 'offset': offset,
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
    d, hop, N, T = c['d'], c['hop'], c['N'], c['T']
    x = v['x']
    fg = TC.causal_conv_torch(x, torch.cat([v['filter'], v['gate']], dim=2), d)
    idx = (torch.arange(T) + c['offset']) // hop
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


def look_ahead(U, V, dn, cu_rows):
    """g[t] = U[t] + V[t + dn] while t + dn is inside the utterance: U, V [rows, C], utterance i = rows cu_rows[i] .. cu_rows[i + 1] - 1."""
    g = U.copy()
    for a, b in zip(cu_rows, cu_rows[1:]):
        if dn < b - a:
            g[a:b - dn] += V[a + dn:b]
    return g


# ---- the front: the causal layer and the affine --------------------------------------------------------------------------------------
FRONT_BASES = ('zero', 'affine', 'accumulate')


def front_case(lengths, dn, seed=21):
    """Inputs of the front backward on utterances of `lengths` samples, one after the other (a uniform batch: N times T): in, d_out,
    scale, d_in0 [rows], the causal filter cf [2, 1, 64], and U, V [rows, 64] of layer 0, whose dilation is dn."""
    rng = np.random.RandomState(seed + dn + 7 * len(lengths) + sum(lengths))
    rows = int(sum(lengths))
    f32 = lambda a: a.astype(np.float32)
    return {'lengths': [int(T) for T in lengths], 'cu_rows': [0] + [int(v) for v in np.cumsum(lengths)], 'dn': dn,
            'in': f32(rng.randn(rows)), 'cf': f32(0.3 * rng.randn(2, 1, 64)), 'U': f32(rng.randn(rows, 64)), 'V': f32(rng.randn(rows, 64)),
            'd_out': f32(rng.randn(rows)), 'scale': f32(0.5 + rng.rand(rows)), 'd_in0': f32(rng.randn(rows))}


def front_base(c, base, dtype=np.float64):
    """What d_in starts from: nothing, d_out * scale (the affine), or what d_in held (accumulate)."""
    if base == 'affine':
        return c['d_out'].astype(dtype) * c['scale'].astype(dtype)
    return c['d_in0'].astype(dtype) if base == 'accumulate' else np.zeros(len(c['in']), dtype=dtype)


def front_backward(c, base, dtype=np.float64):
    """The front backward restated in numpy of `dtype` (include/pwv_hip_train.h; x_0[t] = in[t - 1] cf[0] + in[t] cf[1], in[-1] = 0):
        g0[t]   = U[t] + V[t + dn] while t + dn < T
        d cf[0] = sum_{t > 0} in[t - 1] g0[t],   d cf[1] = sum_t in[t] g0[t]
        d_in[t] = base[t] + g0[t] . cf[1] + (t + 1 < T) g0[t + 1] . cf[0]
    per utterance; returns {'cf': [2, 1, 64], 'd_in': [rows]} in `dtype`."""
    cu = c['cu_rows']
    x, cf = c['in'].astype(dtype), c['cf'].astype(dtype)
    g0 = look_ahead(c['U'].astype(dtype), c['V'].astype(dtype), c['dn'], cu)
    d_in = front_base(c, base, dtype) + g0 @ cf[1, 0]
    nxt = g0 @ cf[0, 0]
    dcf = np.zeros((2, 1, 64), dtype=dtype)
    for a, b in zip(cu, cu[1:]):
        d_in[a:b - 1] += nxt[a + 1:b]
        dcf[0, 0] += x[a:b - 1] @ g0[a + 1:b]
        dcf[1, 0] += x[a:b] @ g0[a:b]
    assert d_in.dtype == dtype and dcf.dtype == dtype
    return {'cf': dcf, 'd_in': d_in}


def front_backward_autograd(c, base):
    """The same by float64 autograd of in -> x_0 (oracle.torch_cpu.causal_conv_torch at dilation 1, every utterance on its own) under
    sum(x_0 * g0); pins front_backward."""
    x = torch.from_numpy(c['in']).double().requires_grad_(True)
    cf = torch.from_numpy(c['cf']).double().requires_grad_(True)
    cu = c['cu_rows']
    g0 = torch.from_numpy(look_ahead(c['U'].astype(np.float64), c['V'].astype(np.float64), c['dn'], cu))
    loss = 0
    for a, b in zip(cu, cu[1:]):
        x0 = TC.causal_conv_torch(x[a:b].reshape(1, b - a, 1), cf, 1)
        loss = loss + (x0[0] * g0[a:b]).sum()
    loss.backward()
    return {'cf': cf.grad.numpy(), 'd_in': front_base(c, base) + x.grad.numpy()}
