"""The yardstick of the transposed-conv training tests: the student with the reference's second conditioning (models.py:109-124: three
stride-4/4/5 transposed convolutions + ReLU, then the crop) restated on top of oracle.torch_cpu._wavenet with the einsum conditioning of
oracle/torch_cpu.py:81-88, its gradients by autograd in float64 / float32, the Adam / EMA trajectory, and one gated layer (+ head) with a
per-sample condition for the kernel-level test.  Nothing here runs on a GPU or calls the package's training code.

ReLU.  A conditioning pre-activation that is closer to zero than float32 can tell (rounding at K = 80 is about 1e-7 of the magnitude)
may fall on either side of the ReLU in a float32 evaluation, and one flipped ReLU would then decide a comparison of gradients.  The
problems here are therefore drawn from seeds at which EVERY pre-activation of the three stages has |v| >= RELU_MARGIN in float64; the
restatement asserts it."""
import functools

import numpy as np
import torch

from oracle import iaf_oracle as O
from oracle import torch_cpu as TC
from tests import train_oracle as TO
from tests import train_power_oracle as PO

N, T, HOP = 2, 240, 80              # 480 rows = 15 units of 32, the utterance boundary in the middle of unit 7
STRIDES = (4, 4, 5)
RELU_MARGIN = 1e-6
SEED = 4                            # of the weights; chosen on the CPU so that the ReLU condition holds (relu_margin())
WIN = 160                           # the power-loss case: win_length <= T, 2 frames of 160 samples at hop 80, nfft 256


def small_cfg(**kw):
    return O.ModelConfig(dilations=[[1, 2, 32, 64], [4, 48, 256, 3]], n_iaf=2, hop_length=HOP, cond_upsample_method='transposed_conv', **kw)


@functools.lru_cache(maxsize=None)
def problem():
    """(cfg, weights, mel, z, wav) of the small model: 2 x 240 samples, hop 80, transposed-conv conditioning."""
    cfg = small_cfg()
    assert tuple(cfg.strides) == STRIDES
    w = O.init_weights(cfg, seed=SEED)
    mel, z = O.synthetic_inputs(N, T, cfg)
    wav = (0.3 * np.random.RandomState(5).randn(N, T, 1)).astype(np.float32)
    return cfg, w, mel, z, wav


def condition(W, melt, cfg, pre=None):
    """models.py:109-124 as oracle/torch_cpu.py:81-88 has it; `pre`, a list, receives every stage's pre-activations."""
    hop, cond = cfg.hop_length, melt
    for i, s in enumerate(cfg.strides):
        w = W['iaf_vocoder/cond/transposed_conv_%d_weights' % i][0]             # [s, Cout, Cin]
        n, t, _ = cond.shape
        o = torch.einsum('ntc,joc->ntjo', cond, w).reshape(n, t * s, w.shape[1])
        if pre is not None:
            pre.append(o.detach())
        cond = torch.relu(o)
    return cond[:, hop // 2: -(hop // 2), :]


def forward(W, melt, x, cfg, pre=None):
    cond = condition(W, melt, cfg, pre)
    for i in range(cfg.n_iaf):
        outs = [TC._wavenet(W, 'iaf_vocoder/iaf%d/%s' % (i, net), x, cond, cfg.dilations[i], cfg.use_biases, cfg.use_skip_connection)
                for net in O.net_names(cfg)]
        x = x * outs[0] + outs[1]
    return x


def relu_margin(weights, mel, cfg):
    """The smallest |pre-activation| of the three conditioning stages in float64."""
    with torch.no_grad():
        W = {k: torch.from_numpy(np.ascontiguousarray(v)).double() for k, v in weights.items() if '/cond/' in k}
        pre = []
        condition(W, torch.from_numpy(mel).double(), cfg, pre)
    return min(float(p.abs().min()) for p in pre)


def loss_and_grads(weights, mel, z, wav, cfg, dtype, power=None, check_relu=True):
    """(terms, pred [N, T, 1] float64 numpy, {name: float64 numpy gradient, or None for a variable the loss does not depend on}) of
    total = L1 (+ w * power for power = (w, win)); terms = {'likelihood', 'power', 'total'}."""
    W = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype).requires_grad_(True) for k, v in weights.items()}
    pre = []
    pred = forward(W, torch.from_numpy(mel).to(dtype), torch.from_numpy(z).to(dtype), cfg, pre)
    if dtype == torch.float64 and check_relu:
        assert min(float(p.abs().min()) for p in pre) >= RELU_MARGIN, 'a conditioning pre-activation sits on the ReLU: draw another seed'
    y = torch.from_numpy(wav).to(dtype)
    l1 = (pred - y).abs().mean()
    pw = PO.power_loss_torch(pred, y, power[1], cfg.hop_length, dtype) if power else torch.zeros((), dtype=dtype)
    total = l1 + power[0] * pw if power else l1
    total.backward()
    terms = {'likelihood': float(l1.detach()), 'power': float(pw.detach()), 'total': float(total.detach())}
    return terms, pred.detach().double().numpy(), {k: (v.grad.double().numpy() if v.grad is not None else None) for k, v in W.items()}


@functools.lru_cache(maxsize=None)
def balanced_weight():
    """The w at which the power term's gradient for pred has the L1's maximum, 1 / (N T), in the float64 reference."""
    cfg, _, _, _, wav = problem()
    g = PO.power_grad_numpy(reference()['pred'], wav, WIN, cfg.hop_length)
    return float(1.0 / (N * T) / np.abs(g).max())


@functools.lru_cache(maxsize=None)
def reference(power=False):
    """{'terms', 'loss', 'pred', 'g64', 'E32', 'w'}: float64 and float32 autograd of the small problem (power: under L1 + balanced_weight()
    * power at WIN); E32 = max over the variables of max|g32 - g64| / max|g64|."""
    cfg, w, mel, z, wav = problem()
    pw = (balanced_weight(), WIN) if power else None
    t64, p64, g64 = loss_and_grads(w, mel, z, wav, cfg, torch.float64, pw)
    _, _, g32 = loss_and_grads(w, mel, z, wav, cfg, torch.float32, pw)
    return {'terms': t64, 'loss': t64['total'], 'pred': p64, 'g64': g64, 'w': pw[0] if pw else None,
            'E32': max(TO.rel_err(g32[k], v) for k, v in g64.items() if v is not None)}


@functools.lru_cache(maxsize=None)
def trajectory(steps=5, single=False):
    """(losses before each of `steps` updates, the shadows after the last) of training on the fixed batch with the restatement and
    tests.train_oracle.adam_ema_numpy: float64 throughout, or -- `single` -- with everything a float32 implementation rounds.  The ReLU
    condition is asserted for the first step, the problem as drawn; later steps move every pre-activation by about the learning rate, and
    what a ReLU that flips there costs a float32 implementation is part of the float32 restatement's own distance, the bar's unit."""
    cfg, w, mel, z, wav = problem()
    dt, tdt = (np.float32, torch.float32) if single else (np.float64, torch.float64)
    W = {k: a.astype(dt) for k, a in w.items()}
    m = {k: np.zeros_like(a) for k, a in W.items()}
    v = {k: np.zeros_like(a) for k, a in W.items()}
    shadow = {k: a.copy() for k, a in W.items()}
    losses = []
    for t in range(1, steps + 1):
        terms, _, g = loss_and_grads(W, mel, z, wav, cfg, tdt, check_relu=t == 1)
        losses.append(terms['total'])
        TO.adam_ema_numpy(W, m, v, shadow, {k: (a.astype(dt) if a is not None else None) for k, a in g.items()}, t)
    return losses, shadow


# ---- one layer ----------------------------------------------------------------------------------------------------------------------
LT = 200                            # the layer tests: 2 x 200 rows = 12.5 units, the utterance boundary inside unit 6
LAYER_RESIDUAL = ('x', 'cond', 'filter', 'gate', 'gc_filter', 'gc_gate', 'filter_bias', 'gate_bias', 'dense', 'dense_bias')
LAYER_LAST = ('x', 'cond', 'filter', 'gate', 'gc_filter', 'gc_gate', 'filter_bias', 'gate_bias', 'skip', 'skip_bias', 'post1', 'post1_bias',
              'post2', 'post2_bias')


@functools.lru_cache(maxsize=None)
def layer_case(d, C, seed=23):
    """Inputs of one gated layer with a per-sample condition on 2 x 200 rows: x [N, T, 64], cond [N, T, C], the weights in TF layouts, g
    [N, T, 64] for the residual form and dy [N, T] for the last-layer + head form.  (No ReLU lies between cond and the outputs.)"""
    rng = np.random.RandomState(seed + d + 1000 * C)
    f32 = lambda a: a.astype(np.float32)
    return {'d': d, 'C': C,
            'x': f32(rng.randn(N, LT, 64)), 'cond': f32(np.abs(rng.randn(N, LT, C))),
            'filter': f32(0.15 * rng.randn(2, 64, 64)), 'gate': f32(0.15 * rng.randn(2, 64, 64)),
            'gc_filter': f32(0.1 * rng.randn(1, C, 64)), 'gc_gate': f32(0.1 * rng.randn(1, C, 64)),
            'filter_bias': f32(0.1 * rng.randn(64)), 'gate_bias': f32(0.1 * rng.randn(64)),
            'dense': f32(0.15 * rng.randn(1, 64, 64)), 'dense_bias': f32(0.1 * rng.randn(64)),
            'skip': f32(0.15 * rng.randn(1, 64, 128)), 'skip_bias': f32(0.1 * rng.randn(128)),
            'post1': f32(0.12 * rng.randn(1, 128, 128)), 'post1_bias': f32(0.1 * rng.randn(128)),
            'post2': f32(0.12 * rng.randn(1, 128, 1)), 'post2_bias': f32(0.1 * rng.randn(1)),
            'g': f32(rng.randn(N, LT, 64)), 'dy': f32(0.5 + rng.randn(N, LT))}


def layer_forward(v, d, last):
    """FG = conv([filter | gate]) + cond [gc_filter | gc_gate] + [filter_bias | gate_bias], the gate, then the residual form's output
    x + o dense + dense_bias or the last form's head; `v` a dict of torch tensors."""
    fg = TC.causal_conv_torch(v['x'], torch.cat([v['filter'], v['gate']], dim=2), d)
    fg = fg + v['cond'] @ torch.cat([v['gc_filter'][0], v['gc_gate'][0]], dim=1) + torch.cat([v['filter_bias'], v['gate_bias']])
    o = torch.tanh(fg[..., :64]) * torch.sigmoid(fg[..., 64:])
    if last:
        h1 = torch.relu(o @ v['skip'][0] + v['skip_bias'])
        return o, (torch.relu(h1 @ v['post1'][0] + v['post1_bias']) @ v['post2'][0] + v['post2_bias'])[..., 0]
    return o, v['x'] + o @ v['dense'][0] + v['dense_bias']


def layer_grads(c, last, dtype):
    """({name: float64 numpy gradient} of sum(out * g) (residual) or sum(y * dy) (last) for LAYER_RESIDUAL / LAYER_LAST, the layer's
    forward output in float64 numpy: x_out, or o in the last form)."""
    names = LAYER_LAST if last else LAYER_RESIDUAL
    v = {k: torch.from_numpy(c[k]).to(dtype).requires_grad_(True) for k in names}
    o, out = layer_forward(v, c['d'], last)
    (out * torch.from_numpy(c['dy'] if last else c['g']).to(dtype)).sum().backward()
    return {k: t.grad.double().numpy() for k, t in v.items()}, (o if last else out).detach().double().numpy()


@functools.lru_cache(maxsize=None)
def layer_reference(d, C, last):
    """(case, g64, forward output in float64, E32 of float32 autograd on the same layer)."""
    c = layer_case(d, C)
    g64, out = layer_grads(c, last, torch.float64)
    g32, _ = layer_grads(c, last, torch.float32)
    return c, g64, out, max(TO.rel_err(g32[k], g64[k]) for k in g64 if np.abs(g64[k]).max() > 0)
