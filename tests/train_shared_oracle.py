"""The yardstick of the tests of training the shared-net architecture (model.shared_nets True: one WaveNet with two outputs per flow,
out = x y[..., 0] + y[..., 1]): the small model of tests/train_oracle.py with the switch set (also with skip connections, also with
transposed-conv conditioning), a forward of its own over oracle.torch_cpu._wavenet -- tests.train_oracle.forward hard-codes two nets --,
its problems and float64 / float32 autograd references for uniform and packed batches, the Adam / EMA trajectory, and a
float64-autograd restatement of the two-output head in both input modes for the kernel-level tests.  Nothing here runs on a GPU or
calls the package's training code."""
import functools

import numpy as np
import torch

from oracle import iaf_oracle as O
from oracle import torch_cpu as TC
from tests import train_cond_oracle as CO
from tests import train_oracle as TO
from tests import train_varlen_oracle as VO

DILATIONS = [[1, 2, 32, 64], [4, 48, 256, 3]]          # tests.train_oracle.small_cfg's
WEIGHT_SEED = 3                                        # tests.train_oracle's; every margin below holds with it (asserted)
# variables of the small shared model: 2 nets x (causal filter + 4 layers x 10 + 4 head) + cond/dense
TOTAL = 2 * (1 + 4 * 10 + 4) + 1
DEAD = 2 * (3 * 2 + 2)                                 # skip, skip_bias of every layer but the last; dense, dense_bias of the last
DEAD_SKIP = 2 * 2                                      # with skip connections: the last layer's dense, dense_bias alone


def small_cfg(hop=TO.HOP, skip=False, tran=False):
    kw = dict(cond_upsample_method='transposed_conv') if tran else {}
    cfg = O.ModelConfig(dilations=DILATIONS, n_iaf=2, hop_length=hop, shared_nets=True, use_skip_connection=bool(skip), **kw)
    assert cfg.dilations == TO.small_cfg(hop).dilations
    return cfg


@functools.lru_cache(maxsize=None)
def weights(skip=False, tran=False):
    return O.init_weights(small_cfg(80 if tran else TO.HOP, skip, tran), seed=WEIGHT_SEED)


def forward(W, melt, x, cfg):
    """The student with one shared net per flow: x <- x y[..., 0:1] + y[..., 1:2], y = _wavenet(...) [N, T, 2]."""
    hop = cfg.hop_length
    if cfg.cond_upsample_method == 'transposed_conv':
        cond = CO.condition(W, melt, cfg)
    else:
        c = torch.relu(melt @ W['iaf_vocoder/cond/dense'][0])
        cond = c.repeat_interleave(hop, dim=1)[:, hop // 2: -(hop // 2), :]
    for i in range(cfg.n_iaf):
        y = TC._wavenet(W, 'iaf_vocoder/iaf%d/shared' % i, x, cond, cfg.dilations[i], cfg.use_biases, cfg.use_skip_connection)
        assert y.shape[-1] == 2
        x = x * y[..., 0:1] + y[..., 1:2]
    return x


def _tensors(weights, dtype, grad=False):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype).requires_grad_(grad) for k, v in weights.items()}


def pred64(weights, mel, z, cfg):
    with torch.no_grad():
        return forward(_tensors(weights, torch.float64), torch.from_numpy(mel).double(), torch.from_numpy(z).double(), cfg).numpy()


def _grads(W):
    return {k: (v.grad.double().numpy() if v.grad is not None else None) for k, v in W.items()}


def loss_and_grads(weights, mel, z, wav, cfg, dtype):
    """(loss, pred [N, T, 1] float64 numpy, {name: float64 numpy gradient, or None}) of the L1 mean |pred - wav|."""
    W = _tensors(weights, dtype, True)
    pred = forward(W, torch.from_numpy(mel).to(dtype), torch.from_numpy(z).to(dtype), cfg)
    loss = (pred - torch.from_numpy(wav).to(dtype)).abs().mean()
    loss.backward()
    return float(loss.detach()), pred.detach().double().numpy(), _grads(W)


def loss_only(weights, mel, z, wav, cfg):
    return float(np.abs(pred64({k: np.asarray(v, dtype=np.float64) for k, v in weights.items()}, mel, z, cfg) - wav.astype(np.float64)).mean())


def relu_margin(w, mel, cfg):
    return CO.relu_margin(w, mel, cfg) if cfg.cond_upsample_method == 'transposed_conv' else TO.relu_margin(w, mel)


# ---- the whole model, uniform batches --------------------------------------------------------------------------------------------------
def problem(N=TO.N, T=TO.T, hop=TO.HOP, skip=False, tran=False):
    """(cfg, weights, mel, z, wav) of the small shared model on N x T samples at hop length `hop`; asserts the two input margins of
    tests.train_oracle (the wav seed is the first from TO.WAV_SEED upward that keeps the sign margin: tests.train_oracle.draw_wav)."""
    return _problem(int(N), int(T), int(hop), bool(skip), bool(tran))


@functools.lru_cache(maxsize=None)
def _problem(N, T, hop, skip, tran):
    cfg, w = small_cfg(hop, skip, tran), weights(skip, tran)
    mel, z = O.synthetic_inputs(N, T, cfg)
    assert relu_margin(w, mel, cfg) >= TO.RELU_MARGIN, 'a conditioning pre-activation sits on the ReLU: draw another seed'
    p64 = pred64(w, mel, z, cfg)
    wav, = TO.draw_wav([p64], TO.WAV_SEED, [(N, T, 1)])
    assert float(np.abs(p64 - wav).min()) >= TO.SIGN_MARGIN
    return cfg, w, mel, z, wav


def reference(N=TO.N, T=TO.T, hop=TO.HOP, skip=False, tran=False):
    """{'loss', 'pred', 'g64', 'g32', 'E32'} as tests.train_oracle.reference, of the shared model."""
    return _reference(int(N), int(T), int(hop), bool(skip), bool(tran))


@functools.lru_cache(maxsize=None)
def _reference(N, T, hop, skip, tran):
    cfg, w, mel, z, wav = problem(N, T, hop, skip, tran)
    l64, p64, g64 = loss_and_grads(w, mel, z, wav, cfg, torch.float64)
    _, _, g32 = loss_and_grads(w, mel, z, wav, cfg, torch.float32)
    return {'loss': l64, 'pred': p64, 'g64': g64, 'g32': g32, 'E32': max(TO.rel_err(g32[k], v) for k, v in g64.items() if v is not None)}


# ---- packed batches ---------------------------------------------------------------------------------------------------------------------
def packed_problem(lengths=tuple(VO.LENGTHS), hop=VO.HOP, skip=False):
    """(cfg, weights, mels, zs, wavs) as tests.train_varlen_oracle.problem (the same seeds per utterance), of the shared model."""
    return _packed_problem(tuple(int(T) for T in lengths), int(hop), bool(skip))


@functools.lru_cache(maxsize=None)
def _packed_problem(lengths, hop, skip):
    cfg, w = small_cfg(hop, skip), weights(skip)
    mels, zs = [], []
    for i, T in enumerate(lengths):
        mel, z = O.synthetic_inputs(1, T, cfg, mel_seed=20 + i, z_seed=40 + i)
        mels.append(mel)
        zs.append(z)
    assert min(TO.relu_margin(w, mel) for mel in mels) >= TO.RELU_MARGIN, 'a conditioning pre-activation sits on the ReLU: draw another seed'
    preds = [pred64(w, mel, z, cfg) for mel, z in zip(mels, zs)]
    wavs = TO.draw_wav(preds, VO.WAV_SEED, [(1, T, 1) for T in lengths])
    assert min(float(np.abs(p - y).min()) for p, y in zip(preds, wavs)) >= TO.SIGN_MARGIN
    return cfg, w, mels, zs, wavs


def packed_loss_and_grads(weights, mels, zs, wavs, cfg, dtype):
    """(loss = sum_i sum_t |pred_i - wav_i| / sum_i T_i, [pred_i [T_i] float64 numpy], gradients), every utterance run on its own."""
    W = _tensors(weights, dtype, True)
    preds = [forward(W, torch.from_numpy(m).to(dtype), torch.from_numpy(z).to(dtype), cfg) for m, z in zip(mels, zs)]
    rows = sum(p.shape[1] for p in preds)
    loss = sum((p - torch.from_numpy(y).to(dtype)).abs().sum() for p, y in zip(preds, wavs)) / rows
    loss.backward()
    return float(loss.detach()), [p.detach().double().numpy().reshape(-1) for p in preds], _grads(W)


def packed_reference(lengths=tuple(VO.LENGTHS), hop=VO.HOP, skip=False):
    """{'loss', 'preds', 'g64', 'g32', 'E32'} of the packed problem (the L1 alone)."""
    return _packed_reference(tuple(int(T) for T in lengths), int(hop), bool(skip))


@functools.lru_cache(maxsize=None)
def _packed_reference(lengths, hop, skip):
    cfg, w, mels, zs, wavs = packed_problem(lengths, hop, skip)
    l64, p64, g64 = packed_loss_and_grads(w, mels, zs, wavs, cfg, torch.float64)
    _, _, g32 = packed_loss_and_grads(w, mels, zs, wavs, cfg, torch.float32)
    return {'loss': l64, 'preds': p64, 'g64': g64, 'g32': g32, 'E32': max(TO.rel_err(g32[k], v) for k, v in g64.items() if v is not None)}


# ---- the optimiser's trajectory ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def trajectory(steps=5, single=False):
    """tests.train_oracle.trajectory on the shared model's fixed batch: (losses before each update + the loss after the last, shadows)."""
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
        TO.adam_ema_numpy(W, m, v, shadow, {k: (a.astype(dt) if a is not None else None) for k, a in g.items()}, t)
        assert all(a.dtype == dt for a in list(W.values()) + list(shadow.values()))
    losses.append(loss_only(W, mel, z, wav, cfg))
    return losses, shadow


# ---- the two-output head -----------------------------------------------------------------------------------------------------------------
GATED, SKIPSUM = 0, 1
HEAD_WEIGHTS = ('skip', 'skip_bias', 'post1', 'post1_bias', 'post2', 'post2_bias')
HEAD_BIASES = ('skip_bias', 'post1_bias', 'post2_bias')


def head_case(N, T, seed=31):
    """Inputs of the head on N x T rows: o [rows, 64] (GATED), S [rows, 128] (SKIPSUM), the weights in TF layouts -- post2 [1, 128, 2] with
    two different columns, post2_bias [2] --, d_out [rows] (a mean: sum d_out = d post2_bias[1] is no cancellation) and d_mul [rows],
    random and not 1."""
    rng = np.random.RandomState(seed + 13 * N + T)
    rows = N * T
    f32 = lambda a: a.astype(np.float32)
    c = {'N': N, 'T': T, 'rows': rows, 'o': f32(np.tanh(rng.randn(rows, 64))), 'S': f32(rng.randn(rows, 128)),
         'skip': f32(0.15 * rng.randn(1, 64, 128)), 'skip_bias': f32(0.1 * rng.randn(128)),
         'post1': f32(0.12 * rng.randn(1, 128, 128)), 'post1_bias': f32(0.1 * rng.randn(128)),
         'post2': f32(0.12 * rng.randn(1, 128, 2)), 'post2_bias': f32(0.1 * rng.randn(2)),
         'd_out': f32(0.5 + rng.randn(rows)), 'd_mul': f32(0.7 + rng.randn(rows))}
    assert np.abs(c['post2'][0, :, 0] - c['post2'][0, :, 1]).min() > 0 and np.abs(c['d_mul'] - 1).min() > 0
    return c


def shared_head(c, mode, dtype, biased=True):
    """The two-output head by autograd in `dtype` under sum(y_0 dy_0) + sum(y_1 dy_1), dy_0 = d_out d_mul, dy_1 = d_out
    (include/pwv_hip_train_shared.h): y0, y1 [rows]; post1, post2 and (biased) their biases; GATED: skip, skip_bias (biased) and d_o
    [rows, 64]; SKIPSUM: dS [rows, 128] and skip_bias = its column sums.  Without `biased` every bias reads as zeros.  float64 numpy."""
    names = [k for k in HEAD_WEIGHTS if (biased or k not in HEAD_BIASES) and (mode == GATED or not k.startswith('skip'))]
    v = {k: torch.from_numpy(c[k]).to(dtype).requires_grad_(True) for k in names}
    bias = lambda k: v[k] if k in v else 0
    if mode == GATED:
        x = torch.from_numpy(c['o']).to(dtype).requires_grad_(True)
        h1 = torch.relu(x @ v['skip'][0] + bias('skip_bias'))
    else:
        x = torch.from_numpy(c['S']).to(dtype).requires_grad_(True)
        h1 = torch.relu(x)
    y = torch.relu(h1 @ v['post1'][0] + bias('post1_bias')) @ v['post2'][0] + bias('post2_bias')
    d_out, d_mul = torch.from_numpy(c['d_out']).to(dtype), torch.from_numpy(c['d_mul']).to(dtype)
    ((y[:, 0] * (d_out * d_mul)).sum() + (y[:, 1] * d_out).sum()).backward()
    out = {k: t.grad.double().numpy() for k, t in v.items()}
    out.update(y0=y.detach().double().numpy()[:, 0], y1=y.detach().double().numpy()[:, 1])
    if mode == GATED:
        out['d_o'] = x.grad.double().numpy()
    else:
        out['dS'] = x.grad.double().numpy()
        out['skip_bias'] = out['dS'].sum(axis=0)
    return out
