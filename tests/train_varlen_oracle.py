"""The yardstick of the packed-training tests: the loss of a packed batch of utterances of different lengths restated on top of
tests.train_oracle.forward (each utterance run at N = 1: an utterance never sees another), its gradients by autograd in float64 /
float32, the packed power cost with the batch's scales on top of tests.train_power_oracle, one gated layer (+ head) on the packed
rows, and the Adam / EMA trajectory.  Nothing here runs on a GPU or calls the package's training code."""
import functools

import numpy as np
import torch

from oracle import iaf_oracle as O
from oracle import torch_cpu as TC
from tests import train_oracle as TO
from tests import train_power_oracle as PO

# 416 rows = 13 units, boundaries at rows 208, 224, 272: two in the middle of a unit (208 = 6.5 units, 272 = 8.5 units), one exactly on a
# unit edge (224 = 7 units); unit 6 holds the end of utterance 0 and all of utterance 1, an utterance of one hop -- shorter than every
# dilation but 1, 2, 3, 4 -- and three utterances are shorter than dilation 64, all than 256.  (At hop 16 every boundary is a multiple
# of 16, so a 32-row unit holds at most two utterances; DENSE below, at hop 8, puts four into one.)
LENGTHS = [208, 16, 48, 144]
DENSE = ([40, 8, 8, 24, 16], 8)         # (lengths, hop) of the kernel-level case: rows 32 .. 63 hold parts of utterances 0, 1, 2 and 3
HOP = 16
ROWS = sum(LENGTHS)
CU_ROWS = [0] + [int(v) for v in np.cumsum(LENGTHS)]
FRAMES = [1 + T // HOP for T in LENGTHS]
CU_FRAMES = [0] + [int(v) for v in np.cumsum(FRAMES)]


WAV_SEED = 60                           # utterance i draws its wav from seed WAV_SEED + k + i, k the first that keeps TO.SIGN_MARGIN


def problem(lengths=tuple(LENGTHS), hop=HOP):
    """(cfg, weights, mels, zs, wavs) of the small model on a packed batch: per utterance mel [1, 1 + T_i / hop, 80], z [1, T_i, 1] and wav
    [1, T_i, 1], each from seeds of its own.  Asserts tests.train_oracle's RELU_MARGIN and SIGN_MARGIN of the inputs."""
    return _problem(tuple(int(T) for T in lengths), int(hop))


@functools.lru_cache(maxsize=None)
def _problem(lengths, hop):
    cfg = TO.small_cfg(hop)
    w = TO.problem()[1]
    mels, zs = [], []
    for i, T in enumerate(lengths):
        mel, z = O.synthetic_inputs(1, T, cfg, mel_seed=20 + i, z_seed=40 + i)
        mels.append(mel)
        zs.append(z)
    assert min(TO.relu_margin(w, mel) for mel in mels) >= TO.RELU_MARGIN, 'a conditioning pre-activation sits on the ReLU: draw another seed'
    wavs = TO.draw_wav([TO.pred64(w, mel, z, cfg) for mel, z in zip(mels, zs)], WAV_SEED, [(1, T, 1) for T in lengths])
    return cfg, w, mels, zs, wavs


def _weights(weights, dtype):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype).requires_grad_(True) for k, v in weights.items()}


def _preds(W, mels, zs, cfg, dtype):
    return [TO.forward(W, torch.from_numpy(m).to(dtype), torch.from_numpy(z).to(dtype), cfg) for m, z in zip(mels, zs)]


def _grads(W):
    return {k: (v.grad.double().numpy() if v.grad is not None else None) for k, v in W.items()}


def power_sum_torch(pred, y, win, hop, dtype):
    """(sum over frames and bins of (|STFT pred|^2 - |STFT y|^2)^2, the number of terms) of ONE utterance [1, T, 1]: the restatement of
    tests.train_power_oracle (its mean times its count), nothing for an utterance shorter than win."""
    T = pred.shape[1]
    F = PO.frame_count(T, win, hop)
    if F == 0:
        return pred.sum() * 0, 0
    terms = F * (PO.fft_length(win) // 2 + 1)
    return PO.power_loss_torch(pred, y, win, hop, dtype) * terms, terms


def loss_and_grads(weights, mels, zs, wavs, cfg, dtype, w=None, win=None):
    """({'likelihood', 'power', 'total'}, [pred_i [T_i] float64 numpy], {name: float64 numpy gradient of total, or None}):
    likelihood = sum_i sum_t |pred_i - wav_i| / sum_i T_i; power (w not None) = sum_i power_sum_i / sum_i terms_i; total = likelihood
    + w * power."""
    W = _weights(weights, dtype)
    preds = _preds(W, mels, zs, cfg, dtype)
    ys = [torch.from_numpy(y).to(dtype) for y in wavs]
    rows = sum(p.shape[1] for p in preds)
    l1 = sum((p - y).abs().sum() for p, y in zip(preds, ys)) / rows
    total, power = l1, None
    if w is not None:
        parts = [power_sum_torch(p, y, win, cfg.hop_length, dtype) for p, y in zip(preds, ys)]
        power = sum(s for s, _ in parts) / sum(n for _, n in parts)
        total = l1 + w * power
    total.backward()
    terms = {'likelihood': float(l1.detach()), 'power': float(power.detach()) if power is not None else 0.0, 'total': float(total.detach())}
    return terms, [p.detach().double().numpy().reshape(-1) for p in preds], _grads(W)


def reference(w=None, win=None, lengths=tuple(LENGTHS), hop=HOP):
    """{'terms', 'preds', 'g64', 'g32', 'E32'}: float64 and float32 autograd of the packed problem (L1, or L1 + w * power at `win`); E32 =
    max over the variables of max|g32 - g64| / max|g64|, as tests.train_oracle.reference computes it."""
    return _reference(w, win, tuple(int(T) for T in lengths), int(hop))


@functools.lru_cache(maxsize=None)
def _reference(w, win, lengths, hop):
    cfg, weights, mels, zs, wavs = problem(lengths, hop)
    t64, p64, g64 = loss_and_grads(weights, mels, zs, wavs, cfg, torch.float64, w, win)
    _, _, g32 = loss_and_grads(weights, mels, zs, wavs, cfg, torch.float32, w, win)
    return {'terms': t64, 'preds': p64, 'g64': g64, 'g32': g32,
            'E32': max(TO.rel_err(g32[k], v) for k, v in g64.items() if v is not None)}


@functools.lru_cache(maxsize=None)
def trajectory(steps=5, single=False):
    """(losses before each of `steps` updates + the loss after the last, the shadows after the last) of training on the fixed packed batch,
    as tests.train_oracle.trajectory: float64 throughout, or -- `single` -- variables, moments, shadows and autograd in float32."""
    cfg, weights, mels, zs, wavs = problem()
    dt, tdt = (np.float32, torch.float32) if single else (np.float64, torch.float64)
    W = {k: a.astype(dt) for k, a in weights.items()}
    m = {k: np.zeros_like(a) for k, a in W.items()}
    v = {k: np.zeros_like(a) for k, a in W.items()}
    shadow = {k: a.copy() for k, a in W.items()}
    losses = []
    for t in range(1, steps + 1):
        terms, _, g = loss_and_grads(W, mels, zs, wavs, cfg, tdt)
        losses.append(terms['total'])
        TO.adam_ema_numpy(W, m, v, shadow, {k: (a.astype(dt) if a is not None else None) for k, a in g.items()}, t)
        assert all(a.dtype == dt for a in list(W.values()) + list(shadow.values()))
    with torch.no_grad():
        Wt = {k: torch.from_numpy(np.ascontiguousarray(a)).double() for k, a in W.items()}
        preds = _preds(Wt, mels, zs, cfg, torch.float64)
        losses.append(float(sum((p - torch.from_numpy(y).double()).abs().sum() for p, y in zip(preds, wavs)) / ROWS))
    return losses, shadow


# ---- the loss head ---------------------------------------------------------------------------------------------------------------------
def head_case(seed=0):
    """(preds, ys): float32 [T_i] per utterance of LENGTHS, |pred - y| > 1e-4 everywhere (tests.train_power_oracle.case)."""
    pairs = [PO.case(T, 1, seed=seed + 3 * i) for i, T in enumerate(LENGTHS)]
    return [p[0] for p, _ in pairs], [y[0] for _, y in pairs]


def head_grad(preds, ys, win, hop, wl1, wp, dtype):
    """d (wl1 * L1 + wp * power) / d pred of the packed batch by autograd in `dtype`, the batch's scales; float64 numpy [rows]."""
    ps = [torch.from_numpy(p).to(dtype).reshape(1, -1, 1).requires_grad_(True) for p in preds]
    ts = [torch.from_numpy(y).to(dtype).reshape(1, -1, 1) for y in ys]
    total = wl1 * sum((p - t).abs().sum() for p, t in zip(ps, ts)) / sum(len(p) for p in preds)
    parts = [power_sum_torch(p, t, win, hop, dtype) for p, t in zip(ps, ts)]
    total = total + wp * sum(s for s, _ in parts) / sum(n for _, n in parts)
    total.backward()
    return np.concatenate([p.grad.double().numpy().reshape(-1) for p in ps])


# ---- one layer on the packed rows ------------------------------------------------------------------------------------------------------
def layer_case(d, seed=11, lengths=tuple(LENGTHS), hop=HOP):
    """tests.train_oracle.layer_case on a packed batch: x, g [rows, 64], dy [rows], P [sum frames, 128]; the weights of the uniform case."""
    c = {k: v for k, v in TO.layer_case(d, seed).items() if k not in ('N', 'T', 'offset')}
    rng = np.random.RandomState(seed + d + 1000)
    f32 = lambda a: a.astype(np.float32)
    rows, frames = sum(lengths), [1 + T // hop for T in lengths]
    c.update(lengths=list(lengths), hop=hop, frames=frames, cu_rows=[0] + [int(v) for v in np.cumsum(lengths)],
             cu_frames=[0] + [int(v) for v in np.cumsum(frames)],
             x=f32(rng.randn(rows, 64)), P=f32(0.5 * rng.randn(sum(frames), 128)), g=f32(rng.randn(rows, 64)), dy=f32(0.5 + rng.randn(rows)))
    return c


def layer_grads(c, last, dtype, g=None):
    """Autograd of sum(out * g) (residual form) or sum(y * dy) (last form + head) over the packed rows, every utterance convolved on its
    own; float64 numpy for the names of tests.train_oracle.LAYER_RESIDUAL / LAYER_LAST."""
    names = TO.LAYER_LAST if last else TO.LAYER_RESIDUAL
    v = {k: torch.from_numpy(c[k]).to(dtype).requires_grad_(True) for k in names}
    d = c['d']
    gg = torch.from_numpy(c['g'] if g is None else g).to(dtype)
    dy = torch.from_numpy(c['dy']).to(dtype)
    loss = 0
    hop = c['hop']
    for i, T in enumerate(c['lengths']):
        r0, f0 = c['cu_rows'][i], c['cu_frames'][i]
        x = v['x'][r0:r0 + T].unsqueeze(0)
        fg = TC.causal_conv_torch(x, torch.cat([v['filter'], v['gate']], dim=2), d)
        idx = (torch.arange(T) + hop // 2) // hop
        fg = fg + v['P'][f0:f0 + c['frames'][i]][idx].unsqueeze(0)
        o = torch.tanh(fg[..., :64]) * torch.sigmoid(fg[..., 64:])
        if last:
            h1 = torch.relu(o @ v['skip'][0] + v['skip_bias'])
            y = torch.relu(h1 @ v['post1'][0] + v['post1_bias']) @ v['post2'][0] + v['post2_bias']
            loss = loss + (y[0, :, 0] * dy[r0:r0 + T]).sum()
        else:
            out = x + o @ v['dense'][0] + v['dense_bias']
            loss = loss + (out[0] * gg[r0:r0 + T]).sum()
    loss.backward()
    return {k: t.grad.double().numpy() for k, t in v.items()}
