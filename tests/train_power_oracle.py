"""The yardstick of the power-loss training tests: the reference's power_loss (models.py:95-99, tf.contrib.signal.stft at its defaults)
restated in differentiable torch ops on the CPU, the gradient of include/pwv_hip_train_loss.h written out in numpy float64, and the
student's total loss L1 + w * power on top of tests.train_oracle.forward.  Nothing here runs on a GPU or calls the package's training
code."""
import functools

import numpy as np
import torch

from tests import train_oracle as TO


def fft_length(win):
    n = 1
    while n < win:
        n *= 2
    return n


def frame_count(T, win, hop):
    return 0 if T < win else 1 + (T - win) // hop


# (T, win, hop) of the kernel tests: nfft 64 > win with 1 to 3 frames per sample; a hop that does not
# divide win; hop > win: gaps that no frame covers, and a tail; win a power of two; the default signal settings (nfft 512, 5-fold overlap);
# and, since (208 - 48) % 20 = 0, one more with a hop below win AND a tail of two samples behind the last frame
SHAPES = [(208, 48, 16), (208, 48, 20), (100, 16, 24), (208, 64, 16), (1200, 400, 80), (210, 48, 20)]


def case(T, n=2, seed=0):
    """(pred, y) float32 [n, T]: y = 0.3 randn, pred = y + 0.2 randn, from the first of the seeds 1000 seed + T, + 1, ... whose draw has
    |pred - y| > 1e-4 everywhere, so that the sign is not in question (a draw of 2400 samples has one closer than that more often than not)."""
    for s in range(1000 * seed + T, 1000 * seed + T + 50):
        rng = np.random.RandomState(s)
        y = (0.3 * rng.randn(n, T)).astype(np.float32)
        pred = (y + (0.2 * rng.randn(n, T)).astype(np.float32)).astype(np.float32)
        if np.abs(pred.astype(np.float64) - y).min() > 1e-4:
            break
    assert np.abs(pred.astype(np.float64) - y).min() > 1e-4
    return pred, y


def power_loss_torch(pred, y, win, hop, dtype):
    """mean over utterances, frames and rfft bins of (|STFT pred|^2 - |STFT y|^2)^2; pred, y: torch [N, T] (or [N, T, 1]).  Periodic Hann
    window of `win`, frame f = samples f hop .. f hop + win - 1, zero-padded behind to the next power of two, no centring, no end padding."""
    pred, y = (t.to(dtype).reshape(t.shape[0], -1) for t in (pred, y))
    window = 0.5 - 0.5 * torch.cos(2.0 * np.pi * torch.arange(win, dtype=torch.float64) / win)
    window = window.to(dtype)
    nfft = fft_length(win)

    def power(x):
        spec = torch.fft.rfft(x.unfold(1, win, hop) * window, n=nfft, dim=2)
        return spec.real ** 2 + spec.imag ** 2

    d = power(pred) - power(y)
    assert d.shape[1:] == (frame_count(pred.shape[1], win, hop), nfft // 2 + 1)
    return (d * d).mean()


def power_grad_numpy(pred, y, win, hop):
    """d mean D^2 / d pred [N, T] by the formula of include/pwv_hip_train_loss.h, float64, direct sums (no FFT):
        4 / (N F B) sum_{f : 0 <= t - f hop < win} w_j sum_b D_b (Ar_b cos(2 pi b j / nfft) + Ai_b sin(2 pi b j / nfft)),   j = t - f hop"""
    pred, y = (np.asarray(a, dtype=np.float64).reshape(np.shape(a)[0], -1) for a in (pred, y))
    N, T = pred.shape
    nfft, F = fft_length(win), frame_count(T, win, hop)
    B = nfft // 2 + 1
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win) / win)
    ang = 2.0 * np.pi * np.outer(np.arange(B), np.arange(win)) / nfft
    C, S = np.cos(ang), np.sin(ang)                                     # [B, win]
    g = np.zeros((N, T))
    for i in range(N):
        for f in range(F):
            a, b = w * pred[i, f * hop:f * hop + win], w * y[i, f * hop:f * hop + win]
            Ar, Ai, Br, Bi = C @ a, S @ a, C @ b, S @ b
            D = (Ar * Ar + Ai * Ai) - (Br * Br + Bi * Bi)
            g[i, f * hop:f * hop + win] += w * ((D * Ar) @ C + (D * Ai) @ S)
    return g * (4.0 / (N * F * B))


def power_grad_autograd(pred, y, win, hop, dtype):
    """The same gradient by autograd of power_loss_torch in `dtype`; float64 numpy [N, T]."""
    p = torch.from_numpy(np.ascontiguousarray(pred)).to(dtype).reshape(np.shape(pred)[0], -1).requires_grad_(True)
    power_loss_torch(p, torch.from_numpy(np.ascontiguousarray(y)), win, hop, dtype).backward()
    return p.grad.double().numpy()


def total_loss_and_grads(weights, mel, z, wav, cfg, w, win, dtype):
    """({'likelihood', 'power', 'total'}, pred [N, T, 1] float64 numpy, {name: float64 numpy gradient of total = L1 + w * power, or None}) of
    the student of tests.train_oracle at hop = cfg.hop_length."""
    W = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype).requires_grad_(True) for k, v in weights.items()}
    pred = TO.forward(W, torch.from_numpy(mel).to(dtype), torch.from_numpy(z).to(dtype), cfg)
    y = torch.from_numpy(wav).to(dtype)
    l1 = (pred - y).abs().mean()
    power = power_loss_torch(pred, y, win, cfg.hop_length, dtype)
    total = l1 + w * power
    total.backward()
    terms = {'likelihood': float(l1.detach()), 'power': float(power.detach()), 'total': float(total.detach())}
    return terms, pred.detach().double().numpy(), {k: (v.grad.double().numpy() if v.grad is not None else None) for k, v in W.items()}


WIN = 48            # the whole-model tests: 11 frames of 48 samples at hop 16 in 208 samples, nfft 64


@functools.lru_cache(maxsize=None)
def balanced_weight():
    """The w at which the two terms' gradients for pred have equal maxima in the float64 reference: max |d L1 / d pred| = 1 / (N T)."""
    cfg, _, _, _, wav = TO.problem()
    g = power_grad_numpy(TO.reference()['pred'], wav, WIN, cfg.hop_length)
    return float(1.0 / (TO.N * TO.T) / np.abs(g).max())


@functools.lru_cache(maxsize=None)
def reference(w=None):
    """{'terms', 'pred', 'g64', 'g32', 'E32'} of the small problem under L1 + w * power (w None: balanced_weight())."""
    cfg, weights, mel, z, wav = TO.problem()
    w = balanced_weight() if w is None else w
    t64, p64, g64 = total_loss_and_grads(weights, mel, z, wav, cfg, w, WIN, torch.float64)
    _, _, g32 = total_loss_and_grads(weights, mel, z, wav, cfg, w, WIN, torch.float32)
    return {'terms': t64, 'pred': p64, 'g64': g64, 'g32': g32, 'w': w,
            'E32': max(TO.rel_err(g32[k], v) for k, v in g64.items() if v is not None)}


@functools.lru_cache(maxsize=None)
def trajectory(steps=5):
    """[{'likelihood', 'power', 'total'} before each of `steps` updates + after the last] of training on the fixed batch under
    L1 + balanced_weight() * power with the float64 restatement (autograd + tests.train_oracle.adam_ema_numpy)."""
    cfg, weights, mel, z, wav = TO.problem()
    w = balanced_weight()
    W = {k: a.astype(np.float64) for k, a in weights.items()}
    m = {k: np.zeros_like(a) for k, a in W.items()}
    v = {k: np.zeros_like(a) for k, a in W.items()}
    shadow = {k: a.copy() for k, a in W.items()}
    out = []
    for t in range(1, steps + 2):
        terms, _, g = total_loss_and_grads(W, mel, z, wav, cfg, w, WIN, torch.float64)
        out.append(terms)
        if t <= steps:
            TO.adam_ema_numpy(W, m, v, shadow, g, t)
    return out
