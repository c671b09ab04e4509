"""Scoring generated audio on the device: the two quantities the reference measures about its output (models.py:90-99), as forward-only
metrics -- l1_loss(out, wav), logged as loss/likelihood, and power_loss(out, wav, win_length, hop_length), logged as loss/power.

    s = score(pred, gt)                     # [N, L, 1] or [N, L] each, CUDA float32 -> Scores
    s = score_varlen(preds, gts)            # lists of [len_i, 1], or what generate_varlen / push_varlen returned
    s.likelihood, s.power_loss, s.total()   # the batch numbers (the reference's reduce_mean over all elements)
    s.l1, s.power, s.frames                 # per utterance
    mel_l1(wav_to_mel_device(pred), mel)    # the L1 of two mels: the one metric that needs no ground-truth wav

The definitions (include/pwv_hip_score.h; DESIGN.md section 9, "Scoring on the device"), all in float64 on the float32 inputs: per utterance
abs_sum = sum |out - y| over its L samples, and power_sum = sum over frames and bins of (P_out - P_y)^2 with P = |rfft|^2 of
tf.contrib.signal.stft(frame_length=win, frame_step=hop) at its defaults -- periodic Hann window, frames zero-padded behind to the
smallest power of two >= win, no centring, pad_end=False: F = 0 frames for L < win, else 1 + (L - win) // hop.  `score_reference` restates
that in numpy.  TensorFlow is not a dependency and was not available to check the restatement against: it follows TF's documentation.

The calls only enqueue on the current stream (pwv_score_f32, csrc/pwv_score.hip); nothing synchronises until a Scores is read.  A row of
the table is the same bits whether its utterance is scored alone, in a uniform batch or in a packed one."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from .hparam import hparam as hp


def fft_length(win_length: int) -> int:
    """The smallest power of two >= win_length (tf.contrib.signal.stft's default fft_length)."""
    n = 1
    while n < win_length:
        n *= 2
    return n


def frame_count(samples: int, win_length: int, hop_length: int) -> int:
    """Frames of an un-centred, un-padded STFT: 0 below one window, else 1 + (L - win) // hop."""
    return 0 if win_length < 1 or samples < win_length else 1 + (samples - win_length) // hop_length


def _bins(win_length: int) -> int:
    return fft_length(win_length) // 2 + 1 if win_length > 0 else 0


class Scores(object):
    """The result of a scoring call: `.table`, float64 [n, 4] = {abs_sum, samples, power_sum, terms} per utterance (on the device when it
    comes from score / score_varlen / mel_l1; any array-like otherwise), and what follows from it.  Reading any property but `.table`
    copies the table to the host (and so waits for the call); nothing is cached, so a Scores over a captured graph's table reads the
    latest replay."""

    def __init__(self, table, win_length=0):
        self.table = table
        self.win_length = int(win_length)

    def numpy(self):
        t = self.table
        return (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).astype(np.float64).reshape(-1, 4)

    @staticmethod
    def _ratio(a, b):
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        with np.errstate(divide='ignore', invalid='ignore'):
            return np.where(b > 0, a / np.where(b > 0, b, 1.0), np.nan)

    @property
    def l1(self):
        """Per utterance: abs_sum / samples (NaN for an empty utterance)."""
        t = self.numpy()
        return self._ratio(t[:, 0], t[:, 1])

    @property
    def power(self):
        """Per utterance: power_sum / terms -- NaN where the utterance is shorter than one window (or in the L1-only mode)."""
        t = self.numpy()
        return self._ratio(t[:, 2], t[:, 3])

    @property
    def samples(self):
        return self.numpy()[:, 1].astype(np.int64)

    @property
    def frames(self):
        """Per utterance: STFT frames that entered power_sum."""
        t, b = self.numpy(), _bins(self.win_length)
        return (t[:, 3] / b).round().astype(np.int64) if b else np.zeros(len(t), np.int64)

    @property
    def likelihood(self):
        """The batch's loss/likelihood: sum abs_sum / sum samples (reduce_mean over all elements)."""
        t = self.numpy()
        return float(self._ratio(t[:, 0].sum(), t[:, 1].sum()))

    @property
    def power_loss(self):
        """The batch's loss/power: sum power_sum / sum terms; an utterance without a frame contributes to neither sum."""
        t = self.numpy()
        return float(self._ratio(t[:, 2].sum(), t[:, 3].sum()))

    def total(self, weight=None):
        """likelihood + weight * power_loss (the reference's combined loss); weight defaults to hp.train.weight_power_loss."""
        w = float(hp.train.weight_power_loss if weight is None else weight)
        t = self.numpy()
        return float(self._ratio(t[:, 0].sum(), t[:, 1].sum()) + w * self._ratio(t[:, 2].sum(), t[:, 3].sum()))


def _settings(win_length, hop_length):
    from . import _lib
    win = int(hp.signal.win_length if win_length is None else win_length)
    hop = int(hp.signal.hop_length if hop_length is None else hop_length)
    if win < 0 or win > _lib.SCORE_MAX_WIN:
        raise ValueError('win_length %d must be 0 (L1 only) .. %d' % (win, _lib.SCORE_MAX_WIN))
    if hop < 1:
        raise ValueError('hop_length %d must be >= 1' % hop)
    return win, hop


def _launch(out, y, cu_rows, n, T, rows, win, hop):
    """One pwv_score_f32 over flat `out` / `y` [>= rows]: the float64 [n, 4] table (device)."""
    from . import _lib, engine
    a = _lib.ScoreArgs()
    a.out, a.y, a.cu_rows = out.data_ptr(), y.data_ptr(), None if cu_rows is None else cu_rows.data_ptr()
    a.n, a.T, a.rows, a.win_length, a.hop_length = n, T, rows, win, hop
    need = int(_lib.lib().pwv_score_workspace_bytes(ctypes.byref(a)))
    if need == 0:
        _lib.check(-1, 'pwv_score_workspace_bytes')
    table = torch.empty((n, 4), dtype=torch.float64, device=out.device)
    work = torch.empty((need // 8,), dtype=torch.float64, device=out.device)
    a.result, a.workspace, a.workspace_bytes = table.data_ptr(), work.data_ptr(), need
    _lib.check(_lib.lib().pwv_score_f32(ctypes.byref(a), engine._stream()), 'pwv_score_f32')
    return table


def _uniform(t, what):
    from . import engine
    t = engine._require_cuda_f32(t, what)
    if t.dim() == 3 and t.shape[2] == 1:
        t = t[:, :, 0]
    if t.dim() != 2:
        raise ValueError('%s must be [N, L, 1] or [N, L], got %s' % (what, tuple(t.shape)))
    return t.contiguous()


def score(pred, gt, win_length=None, hop_length=None) -> Scores:
    """pred, gt: CUDA float32 [N, L, 1] or [N, L] -> Scores of the N utterances.  win_length / hop_length default to hp.signal's;
    win_length=0 scores the L1 alone."""
    win, hop = _settings(win_length, hop_length)
    pred, gt = _uniform(pred, 'pred'), _uniform(gt, 'gt')
    if pred.shape != gt.shape or pred.device != gt.device:
        raise ValueError('pred %s and gt %s differ in shape or device' % (tuple(pred.shape), tuple(gt.shape)))
    n, length = pred.shape
    if n < 1:
        raise ValueError('nothing to score: pred is %s' % (tuple(pred.shape),))
    return Scores(_launch(pred, gt, None, n, length, n * length, win, hop), win)


def _flat(t, what):
    from . import engine
    t = engine._require_cuda_f32(t, what)
    if t.dim() == 2 and t.shape[1] == 1:
        t = t[:, 0]
    if t.dim() != 1:
        raise ValueError('%s must be [len, 1] or [len], got %s' % (what, tuple(t.shape)))
    return t.contiguous()


def _packed(items, what):
    """(flat [rows] tensor, lengths) of a list of [len_i, 1] tensors, or of a VarlenOutput / RaggedOutput (its .packed, no copy)."""
    lengths = [int(p.shape[0]) for p in items]
    whole = getattr(items, 'packed', None)
    if whole is not None and int(whole.shape[0]) == sum(lengths):
        return _flat(whole, what + '.packed'), lengths
    pieces = [_flat(p, '%s[%d]' % (what, i)) for i, p in enumerate(items)]
    flat = torch.empty((sum(lengths),), dtype=torch.float32, device=pieces[0].device)
    at = 0
    for p in pieces:
        flat[at:at + p.shape[0]].copy_(p)
        at += p.shape[0]
    return flat, lengths


def score_varlen(preds, gts, win_length=None, hop_length=None, cu_rows=None) -> Scores:
    """Utterances of different lengths in one call.  preds, gts: lists of [len_i, 1] (or [len_i]) CUDA float32 tensors, or the
    VarlenOutput / RaggedOutput of generate_varlen / push_varlen (their `.packed` is scored in place).  A prediction whose length differs
    from its ground truth's is a ValueError naming the utterance.

    The CAPACITY form, for a captured graph: preds and gts are packed tensors [rows, 1] (or [rows]) and cu_rows a device int32 [n + 1]
    of prefix sums.  The lengths are then read on the device alone -- nothing here looks at them -- so a capture of the call is replayed
    for any bounds written into the same cu_rows tensor that fit n and rows."""
    win, hop = _settings(win_length, hop_length)
    if cu_rows is not None:
        pred, gt = _flat(preds, 'preds'), _flat(gts, 'gts')
        if pred.shape != gt.shape or pred.device != gt.device:
            raise ValueError('preds %s and gts %s differ in shape or device' % (tuple(pred.shape), tuple(gt.shape)))
        if not isinstance(cu_rows, torch.Tensor) or cu_rows.dtype != torch.int32 or cu_rows.dim() != 1 or cu_rows.shape[0] < 2 \
                or cu_rows.device != pred.device or not cu_rows.is_contiguous():
            raise ValueError('cu_rows must be a contiguous int32 [n + 1] tensor on the device of preds')
        n = int(cu_rows.shape[0]) - 1
        return Scores(_launch(pred, gt, cu_rows, n, 0, int(pred.shape[0]), win, hop), win)
    for what, items in (('preds', preds), ('gts', gts)):
        if not isinstance(items, (list, tuple)) or not len(items):
            raise ValueError('%s must be a non-empty list of [len, 1] tensors' % what)
    if len(preds) != len(gts):
        raise ValueError('%d predictions for %d ground truths' % (len(preds), len(gts)))
    for i, (a, b) in enumerate(zip(preds, gts)):
        if int(a.shape[0]) != int(b.shape[0]):
            raise ValueError('utterance %d: the prediction has %d samples, its ground truth %d' % (i, a.shape[0], b.shape[0]))
    pred, lengths = _packed(preds, 'preds')
    gt, _ = _packed(gts, 'gts')
    if pred.device != gt.device:
        raise ValueError('preds and gts live on different devices')
    cu = torch.tensor(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32), dtype=torch.int32, device=pred.device)
    return Scores(_launch(pred, gt, cu, len(lengths), 0, int(pred.shape[0]), win, hop), win)


def mel_l1(mel_a, mel_b) -> Scores:
    """The L1 of two mels (the kernel's L1-only mode, win_length = 0): [N, frames, n_mels] tensors, or lists of [frames_i, n_mels].
    `.l1` is the mean |a - b| per utterance, `.likelihood` over the batch.  Used as mel_l1(wav_to_mel_device(pred), mel_in): what the
    vocoder kept of its conditioning, measurable without a ground-truth wav."""
    if isinstance(mel_a, (list, tuple)):
        if not isinstance(mel_b, (list, tuple)) or len(mel_a) != len(mel_b):
            raise ValueError('mel_a and mel_b must be lists of the same length')
        for i, (a, b) in enumerate(zip(mel_a, mel_b)):
            if tuple(a.shape) != tuple(b.shape):
                raise ValueError('utterance %d: mels of shape %s and %s' % (i, tuple(a.shape), tuple(b.shape)))
        return score_varlen([a.reshape(-1) for a in mel_a], [b.reshape(-1) for b in mel_b], win_length=0, hop_length=1)
    if tuple(mel_a.shape) != tuple(mel_b.shape) or mel_a.dim() < 2:
        raise ValueError('mels of shape %s and %s' % (tuple(mel_a.shape), tuple(mel_b.shape)))
    return score(mel_a.reshape(mel_a.shape[0], -1), mel_b.reshape(mel_b.shape[0], -1), win_length=0, hop_length=1)


def power_frames(x, win_length: int, hop_length: int):
    """|rfft|^2 of the frames of one utterance `x` [L] (float64 arithmetic on the values as given): [F, fft_length / 2 + 1]."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    frames, nfft = frame_count(len(x), win_length, hop_length), fft_length(win_length)
    if frames == 0:
        return np.zeros((0, nfft // 2 + 1))
    window = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win_length) / win_length)
    idx = hop_length * np.arange(frames)[:, None] + np.arange(win_length)[None, :]
    spec = np.fft.rfft(x[idx] * window, n=nfft, axis=1)              # (n > win: zero-padded behind)
    return spec.real ** 2 + spec.imag ** 2


def score_reference(pred, gt, win_length: int, hop_length: int):
    """The numpy float64 restatement of the table: pred, gt = arrays [N, L] / [N, L, 1] or lists of [len_i] / [len_i, 1] utterances ->
    float64 [n, 4] = {abs_sum, samples, power_sum, terms}.  The values are used as given (float32 inputs are what the device sees)."""
    def utterances(v, what):
        if isinstance(v, (list, tuple)):
            return [np.asarray(u, dtype=np.float64).reshape(-1) for u in v]
        v = np.asarray(v, dtype=np.float64)
        if v.ndim == 3 and v.shape[2] == 1:
            v = v[:, :, 0]
        if v.ndim != 2:
            raise ValueError('%s must be [N, L], [N, L, 1] or a list of utterances, got %s' % (what, v.shape))
        return list(v)

    a, b = utterances(pred, 'pred'), utterances(gt, 'gt')
    if len(a) != len(b):
        raise ValueError('%d predictions for %d ground truths' % (len(a), len(b)))
    table = np.zeros((len(a), 4))
    for i, (p, y) in enumerate(zip(a, b)):
        if p.shape != y.shape:
            raise ValueError('utterance %d: the prediction has %d samples, its ground truth %d' % (i, len(p), len(y)))
        table[i, 0], table[i, 1] = np.abs(p - y).sum(), len(p)
        if win_length > 0:
            d = power_frames(p, win_length, hop_length) - power_frames(y, win_length, hop_length)
            table[i, 2], table[i, 3] = (d * d).sum(), d.size
    return table
