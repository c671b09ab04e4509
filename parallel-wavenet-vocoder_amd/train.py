"""Training of the IAF-WaveNet student, on one GPU or data-parallel over the GPUs of a node: the reference's loss (models.py:90-99: the L1, and on request weight_power_loss
times the STFT power loss -- pwv_train_loss_f32, include/pwv_hip_train_loss.h), its gradient for every variable (pwv_train_* kernels,
include/pwv_hip_train.h), TensorFlow's Adam and the reference's EMA (models.py:72-76, :101-103), and the loop of train.py:25-71.
DESIGN.md section 9, "Training".

    python -m pwv_amd.train CASE [--ckpt=NAME] [--steps=N] [--seed=S] [--varlen] [--gpus=N]

Scope: what hparams/default.yaml trains -- filter_width 2, R = D = 64, S = 128, 'repeat' conditioning, no normalisers, no skip
accumulation, separate scaler and shifter nets, exact-fp32 arithmetic; uniform [N, T] batches (loss_and_grad) or packed batches of
utterances of different lengths, unpadded (loss_and_grad_varlen, `--varlen`).  And the reference's second architecture,
cond_upsample_method 'transposed_conv' (models.py:109-124; hparams test/tran): uniform batches at hop_length 80 = 4 * 4 * 5, an even
condition_channels <= 96, no normalised conditioning.  And, on request (use_skip_connection=True; the command line asks when the case
sets model.use_skip_connection, hparams train/small_skip), the skip-connection architecture (modules.py:142-147, :242-250): the head
of every net reads the sum of all layers' skip outputs -- uniform and packed batches, one GPU or data-parallel, with or without the
power loss (include/pwv_hip_train_skip.h; DESIGN.md section 9, "Training the skip-connection architecture"); not together with
'transposed_conv'.  And, on request too (shared_nets=True; the command line asks when the case sets model.shared_nets, hparams
train/small_shared), the project's own shared-net architecture (modules.SharedIAFLayer, bench/c2): ONE net per flow whose head has two
outputs, out = x y[..., 0] + y[..., 1] -- the two-output head of include/pwv_hip_train_shared.h on the unchanged layer kernels; uniform
and packed batches, with skip connections (both requests), the power loss, fused or data-parallel, or 'transposed_conv' (DESIGN.md
section 9, "Training the shared-net architecture").  Everything else is refused with a PwvError that names the reason (`refusal`);
nothing falls back to another implementation.

Data-parallel (the reference's SyncMultiGPUTrainerReplicated, train.py:66-69): DataParallelTrainer, one replica per rank; the gradients
of a step are packed into ONE flat arena, all-reduced once, and one fused Adam + EMA launch applies the same update on every rank
(include/pwv_hip_train_opt.h; Trainer(fused=True) is the same optimiser in one process).  DESIGN.md section 9, "Data-parallel training".

Division of work.  Sample rate (the hot path): HIP kernels, one net per call -- the forward keeps every layer's input and the last
layer's gated output, the backward recomputes F, G, o and the head's hidden layers from them.  Frame rate: the conditioning dense +
ReLU and the projections P = frames [gc_filter | gc_gate] + [filter_bias | gate_bias] of all net-layers as ONE matrix product, both on
the project's exact-fp32 GEMM (pwv_linear_f32: a row of P does not depend on the rows next to it); in torch (plumbing) their backward
from the dP the kernels leave, the flow's affine out = in * s + b and the loss.

The driver.  One _net_forward and one _net_backward serve every architecture and both head widths.  What differs between them is
data on the _Geometry of the batch: the batch itself (_Uniform or _Packed), the conditioning (_Projected: P; _PerSample: the
condition below) and the two architecture flags; its `front`, `layer` and `head` name the entry point of a call and fill its struct,
and _call is the one place a training kernel is enqueued.

Transposed-conv conditioning.  The condition changes every sample, so there is no P: the layer kernels of
include/pwv_hip_train_cond.h form c[t] [gc_filter | gc_gate] + biases, the gradients of gc_* and of the biases, and d_cond inside the
unit.  The three stride-4/4/5 stages run as linear_op(..., relu) on the re-laid-out [Cin, s C] weights (as models._condition does) and
keep their outputs; the kernels read the last stage's UNCROPPED output through a row offset (no crop), add every net-layer's d_cond
into one buffer of the same shape whose margins stay zero (the crop's adjoint), and torch takes that back through the stages.
"""
from __future__ import annotations

import ctypes
import glob
import math
import os
import sys
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _lib
from ._lib import PwvError
from .hparam import hparam as hp
from .variables import EMA_SUFFIX, get_default_store, variable_scope

SCOPE = 'iaf_vocoder'
ADAM_BETA1 = 0.9            # tf.train.AdamOptimizer's defaults (models.py:101-103 sets the learning rate and beta2 only)
ADAM_EPS = 1e-8
TCONV_STRIDES = (4, 4, 5)   # models.py:109-124: the strides of the three transposed convolutions; their product is the hop


# ---- what is refused ----------------------------------------------------------------------------------------------------------------
def refusal(model=None, wav=None, melspec=None, power_weight=None, packed=False, use_skip_connection=None, *,
            shared_nets: Optional[bool] = None) -> Optional[str]:
    """Why the current hparams / this model / these inputs cannot be trained here, or None.  Looks at structure only: no GPU.
    `power_weight`: the weight of the STFT power loss the caller asks for explicitly (loss_and_grad's argument); None = the L1 alone,
    and then hparams that ask for a power loss are refused instead of being trained without it.  `packed`: the caller is
    loss_and_grad_varlen, which takes its lengths from the utterances and not from the model.  `use_skip_connection`: True = the
    caller asks for the skip-connection architecture (hparams that say False are then a mismatch); None = the default architecture,
    and hparams with model.use_skip_connection are refused instead of being trained as something else.  `shared_nets`: the same for
    the shared-net architecture (model.shared_nets: one net with two outputs per flow); the two requests combine."""
    m = hp.model
    if use_skip_connection not in (None, True):
        return 'use_skip_connection %r: pass True to train the skip-connection architecture, None for the default one' % (use_skip_connection,)
    if use_skip_connection and not m.use_skip_connection:
        return ('use_skip_connection=True under hparams with model.use_skip_connection False: the request does not match the '
                'architecture the hparams describe')
    if shared_nets not in (None, True):
        return 'shared_nets %r: pass True to train the shared-net architecture, None for separate scaler and shifter nets' % (shared_nets,)
    if shared_nets and not m.get('shared_nets'):
        return ('shared_nets=True under hparams with model.shared_nets False: the request does not match the architecture the hparams '
                'describe')
    if m.cond_upsample_method == 'transposed_conv':
        what = "cond_upsample_method 'transposed_conv': transposed-conv conditioning is differentiated "
        hop, C = int(hp.signal.hop_length), int(m.condition_channels)
        if hop != int(np.prod(TCONV_STRIDES)):
            return what + 'at hop_length 80 only, not at hop_length %d: the strides %s multiply to %d' % (hop, TCONV_STRIDES, int(np.prod(TCONV_STRIDES)))
        if m.get('normalize_cond'):
            return what + 'without normalisers only, not with normalize_cond %r' % m.normalize_cond
        if C < 2 or C % 2 or C > _lib.TRAIN_COND_MAX:
            return what + 'for an even condition_channels of 2 .. %d, not %d (the per-sample layer kernels)' % (_lib.TRAIN_COND_MAX, C)
        if packed or any(isinstance(t, (list, tuple)) for t in (wav, melspec)):
            return what + 'on uniform [N, T] batches only: per-sample conditioning is not packed (generate_varlen pads such batches too)'
    elif m.cond_upsample_method != 'repeat':
        return "cond_upsample_method %r: only 'repeat' and 'transposed_conv' conditioning are differentiated" % m.cond_upsample_method
    if m.get('normalize_cond'):
        return 'normalize_cond %r: normalised conditioning is not differentiated' % m.normalize_cond
    if m.get('normalize_wavenet'):
        return "normalize_wavenet %r: the 'bn' / 'in' normalisers are not differentiated" % m.normalize_wavenet
    if m.get('normalize'):
        return "normalize %r: the 'bn' / 'in' normalisers are not differentiated" % m.normalize
    if m.use_skip_connection and not use_skip_connection:
        return ('use_skip_connection True: skip accumulation over all layers is not differentiated by a bare call; it is trained on '
                'request (loss_and_grad / loss_and_grad_varlen / Trainer: use_skip_connection=True)')
    if m.use_skip_connection and m.cond_upsample_method == 'transposed_conv':
        return ("use_skip_connection True with cond_upsample_method 'transposed_conv': skip accumulation is not differentiated together "
                'with per-sample conditioning (the per-sample layer kernels\' 62 KB of LDS and the dS tile leave no room for two workgroups '
                'per compute unit)')
    if m.get('shared_nets') and not shared_nets:
        return ('shared_nets True: one shared net per flow is not differentiated by a bare call; it is trained on request '
                '(loss_and_grad / loss_and_grad_varlen / Trainer: shared_nets=True)')
    shape = (m.filter_width, m.residual_channels, m.dilation_channels, m.skip_channels)
    if shape != (2, 64, 64, 128):
        return 'filter_width, residual, dilation, skip channels = %s: outside the fused shape (2, 64, 64, 128)' % (shape,)
    if len(m.dilations) != m.n_iaf or any(len(d) < 1 or min(d) < 1 for d in m.dilations):
        return 'dilations %r do not give n_iaf = %d flows of at least one layer' % (m.dilations, m.n_iaf)
    if power_weight is None and float(hp.train.get('weight_power_loss', 0) or 0) > 0:
        return ('train.weight_power_loss %g > 0: this call differentiates the L1 alone; the STFT power loss is trained on request '
                '(loss_and_grad / Trainer: power_weight=...)' % float(hp.train.weight_power_loss))
    if power_weight is not None:
        if not (math.isfinite(float(power_weight)) and float(power_weight) >= 0):
            return 'power_weight %r must be a finite number >= 0' % (power_weight,)
        length = None if packed else getattr(model, 'length', None)
        if float(power_weight) > 0 and length is not None and length < int(hp.signal.win_length):
            return ('power_weight %g > 0 with length %d shorter than signal.win_length %d: the STFT power loss has no frame'
                    % (float(power_weight), length, int(hp.signal.win_length)))
    prec = getattr(model, 'precision', None)
    if prec not in (None, 'f32'):
        return "precision %r: training runs in exact fp32 ('f16x3' / 'f16' are not differentiated)" % prec
    for what, t in (('wav', wav), ('melspec', melspec)):
        if isinstance(t, (list, tuple)):
            return 'packed inputs: %s is a list of utterances (uniform [N, T] batches only)' % what
        if t is not None and (hasattr(t, 'push') or hasattr(t, 'cu_rows')):
            return 'streaming inputs: %s is a stream (uniform [N, T] batches only)' % what
    if melspec is not None and getattr(melspec, 'dim', lambda: 3)() != 3:
        return 'packed inputs: melspec must be [N, t_mel, n_mels], got %s' % (tuple(melspec.shape),)
    return None


# ---- the variables ------------------------------------------------------------------------------------------------------------------
class _Net(object):
    """One WaveNet of the model: its variables by role, its dilations, its first column in the projection bank."""

    def __init__(self, net, col):
        self.scope, self.dilations, self.col = net.full_scope, list(net.dilations), col
        self.cf = net.causal_filter()
        self.layers = [net.layer_variables(j, with_cond=True) for j in range(len(self.dilations))]
        self.head = net.head_variables()

    def name(self, j, role):
        return '%s/dilated_stack/layer%d/%s' % (self.scope, j, role)


def model_nets(model, store) -> List[List[_Net]]:
    """[[scaler, shifter] per flow]; creates (glorot / zeros, like tf.get_variable) every variable the store lacks."""
    with variable_scope(SCOPE, absolute=True):
        flows = model._flows(store, True, 'f32')
    out, col = [], 0
    for iaf in flows:
        pair = []
        for net in iaf.nets():
            pair.append(_Net(net, col))
            col += 128 * len(net.dilations)
        out.append(pair)
    return out


def cond_dense(store):
    return store.get_variable(SCOPE + '/cond/dense', [1, hp.signal.n_mels, hp.model.condition_channels])


def cond_tconv(store):
    """The three transposed-conv weights, TF layout [1, stride, C, Cin] (models.py:113-116)."""
    C = hp.model.condition_channels
    return [store.get_variable(SCOPE + '/cond/transposed_conv_%d_weights' % i, [1, s, C, C if i else hp.signal.n_mels])
            for i, s in enumerate(TCONV_STRIDES)]


def cond_variables(store):
    """The variables of the conditioning the hparams choose (created if the store lacks them)."""
    return cond_tconv(store) if hp.model.cond_upsample_method == 'transposed_conv' else [cond_dense(store)]


def trainable_names(store) -> List[str]:
    return sorted(store.trainable_variables(SCOPE))


# ---- the kernels --------------------------------------------------------------------------------------------------------------------
def _ptr(t):
    return None if t is None else t.data_ptr()


def _call(name, args):
    from . import engine
    _lib.check(getattr(_lib.lib(), name)(ctypes.byref(args), engine._stream()), name)


def _tile32(rows, device):
    return torch.empty(((rows + 31) // 32) * 32 * 64, dtype=torch.float32, device=device)


def _tile32w(rows, device):
    return torch.empty(((rows + 31) // 32) * 32 * 128, dtype=torch.float32, device=device)


def _fill(a, kw):
    """Set the fields `kw` of the struct `a`, tensors as their addresses (a struct with an embedded pwv_train_args routes the names)."""
    kw = {k: _ptr(v) if isinstance(v, torch.Tensor) else v for k, v in kw.items()}
    if isinstance(a, _lib.EmbedsTrainArgs):
        return a.set(**kw)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


class _Uniform(object):
    """A uniform batch [N, T] with `frames` condition frames per utterance (include/pwv_hip_train.h)."""
    prefix = 'pwv_train_'

    def __init__(self, N, T, frames):
        self.N, self.T, self.rows, self.frames = N, T, N * T, frames

    def tables(self):
        return {}

    def args(self, **common):
        return _lib.TrainArgs(N=self.N, T=self.T, cond_frames=self.frames, **common)


class _Packed(object):
    """A packed batch (include/pwv_hip_train_varlen.h): `layout` an engine.VarlenGeometry.  The entry points that depend on where an
    utterance begins take the device tables; to a row-local call (the head, the workspace) the batch is uniform at N = 1, T = rows."""
    prefix = 'pwv_train_varlen_'

    def __init__(self, layout):
        self.layout = layout
        self.N, self.T, self.rows, self.frames = 1, layout.rows, layout.rows, layout.total_frames

    def tables(self):
        g = self.layout
        return dict(cu_rows=_ptr(g.cu_rows), cu_frames=_ptr(g.cu_frames), n=g.n, rows=g.rows, proj_rows=g.total_frames)

    def args(self, **common):
        return _lib.TrainVarlenArgs(**common, **self.tables())


class _Projected(object):
    """Conditioning at frame rate: a layer reads its 128 columns of the projection `P` and fills its slots of dP."""
    per_sample = False
    P = None

    def fwd(self, net, j, v):
        """What a layer's forward call reads of the conditioning."""
        return dict(proj=self.P[0, net.col + 128 * j:])

    def bwd(self, net, j, v, dP, g, opt):
        """... and its backward call: P, and the dP slots it fills."""
        return dict(proj=self.P[0, net.col + 128 * j:], d_proj=dP[0, net.col + 128 * j:])


class _PerSample(object):
    """A per-sample condition on a uniform batch (include/pwv_hip_train_cond.h): the layer calls read `cond`, the uncropped
    [N, T + hop, C] output of the last transposed-conv stage, through a row offset of hop / 2, and add to `d_cond` of the same shape
    (zeros to begin with: its margins are the crop's adjoint).  The front, the head and the loss are the uniform ones."""
    per_sample = True

    def __init__(self, C):
        self.C = C
        self.cond = self.d_cond = None
        self.started = 0                    # the first layer backward of a step writes its rows of d_cond, the others add

    def set(self, cond):
        assert cond.is_contiguous()
        self.cond, self.d_cond, self.started = cond, torch.zeros_like(cond), 0

    def args(self, geo):
        skip = geo.off * self.C * 4         # bytes to sample 0 of utterance 0
        return _lib.TrainCondArgs(N=geo.N, T=geo.T, max_workgroups=geo.max_workgroups, dilation=1, next_dilation=1,
                                  cond=self.cond.data_ptr() + skip, d_cond=self.d_cond.data_ptr() + skip, cond_channels=self.C,
                                  cond_row_stride=self.C, cond_utt_rows=geo.T + geo.hop)

    def fwd(self, net, j, v):
        return dict(gc_filter=v['gc_filter'], gc_gate=v['gc_gate'], filter_bias=v.get('filter_bias'), gate_bias=v.get('gate_bias'))

    def bwd(self, net, j, v, dP, g, opt):
        kw = dict(self.fwd(net, j, v), d_gc_filter=g(net.name(j, 'gc_filter'), v['gc_filter']),
                  d_gc_gate=g(net.name(j, 'gc_gate'), v['gc_gate']), d_filter_bias=opt(v, 'filter_bias', net.name(j, 'filter_bias')),
                  d_gate_bias=opt(v, 'gate_bias', net.name(j, 'gate_bias')), d_cond_accumulate=self.started)
        self.started = 1
        return kw


class _Geometry(object):
    """Which entry point a call of a batch goes to and the struct it takes: `batch` a _Uniform or a _Packed, `cond` a _Projected (`cols`
    the columns of P) or a _PerSample, `skip` the skip-connection architecture (include/pwv_hip_train_skip.h: its layer and head calls
    take pwv_train_skip_args -- the batch's own struct in front, the packed tables copied behind it), `shared` one net per flow with
    two outputs (include/pwv_hip_train_shared.h: its head calls take pwv_train_shared_args -- the uniform struct in front, row-local).
    `front`, `layer` and `head` return (entry point, filled struct): the arguments of _call."""

    def __init__(self, batch, cond, cols, max_workgroups, skip=False, shared=False):
        self.batch, self.cond, self.cols, self.max_workgroups, self.skip, self.shared = batch, cond, cols, max_workgroups, skip, shared
        self.N, self.T, self.rows, self.frames = batch.N, batch.T, batch.rows, batch.frames
        self.hop, self.off = hp.signal.hop_length, hp.signal.hop_length // 2
        self.kmax = (self.hop + 30) // 32 + 1

    def _common(self):
        return dict(cond_hop=self.hop, cond_offset=self.off, proj_row_stride=self.cols, d_proj_row_stride=self.cols,
                    max_workgroups=self.max_workgroups, dilation=1, next_dilation=1)

    def _row_local(self):
        return _lib.TrainArgs(N=self.N, T=self.T, cond_frames=self.frames, **self._common())

    def _skip_args(self):
        return _lib.TrainSkipArgs(**self.batch.tables()).embed(self.batch.args(**self._common()))

    def front(self, kind, **kw):
        """'front_fwd' or 'front_bwd'."""
        return '%s%s_f32' % (self.batch.prefix, kind), _fill(self.batch.args(**self._common()), kw)

    def layer(self, kind, **kw):
        """'layer_fwd' or 'layer_bwd'."""
        if self.skip:
            return 'pwv_train_skip_%s_f32' % kind, _fill(self._skip_args(), kw)
        if self.cond.per_sample:
            return 'pwv_train_cond_%s_f32' % kind, _fill(self.cond.args(self), kw)
        return self.front(kind, **kw)

    def head(self, kind, **kw):
        """'fwd' or 'bwd' of the head, which is row-independent: the same call for either batch."""
        if self.shared:
            head_in = _lib.TRAIN_HEAD_IN_SKIPSUM if self.skip else _lib.TRAIN_HEAD_IN_GATED
            return 'pwv_train_shared_head_%s_f32' % kind, _fill(_lib.TrainSharedArgs(head_in=head_in).embed(self._row_local()), kw)
        if self.skip:
            return 'pwv_train_skip_head_%s_f32' % kind, _fill(self._skip_args(), kw)
        return 'pwv_train_head_%s_f32' % kind, _fill(self._row_local(), kw)

    def workspace(self, device):
        """The workspace of every weight-gradient reduction of the batch: the largest any of its calls asks for."""
        if self.skip:
            asks = [('pwv_train_skip_workspace_bytes', self._skip_args())]
        elif self.cond.per_sample:
            asks = [('pwv_train_cond_workspace_bytes', self.cond.args(self))]
        else:
            asks = [('pwv_train_workspace_bytes', self._row_local())]
        if self.shared:                     # the two-output head's partial is the larger one
            asks.append(('pwv_train_shared_workspace_bytes', self.head('fwd')[1]))
        need = 0
        for name, a in asks:
            got = getattr(_lib.lib(), name)(ctypes.byref(a))
            if not got:
                _lib.check(-1, name)
            need = max(need, got)
        return torch.empty(need // 4, dtype=torch.float32, device=device)


def _net_forward(net: _Net, geo: _Geometry, xin):
    """x_j for every layer, the head's input and the net's output y [rows] ([2, rows] of a shared net: the scale plane, the shift
    plane).  The head's input is the last layer's o -- or, under skip connections, the net's skip sum S: layer 0 writes it, every other
    layer adds to it in stream order, and the last layer has no dense product and leaves no o."""
    dev, L = xin.device, len(net.dilations)
    xs = [_tile32(geo.rows, dev) for _ in range(L)]
    hin = (_tile32w if geo.skip else _tile32)(geo.rows, dev)
    y = torch.empty((2, geo.rows) if geo.shared else geo.rows, dtype=torch.float32, device=dev)
    _call(*geo.front('front_fwd', in_=xin, causal_filter=net.cf, x_out=xs[0]))
    for j, d in enumerate(net.dilations):
        v, last = net.layers[j], j == L - 1
        dense = not (last and geo.skip)
        x_out = (None if geo.skip else hin) if last else xs[j + 1]
        skip = dict(skip=v['skip'], skip_bias=v.get('skip_bias'), skip_sum=hin, skip_accumulate=int(j > 0)) if geo.skip else {}
        _call(*geo.layer('layer_fwd', form=_lib.TRAIN_LAST if last else _lib.TRAIN_RESIDUAL, dilation=d, x=xs[j], filter=v['filter'],
                         gate=v['gate'], dense=v['dense'] if dense else None, dense_bias=v.get('dense_bias') if dense else None,
                         x_out=x_out, **skip, **geo.cond.fwd(net, j, v)))
    h, lv = net.head, net.layers[-1]
    front = dict(skip_sum=hin) if geo.skip else dict(x=hin, skip=lv['skip'], skip_bias=lv.get('skip_bias'))
    out = dict(y=y[0], y_shift=y[1]) if geo.shared else dict(y=y)
    _call(*geo.head('fwd', post1=h['postprocess1'], post1_bias=h.get('postprocess1_bias'), post2=h['postprocess2'],
                    post2_bias=h.get('postprocess2_bias'), **front, **out))
    return xs, hin, y


def _net_backward(net: _Net, geo: _Geometry, saved, xin, d_out, d_mul, scale, d_in, accumulate, dP, ws, grads):
    """The net's share of the gradients into `grads`, of dP and of d_in.  Under skip connections the head leaves dS and its column
    sums, which are every layer's d skip_bias; every layer takes dS skip^T into its d o and leaves its d skip."""
    xs, hin, _ = saved
    dev, L = xin.device, len(net.dilations)
    g = lambda name, like: grads.setdefault(name, torch.empty_like(like))
    h, lv = net.head, net.layers[-1]
    hp_ = net.scope + '/postprocessing/'
    opt = lambda d, key, name: g(name, d[key]) if key in d else None
    d_hin = torch.empty_like(hin)           # d o, or dS
    if geo.skip:
        biased = [j for j in range(L) if 'skip_bias' in net.layers[j]]
        sums = torch.empty(128, dtype=torch.float32, device=dev) if biased else None
        front = dict(skip_sum=hin, d_skip_sum_out=d_hin, d_skip_bias=sums)
    else:
        front = dict(x=hin, skip=lv['skip'], skip_bias=lv.get('skip_bias'), d_o_out=d_hin, d_skip=g(net.name(L - 1, 'skip'), lv['skip']),
                     d_skip_bias=opt(lv, 'skip_bias', net.name(L - 1, 'skip_bias')))
    _call(*geo.head(
        'bwd', d_out=d_out, d_mul=d_mul, post1=h['postprocess1'], post1_bias=h.get('postprocess1_bias'), post2=h['postprocess2'],
        post2_bias=h.get('postprocess2_bias'), **front,
        d_post1=g(hp_ + 'postprocess1', h['postprocess1']), d_post1_bias=opt(h, 'postprocess1_bias', hp_ + 'postprocess1_bias'),
        d_post2=g(hp_ + 'postprocess2', h['postprocess2']), d_post2_bias=opt(h, 'postprocess2_bias', hp_ + 'postprocess2_bias'),
        workspace=ws, workspace_bytes=ws.numel() * 4))
    if geo.skip and biased:
        copies = sums.repeat(len(biased), 1)                                            # one launch: the same bits for every layer
        for k, j in enumerate(biased):
            grads[net.name(j, 'skip_bias')] = copies[k]
    uv = [(_tile32(geo.rows, dev), _tile32(geo.rows, dev)) for _ in range(2)]
    for j in range(L - 1, -1, -1):
        v, last = net.layers[j], j == L - 1
        u_next, v_next = (None, None) if last else uv[(j + 1) & 1]
        if geo.skip:
            skip = dict(dense=None if last else v['dense'], skip=v['skip'], d_skip_sum=d_hin, d_skip=g(net.name(j, 'skip'), v['skip']))
        else:
            skip = dict(dense=v['dense'], d_o=d_hin if last else None)
        _call(*geo.layer(
            'layer_bwd', form=_lib.TRAIN_LAST if last else _lib.TRAIN_RESIDUAL, dilation=net.dilations[j],
            next_dilation=1 if last else net.dilations[j + 1], x=xs[j],
            filter=v['filter'], gate=v['gate'], u_next=u_next, v_next=v_next, **skip,
            u=uv[j & 1][0], v=uv[j & 1][1], **geo.cond.bwd(net, j, v, dP, g, opt),
            d_filter=g(net.name(j, 'filter'), v['filter']), d_gate=g(net.name(j, 'gate'), v['gate']),
            d_dense=None if last else g(net.name(j, 'dense'), v['dense']),
            d_dense_bias=None if last else opt(v, 'dense_bias', net.name(j, 'dense_bias')),
            workspace=ws, workspace_bytes=ws.numel() * 4))
    _call(*geo.front(
        'front_bwd', in_=xin, causal_filter=net.cf, u_next=uv[0][0], v_next=uv[0][1], next_dilation=net.dilations[0], d_out=d_out,
        scale=scale, d_in=d_in, accumulate=int(accumulate), d_causal_filter=g(net.scope + '/causal_layer/filter', net.cf),
        workspace=ws, workspace_bytes=ws.numel() * 4))


def _loss_head(pred, y, shape, w):
    """The loss head on the device: weight_l1 = 1, weight_power = w, hp.signal.win_length / hop_length.  `shape`: (N, T) of a uniform
    batch (pwv_train_loss_f32) or the engine.VarlenGeometry of a packed one (pwv_train_loss_varlen_f32: the lengths are read from
    layout.cu_rows on the device).  Returns (d_out [rows] float32, {'likelihood', 'power', 'total'} float32 device scalars); only
    enqueues."""
    kw = dict(out=_ptr(pred), y=_ptr(y), win_length=int(hp.signal.win_length), hop_length=int(hp.signal.hop_length), weight_l1=1.0,
              weight_power=float(w))
    if isinstance(shape, tuple):
        (n, T), name = shape, 'pwv_train_loss'
        rows, a = n * T, _lib.TrainLossArgs(n=n, T=T, **kw)
    else:
        n, rows, name = shape.n, shape.rows, 'pwv_train_loss_varlen'
        a = _lib.TrainLossVarlenArgs(cu_rows=_ptr(shape.cu_rows), n=n, rows=rows, **kw)
    need = int(getattr(_lib.lib(), name + '_workspace_bytes')(ctypes.byref(a)))
    if not need:
        _lib.check(-1, name + '_workspace_bytes')
    d_out = torch.empty(rows, dtype=torch.float32, device=pred.device)
    table = torch.empty((n, 4), dtype=torch.float64, device=pred.device)
    work = torch.empty(need // 8, dtype=torch.float64, device=pred.device)
    a.d_out, a.result, a.workspace, a.workspace_bytes = _ptr(d_out), _ptr(table), _ptr(work), need
    _call(name + '_f32', a)
    sums = table.sum(dim=0)                                              # {abs_sum, samples, power_sum, terms} of the batch
    likelihood = sums[0] / sums[1]
    power = sums[2] / sums[3] if w > 0 else torch.zeros_like(likelihood)       # (weight 0: no frame is formed, terms = 0)
    total = likelihood + float(w) * power
    return d_out, {'likelihood': likelihood.to(torch.float32), 'power': power.to(torch.float32), 'total': total.to(torch.float32)}


def _head(shape, rows, power_weight, terms):
    """head(pred, y) -> (loss, d_out [rows]) of _forward_backward: the L1 in torch (power_weight None) or _loss_head on `shape`."""
    def head(x, y):
        if power_weight is None:
            diff = x - y
            return diff.abs().mean(), torch.sign(diff) / float(rows)
        d_out, parts = _loss_head(x.contiguous(), y.contiguous(), shape, float(power_weight))
        if terms is not None:
            terms.update(parts)
        return parts['total'], d_out
    return head


def loss_and_grad(model, wav, melspec, z=None, seed=None, max_workgroups: int = 0, power_weight: Optional[float] = None,
                  terms: Optional[dict] = None, use_skip_connection: Optional[bool] = None, *, shared_nets: Optional[bool] = None):
    """(loss, pred, grads) of one batch: `loss` the L1 mean |pred - wav| as a device scalar (models.py:93 `loss/likelihood`), `pred`
    [N, T, 1] the model's output, `grads` {name: device tensor of the variable's shape} for EVERY trainable variable of the store under
    'iaf_vocoder' -- exact zeros for the ones the model never reads (skip / skip_bias of every layer but the last, dense / dense_bias of
    the last).  wav [N, T] or [N, T, 1], melspec [N, 1 + T / hop, n_mels], both on the GPU; z [N, T, 1] replaces the logistic noise the
    forward draws (`seed`: as IAFVocoder.sample_noise).  Only enqueues; `max_workgroups` (0: two per compute unit) sets the number of
    partials of every weight-gradient reduction.

    `power_weight` = w >= 0 asks for the reference's whole cost, likelihood + w * power (models.py:95-99; hp.train.weight_power_loss is
    not consulted): the loss head is then one pwv_train_loss_f32 (include/pwv_hip_train_loss.h) with hp.signal.win_length / hop_length,
    `loss` is the total as a float32 device scalar, and `terms`, if a dict is passed, receives the device scalars 'likelihood', 'power'
    and 'total'.  None: the L1 alone, and hparams with train.weight_power_loss > 0 are refused.

    `use_skip_connection` = True asks for the skip-connection architecture (hparams with model.use_skip_connection; the kernels of
    include/pwv_hip_train_skip.h): the head of every net reads the sum of all layers' skip outputs, every layer's skip / skip_bias has a
    gradient and the exact zeros are the last layer's dense / dense_bias.  None: the default architecture, launch for launch what it
    was, and hparams with model.use_skip_connection are refused.

    `shared_nets` = True asks for the shared-net architecture (hparams with model.shared_nets; the two-output head of
    include/pwv_hip_train_shared.h): each flow has ONE net whose head leaves the scale and the shift plane, one backward per flow, and
    the variables are 'iaf_vocoder/iafK/shared/...'.  It combines with use_skip_connection=True, the power loss, packed batches and
    transposed-conv conditioning.  None: two nets per flow, and hparams with model.shared_nets are refused."""
    from . import engine
    why = refusal(model, wav, melspec, power_weight=power_weight, use_skip_connection=use_skip_connection, shared_nets=shared_nets)
    if why:
        raise PwvError('training refused: ' + why)
    store = model.store or get_default_store()
    melspec = engine._require_cuda_f32(melspec, 'melspec')
    wav = engine._require_cuda_f32(wav, 'wav')
    N, t_mel, n_mels = melspec.shape
    T, hop = model.length, hp.signal.hop_length
    if n_mels != hp.signal.n_mels or T % hop or hop % 2 or t_mel != 1 + T // hop:
        raise ValueError('melspec must be [N, 1 + %d / %d, %d] with an even hop that divides the length, got %s' % (T, hop, hp.signal.n_mels, tuple(melspec.shape)))
    if wav.numel() != N * T:
        raise ValueError('wav must be [%d, %d] or [%d, %d, 1], got %s' % (N, T, N, T, tuple(wav.shape)))
    dev = melspec.device
    if z is None:
        noise = model.sample_noise(N, dev, seed=seed)
    else:
        noise = engine._require_cuda_f32(z, 'z')
        if noise.numel() != N * T:
            raise ValueError('z must be [%d, %d, 1], got %s' % (N, T, tuple(noise.shape)))
    flows = model_nets(model, store)
    cols = sum(128 * len(net.dilations) for pair in flows for net in pair)
    if hp.model.cond_upsample_method == 'transposed_conv':      # no frames, no P: nothing there is at frame rate
        batch, cond, cols = _Uniform(N, T, 0), _PerSample(int(hp.model.condition_channels)), 0
    else:
        batch, cond = _Uniform(N, T, t_mel), _Projected()
    geo = _Geometry(batch, cond, cols, int(max_workgroups), skip=bool(use_skip_connection), shared=bool(shared_nets))

    loss, x, grads = _forward_backward(store, flows, geo, melspec.reshape(N * t_mel, n_mels), noise.reshape(N * T).contiguous(),
                                       wav.reshape(N * T), _head((N, T), N * T, power_weight, terms))
    return loss, x.reshape(N, T, 1), grads


def _tconv_forward(store, mel2, C):
    """The three transposed convolutions of models.py:109-124 on the frames `mel2` [M, n_mels], kernel width == stride:
    out[t s + j, co] = sum_ci in[t, ci] w[0, j, co, ci], a GEMM on the re-laid-out [Cin, s C] weight, + ReLU (as models._condition runs
    them, on the project's row-independent exact-fp32 GEMM).  Returns [(input [rows, Cin], weight [Cin, s C], output [rows, s C])] per
    stage, kept for the backward; the last output, seen as [M * 80, C], is the uncropped condition."""
    from . import engine
    stages, cur = [], mel2
    for w, stride in zip(cond_tconv(store), TCONV_STRIDES):
        wmat = w[0].permute(2, 0, 1).reshape(w.shape[3], stride * C).contiguous()
        out = engine.linear_op(cur, wmat, None, True, 'f32')
        stages.append((cur, wmat, out))
        cur = out.reshape(-1, C)
    return stages


def _tconv_backward(stages, d_cond, grads):
    """d_cond (the shape of the uncropped condition; zero margins: the crop's adjoint) back through the stages, in torch: per stage
    d_pre = d_out * (out > 0), dW = in^T d_pre -- into `grads` in the TF layout [1, s, C, Cin] --, d_in = d_pre Wmat^T."""
    C = d_cond.shape[-1]
    d = d_cond.reshape(-1, C)
    for i in range(len(stages) - 1, -1, -1):
        cur, wmat, out = stages[i]
        d_pre = d.reshape(out.shape) * (out > 0).to(torch.float32)
        dw = cur.t() @ d_pre                                                                                             # [Cin, s C]
        grads[SCOPE + '/cond/transposed_conv_%d_weights' % i] = dw.reshape(wmat.shape[0], TCONV_STRIDES[i], C).permute(1, 2, 0).unsqueeze(0).contiguous()
        if i > 0:
            d = d_pre @ wmat.t()


def _forward_backward(store, flows, geo, mel2, x, y, head):
    """What a uniform and a packed batch share: `mel2` [M, n_mels] the frames of the batch row after row, `x` [rows] the noise, `y`
    [rows] the ground truth, `geo` the geometry of the kernels' calls, `head(pred, y)` -> (loss, d_out [rows]).  Returns (loss, pred
    [rows], grads)."""
    dev = mel2.device
    nets = [net for pair in flows for net in pair]
    cols = geo.cols
    per_sample = geo.cond.per_sample

    # frame rate, forward: frames = relu(mel dense); P = frames [gc_filter | gc_gate] + [filter_bias | gate_bias] for every net-layer.
    # Both products run on the project's exact-fp32 GEMM (pwv_linear_f32), whose sum over K has one order whatever the number of rows:
    # a row of P, and with it an utterance's prediction, does not depend on what else is in the batch.  (A BLAS picks its kernel, and
    # the order of that sum, by the row count.)
    from . import engine
    zeros64 = torch.zeros(64, dtype=torch.float32, device=dev)
    mel2 = mel2.contiguous()
    if per_sample:
        stages = _tconv_forward(store, mel2, geo.cond.C)
        geo.cond.set(stages[-1][2].reshape(geo.N, geo.T + geo.hop, geo.cond.C))          # uncropped: the kernels skip hop / 2 rows themselves
    else:
        dense = cond_dense(store)
        frames = engine.linear_op(mel2, dense[0].contiguous(), None, True, 'f32')
        bank_w = torch.cat([v[k][0] for net in nets for v in net.layers for k in ('gc_filter', 'gc_gate')], dim=1)          # [C, cols]
        bank_b = torch.cat([v.get(k, zeros64) for net in nets for v in net.layers for k in ('filter_bias', 'gate_bias')])
        geo.cond.P = engine.linear_op(frames, bank_w, bank_b, False, 'f32')                                                     # [M, cols]

    # sample rate, forward
    assert all(len(pair) == (1 if geo.shared else 2) for pair in flows)
    ws = geo.workspace(dev)
    saved = []
    for pair in flows:
        s = [_net_forward(net, geo, x) for net in pair]
        saved.append((x, s))
        if geo.shared:
            x = x * s[0][2][0] + s[0][2][1]                                             # SharedIAFLayer: out = x y[..., 0] + y[..., 1]
        else:
            x = x * s[0][2] + s[1][2]                                                   # modules.py:59
    loss, d_out = head(x, y)

    # sample rate, backward
    grads: Dict[str, torch.Tensor] = {}
    M = mel2.shape[0]
    # K slots per P row (include/pwv_hip_train.h); a per-sample condition has no P: its layers add to geo.cond.d_cond instead
    dP = None if per_sample else torch.zeros((M * geo.kmax, cols), dtype=torch.float32, device=dev)
    for i in range(len(flows) - 1, -1, -1):
        xin, s = saved[i]
        d_in = torch.empty_like(xin) if i > 0 else None
        if geo.shared:                      # one net: the head forms ds = d out * in and db = d out itself
            _net_backward(flows[i][0], geo, s[0], xin, d_out, xin, s[0][2][0], d_in, False, dP, ws, grads)
            d_out = d_in
            continue
        _net_backward(flows[i][0], geo, s[0], xin, d_out, xin, s[0][2], d_in, False, dP, ws, grads)       # ds = d out * in
        _net_backward(flows[i][1], geo, s[1], xin, d_out, None, None, d_in, True, dP, ws, grads)          # db = d out
        d_out = d_in

    if per_sample:       # (the gradients of gc_* and of the biases came straight from the kernels)
        _tconv_backward(stages, geo.cond.d_cond, grads)
        return _fill_unread(store, grads, loss, x)

    # frame rate, backward
    dPs = dP.reshape(M, geo.kmax, cols).sum(dim=1)
    d_bank_w = frames.t() @ dPs                                                                                          # [C, cols]
    d_bank_b = dPs.sum(dim=0)
    d_pre = (dPs @ bank_w.t()) * (frames > 0).to(torch.float32)
    grads[SCOPE + '/cond/dense'] = (mel2.t() @ d_pre).unsqueeze(0)
    C = bank_w.shape[0]
    gw = d_bank_w.reshape(C, cols // 64, 64).permute(1, 0, 2).contiguous()                                               # [2 per net-layer, C, 64]
    gb = d_bank_b.reshape(cols // 64, 64)
    i = 0
    for net in nets:
        for j, v in enumerate(net.layers):
            grads[net.name(j, 'gc_filter')], grads[net.name(j, 'gc_gate')] = gw[i:i + 1], gw[i + 1:i + 2]
            if 'filter_bias' in v:
                grads[net.name(j, 'filter_bias')], grads[net.name(j, 'gate_bias')] = gb[i], gb[i + 1]
            i += 2
    return _fill_unread(store, grads, loss, x)


class _Grads(dict):
    """The gradients of a step by name; `unread`: the names whose entries are the zeros of variables the model never reads."""
    unread = ()


def _fill_unread(store, grads, loss, x):
    grads = _Grads(grads)
    grads.unread = tuple(name for name in trainable_names(store) if name not in grads)       # what the model never reads
    for name in grads.unread:
        grads[name] = torch.zeros_like(store.vars[name])
    return loss, x, grads


# ---- packed batches: utterances of different lengths, unpadded ("Packed training") ------------------------------
def loss_and_grad_varlen(model, wavs, mels, z=None, seeds=None, max_workgroups: int = 0, power_weight: Optional[float] = None,
                         terms: Optional[dict] = None, use_skip_connection: Optional[bool] = None, *,
                         shared_nets: Optional[bool] = None):
    """loss_and_grad over utterances of DIFFERENT lengths in one packed batch, without padding: (loss, preds, grads).  wavs[i] is [T_i] or
    [T_i, 1] and mels[i] [1 + T_i / hop, n_mels], both on the GPU, T_i >= hop a multiple of hop.  `loss` = sum |pred - wav| / sum T_i
    (with `power_weight` = w: + w * power, the STFT power loss over the frames of all utterances that are at least win_length long --
    pwv_train_loss_varlen_f32; `terms` as for loss_and_grad); `preds` a list of [T_i, 1] views of one packed result; `grads` the dict of
    loss_and_grad, exact zeros for unread variables included.  `seeds` (one integer per utterance) gives every utterance a noise stream
    of its own, as IAFVocoder.generate_varlen does; `z`, a list of [T_i, 1] (or [T_i]), replaces the noise; with neither, one draw of
    sum T_i counters continues the model's stream.  The constructor's batch_size and length are not used.  Only enqueues: the kernels
    read the lengths from device tables (include/pwv_hip_train_varlen.h).  `use_skip_connection`, `shared_nets`: as for loss_and_grad."""
    from . import engine
    from .models import noise_streams
    why = refusal(model, power_weight=power_weight, packed=True, use_skip_connection=use_skip_connection, shared_nets=shared_nets)
    if why:
        raise PwvError('training refused: ' + why)
    if not isinstance(wavs, (list, tuple)) or not isinstance(mels, (list, tuple)) or not wavs:
        raise ValueError('wavs and mels must be non-empty lists of tensors, one entry per utterance')
    if len(wavs) != len(mels):
        raise ValueError('wavs holds %d utterances, mels %d' % (len(wavs), len(mels)))
    n, hop = len(wavs), int(hp.signal.hop_length)
    if hop % 2:
        raise ValueError('hop_length %d must be even' % hop)
    lengths = []
    for i, (w, m) in enumerate(zip(wavs, mels)):
        T = int(w.numel())
        if getattr(w, 'dim', lambda: 0)() not in (1, 2) or (w.dim() == 2 and w.shape[1] != 1):
            raise ValueError('wavs[%d] must be [T] or [T, 1], got %s' % (i, tuple(w.shape)))
        if T < hop or T % hop:
            raise ValueError('wavs[%d]: utterance %d has %d samples, not a multiple of hop_length %d (at least one hop)' % (i, i, T, hop))
        if m.dim() != 2 or m.shape[1] != hp.signal.n_mels or m.shape[0] != 1 + T // hop:
            raise ValueError('mels[%d]: utterance %d of %d samples needs a mel of [%d, %d], got %s'
                             % (i, i, T, 1 + T // hop, hp.signal.n_mels, tuple(m.shape)))
        lengths.append(T)
    if power_weight is not None and float(power_weight) > 0 and max(lengths) < int(hp.signal.win_length):
        raise PwvError('training refused: power_weight %g > 0 with no utterance as long as signal.win_length %d (the longest has %d samples): '
                       'the STFT power loss has no frame' % (float(power_weight), int(hp.signal.win_length), max(lengths)))
    streams = noise_streams(seeds, None, n, z)
    if z is not None:
        if not isinstance(z, (list, tuple)) or len(z) != n:
            raise ValueError('z must be a list of %d tensors, one [T_i, 1] per utterance' % n)
        for i, v in enumerate(z):
            if int(v.numel()) != lengths[i]:
                raise ValueError('z[%d] must be [%d, 1] (utterance %d), got %s' % (i, lengths[i], i, tuple(v.shape)))
    store = model.store or get_default_store()
    mels = [engine._require_cuda_f32(m, 'mels[%d]' % i) for i, m in enumerate(mels)]
    wavs = [engine._require_cuda_f32(w, 'wavs[%d]' % i) for i, w in enumerate(wavs)]
    dev = mels[0].device
    layout = engine.VarlenGeometry(lengths, hop, dev)
    if streams is not None:
        noise = engine.logistic_noise_packed_op(layout.cu_rows, layout.stream_table(streams), layout.rows)
    elif z is None:
        noise = engine.logistic_noise_op((layout.rows, 1), dev, seed=model._seed(), offset=model.noise_offset)
        model.noise_offset += layout.rows
    else:
        noise = torch.cat([engine._require_cuda_f32(v, 'z[%d]' % i).reshape(-1) for i, v in enumerate(z)])
    flows = model_nets(model, store)
    cols = sum(128 * len(net.dilations) for pair in flows for net in pair)
    geo = _Geometry(_Packed(layout), _Projected(), cols, int(max_workgroups), skip=bool(use_skip_connection), shared=bool(shared_nets))

    loss, x, grads = _forward_backward(store, flows, geo, torch.cat(mels), noise.reshape(layout.rows).contiguous(),
                                       torch.cat([w.reshape(-1) for w in wavs]), _head(layout, layout.rows, power_weight, terms))
    packed = x.reshape(layout.rows, 1)
    return loss, [packed[a:b] for a, b in zip(layout.cu_rows_host, layout.cu_rows_host[1:])], grads


# ---- the optimiser ------------------------------------------------------------------------------------------------------------------
def adam_ema_update(vars, grads, state, lr, beta1=ADAM_BETA1, beta2=0.999, eps=ADAM_EPS, ema_decay=None):
    """One step of tf.train.AdamOptimizer on the tensors `vars` (updated in place) with `grads`, then the reference's EMA
    (models.py:72-76) of the UPDATED variables.  `state` is None at the first step, else what the last step returned:
    {'t', 'm', 'v', 'shadow'} (lists parallel to `vars`; the shadows start at the initial values; 'shadow' is None without ema_decay).
        lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t);  m <- beta1 m + (1 - beta1) g;  v <- beta2 v + (1 - beta2) g^2
        var <- var - lr_t m / (sqrt(v) + eps)                 (TensorFlow's epsilon placement, not torch's)
        shadow <- shadow - (1 - decay) (shadow - var)
    Tensors of any device and float dtype; torch._foreach ops only, no per-variable arithmetic."""
    vars, grads = list(vars), list(grads)
    if state is None:
        state = {'t': 0, 'm': [torch.zeros_like(v) for v in vars], 'v': [torch.zeros_like(v) for v in vars],
                 'shadow': [v.clone() for v in vars] if ema_decay is not None else None}
    state['t'] += 1
    t = state['t']
    lr_t = float(lr) * math.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)
    m, v = state['m'], state['v']
    torch._foreach_mul_(m, beta1)
    torch._foreach_add_(m, grads, alpha=1.0 - beta1)
    torch._foreach_mul_(v, beta2)
    torch._foreach_addcmul_(v, grads, grads, value=1.0 - beta2)
    denom = torch._foreach_sqrt(v)
    torch._foreach_add_(denom, eps)
    torch._foreach_addcdiv_(vars, m, denom, value=-lr_t)
    if ema_decay is not None:
        if state.get('shadow') is None:
            state['shadow'] = [x.clone() for x in vars]
        gap = torch._foreach_sub(state['shadow'], vars)
        torch._foreach_add_(state['shadow'], gap, alpha=-(1.0 - float(ema_decay)))
    return state


# ---- the gradient arena and the fused optimiser (include/pwv_hip_train_opt.h; DESIGN.md section 9, "Data-parallel training") ----------
class ArenaLayout(object):
    """Where every variable lies in a flat float32 arena: `names` sorted, `shapes`, `counts`, `offsets` (floats, multiples of 4) parallel
    to them, `total` floats = sum of the counts rounded up to 4."""

    def __init__(self, names, shapes, counts, offsets, total):
        self.names, self.shapes, self.counts, self.offsets, self.total = names, shapes, counts, offsets, total
        self.index = {n: i for i, n in enumerate(names)}

    def views(self, arena):
        """One view of `arena` per variable, in the variable's shape."""
        return [arena[o:o + c].view(s) for o, c, s in zip(self.offsets, self.counts, self.shapes)]


def arena_layout(names, shapes) -> ArenaLayout:
    """THE layout of the gradient, m, v and shadow arenas, a pure function of the variables' names and shapes: variables in sorted-name
    order, each at an offset that is a multiple of 4 floats (16 bytes), the up to 3 floats of padding behind a variable never written.
    `shapes`: a mapping name -> shape, or a sequence parallel to `names`."""
    names = list(names)
    if len(set(names)) != len(names):
        raise ValueError('arena_layout: a name occurs twice')
    by_name = dict(shapes) if isinstance(shapes, dict) else dict(zip(names, shapes))
    order = sorted(names)
    out_shapes = [tuple(int(d) for d in by_name[n]) for n in order]
    counts = [int(np.prod(s, dtype=np.int64)) if len(s) else 1 for s in out_shapes]
    if any(c < 1 for c in counts):
        raise ValueError('arena_layout: a variable without elements')
    offsets, at = [], 0
    for c in counts:
        offsets.append(at)
        at += (c + 3) // 4 * 4
    return ArenaLayout(order, out_shapes, counts, offsets, at)


def arena_block_map(counts) -> np.ndarray:
    """int32 [blocks, 2] = {tensor, chunk}: every chunk of _lib.TRAIN_OPT_CHUNK floats of every tensor once, tensor after tensor."""
    recs = [(i, c) for i, count in enumerate(counts) for c in range((int(count) + _lib.TRAIN_OPT_CHUNK - 1) // _lib.TRAIN_OPT_CHUNK)]
    return np.asarray(recs, dtype=np.int32).reshape(-1, 2)


def noise_offset(step: int, world: int, rank: int, N: int, T: int) -> int:
    """The first noise counter of rank `rank` at (0-based) step `step` of data-parallel training on uniform [N, T] local batches: with one
    noise_seed the ranks together draw exactly the counters that one process training the concatenated [world N, T] batch draws at that
    step -- (step world + rank) N T."""
    return (int(step) * int(world) + int(rank)) * int(N) * int(T)


def allreduce_sum_(flat, group=None, host=None):
    """SUM all-reduce of the flat tensor `flat` over `group`, in place.  A CPU tensor, or any tensor under the `nccl` backend (RCCL), is
    reduced where it is; a GPU tensor under another backend (gloo: the CPU tests, the one-GPU dry run) goes through `host`, a pinned CPU
    tensor of the same size (made here if None).  Every rank ends with the same bits.  Returns `flat`."""
    import torch.distributed as dist
    if not flat.is_cuda or dist.get_backend(group) == 'nccl':
        dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
        return flat
    return _through_host(flat, host, lambda t: dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group))


def broadcast_(flat, src=0, group=None, host=None):
    """`flat` of rank `src` to every rank, in place; the route of allreduce_sum_."""
    import torch.distributed as dist
    if not flat.is_cuda or dist.get_backend(group) == 'nccl':
        dist.broadcast(flat, src=src, group=group)
        return flat
    return _through_host(flat, host, lambda t: dist.broadcast(t, src=src, group=group))


def _through_host(flat, host, collective):
    if host is None:
        host = torch.empty(flat.numel(), dtype=flat.dtype, pin_memory=True)
    host.copy_(flat)                    # (synchronises with the stream that filled `flat`)
    collective(host)
    flat.copy_(host)
    return flat


class _Tables(object):
    """The tables of one call of include/pwv_hip_train_opt.h: n tensors at their arena offsets and the block map, on the device and on the
    host (the library reads its refusals from the host copies)."""

    def __init__(self, tensors, offsets, counts, device):
        self.tensors = tensors              # kept alive until the launch that reads their addresses is enqueued
        self.table_host = np.ascontiguousarray([[t.data_ptr(), o, c] for t, o, c in zip(tensors, offsets, counts)], dtype=np.int64)
        self.map_host = arena_block_map(counts)
        self.table, self.map = torch.from_numpy(self.table_host).to(device), torch.from_numpy(self.map_host).to(device)
        self.n, self.blocks = len(tensors), int(self.map_host.shape[0])
        self._pinned, self._turn = None, 0

    def retarget(self, tensors):
        """The same layout over other tensors of the same sizes (the gradients of the next step): only the addresses change."""
        self.tensors = tensors
        self.table_host[:, 0] = [t.data_ptr() for t in tensors]
        # an asynchronous upload from one of two pinned copies, so that a step does not wait for the device; a pinned copy is written
        # again two steps later, once the event behind its upload has passed
        if self._pinned is None:
            self._pinned = [[torch.empty(self.table_host.shape, dtype=torch.int64, pin_memory=True), None] for _ in range(2)]
        slot = self._pinned[self._turn]
        self._turn ^= 1
        if slot[1] is not None:
            slot[1].synchronize()
        slot[0].numpy()[:] = self.table_host
        self.table.copy_(slot[0], non_blocking=True)
        slot[1] = torch.cuda.Event()
        slot[1].record()
        return self

    def fields(self):
        return dict(table=self.table.data_ptr(), block_map=self.map.data_ptr(), table_host=self.table_host.ctypes.data,
                    block_map_host=self.map_host.ctypes.data, n=self.n, blocks=self.blocks)


def _arena_tensor(t, what):
    if not (t.is_cuda and t.dtype == torch.float32):
        raise PwvError('%s must be a float32 tensor on the GPU: the arena kernels have no CPU fallback' % what)
    return t if t.is_contiguous() else t.contiguous()


class _Arenas(object):
    """The four arenas of a fused trainer over the variables `vars` (parallel to the sorted `names`), and the launches over them."""

    def __init__(self, names, vars, ema):
        vars = [_arena_tensor(v, n) for n, v in zip(names, vars)]
        self.layout = arena_layout(names, [tuple(v.shape) for v in vars])
        assert self.layout.names == list(names)
        dev, total = vars[0].device, self.layout.total
        self.device = dev
        self.grad, self.m, self.v = (torch.zeros(total, dtype=torch.float32, device=dev) for _ in range(3))
        self.shadow = torch.zeros(total, dtype=torch.float32, device=dev) if ema else None
        self.vars = _Tables(vars, self.layout.offsets, self.layout.counts, dev)
        self._grad_tables = None

    def pack(self, tables, arena, unpack=False):
        a = _lib.TrainOptPackArgs(arena=arena.data_ptr(), arena_floats=arena.numel(), **tables.fields())
        _call('pwv_train_opt_unpack_f32' if unpack else 'pwv_train_opt_pack_f32', a)

    def pack_grads(self, grads):
        """The gradients the model formed into the gradient arena, one launch; the slots of `grads.unread` keep their zeros."""
        lay = self.layout
        unread = getattr(grads, 'unread', ())
        if self._grad_tables is None or self._grad_tables[0] != unread:
            skip = frozenset(unread)
            names = [n for n in lay.names if n not in skip]
            idx = [lay.index[n] for n in names]
            tensors = [_arena_tensor(grads[n], 'the gradient of ' + n) for n in names]
            tables = _Tables(tensors, [lay.offsets[i] for i in idx], [lay.counts[i] for i in idx], self.device)
            self._grad_tables = (unread, names, tables, tables.table_host[:, 2].tolist())
        else:
            _, names, tables, counts = self._grad_tables
            tensors = [_arena_tensor(grads[n], 'the gradient of ' + n) for n in names]
            tables.retarget(tensors)
        _, names, tables, counts = self._grad_tables
        if [t.numel() for t in tensors] != counts:
            raise PwvError('a gradient does not have the size of its variable')
        self.pack(tables, self.grad)

    def adam_ema(self, lr_t, beta1, beta2, eps, decay, grad_scale):
        a = _lib.TrainOptAdamArgs(grad=self.grad.data_ptr(), m=self.m.data_ptr(), v=self.v.data_ptr(), shadow=_ptr(self.shadow),
                                  arena_floats=self.grad.numel(), lr_t=lr_t, beta1=beta1, beta2=beta2, eps=eps,
                                  decay=-1.0 if decay is None else float(decay), grad_scale=grad_scale, **self.vars.fields())
        _call('pwv_train_opt_adam_ema_f32', a)


def arena_pack(tensors, layout: ArenaLayout, arena):
    """One pwv_train_opt_pack_f32 launch: `tensors` (float32, on the GPU, parallel to layout.names) into the flat `arena`."""
    _arena_copy(tensors, layout, arena, False)


def arena_unpack(tensors, layout: ArenaLayout, arena):
    """One pwv_train_opt_unpack_f32 launch: the flat `arena` into `tensors` (contiguous, float32, on the GPU, parallel to layout.names)."""
    _arena_copy(tensors, layout, arena, True)


def _arena_copy(tensors, layout, arena, unpack):
    tensors = list(tensors)
    if len(tensors) != len(layout.names) or any(t.numel() != c for t, c in zip(tensors, layout.counts)):
        raise ValueError('the tensors do not have the sizes of the layout')
    if unpack and not all(t.is_contiguous() for t in tensors):
        raise ValueError('arena_unpack writes contiguous tensors only')
    if arena.numel() < layout.total or not arena.is_contiguous():
        raise ValueError('the arena must be flat and hold the layout\'s %d floats' % layout.total)
    tensors = [_arena_tensor(t, n) for n, t in zip(layout.names, tensors)]
    tables = _Tables(tensors, layout.offsets, layout.counts, _arena_tensor(arena, 'the arena').device)
    a = _lib.TrainOptPackArgs(arena=arena.data_ptr(), arena_floats=arena.numel(), **tables.fields())
    _call('pwv_train_opt_unpack_f32' if unpack else 'pwv_train_opt_pack_f32', a)


_UNSET = object()


class Trainer(object):
    """The reference's training step (models.py:80-103) on one model: loss_and_grad, then adam_ema_update on the store's variables in
    place.  Defaults from hparams: lr = train.lr, beta2 = train.adam_beta2, ema_decay = train.ema_decay if train.use_ema.
    `power_weight` goes to every loss_and_grad; `terms` then holds the last step's 'likelihood', 'power' and 'total' (device scalars).
    `use_skip_connection` goes to every loss_and_grad too: True trains the skip-connection architecture.  So does `shared_nets`: True
    trains the shared-net architecture (one net per flow; the variables and the .npz names are 'iaf_vocoder/iafK/shared/...').

    `fused` (default False: adam_ema_update's torch._foreach passes, launch for launch what they were): the gradients of a step are
    packed into one flat arena by one launch and ONE pwv_train_opt_adam_ema_f32 launch updates the model
    (include/pwv_hip_train_opt.h); state['m' | 'v' | 'shadow'] are then views into the m, v and shadow arenas, and save / load /
    shadows() work as before -- an .npz of either path loads into the other."""

    def __init__(self, model, lr=None, beta2=None, ema_decay=_UNSET, max_workgroups: int = 0, power_weight: Optional[float] = None,
                 fused: bool = False, *, use_skip_connection: Optional[bool] = None, shared_nets: Optional[bool] = None):
        self.model = model
        self.use_skip_connection = use_skip_connection      # None: the default architecture; True: skip connections (loss_and_grad)
        self.shared_nets = shared_nets                      # None: two nets per flow; True: one shared net per flow (loss_and_grad)
        self.fused = bool(fused)
        self.arenas: Optional[_Arenas] = None
        self._vars_version = None
        self.power_weight = power_weight        # None: the L1 alone; w >= 0: likelihood + w * power (loss_and_grad)
        self.terms: Dict[str, torch.Tensor] = {}
        self.store = model.store or get_default_store()
        self.lr = float(hp.train.lr if lr is None else lr)
        self.beta1, self.beta2 = ADAM_BETA1, float(hp.train.adam_beta2 if beta2 is None else beta2)
        if ema_decay is _UNSET:
            ema_decay = hp.train.ema_decay if hp.train.use_ema else None
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.max_workgroups = max_workgroups
        self.names: Optional[List[str]] = None
        self.state = None

    def _bind(self, packed=False):
        """Every variable of the model exists from here on; the optimiser's lists follow the sorted names."""
        why = refusal(self.model, power_weight=self.power_weight, packed=packed, use_skip_connection=self.use_skip_connection,
                      shared_nets=self.shared_nets)
        if why:
            raise PwvError('training refused: ' + why)
        if self.names is None:
            model_nets(self.model, self.store)
            cond_variables(self.store)
            self.names = trainable_names(self.store)
        return [self.store.vars[n] for n in self.names]

    def step(self, wav, mel, z=None):
        """One step on one batch; returns the loss BEFORE the update (a device scalar; with a power_weight: the total)."""
        vars = self._bind()
        terms: Dict[str, torch.Tensor] = {}
        loss, _, grads = loss_and_grad(self.model, wav, mel, z=z, max_workgroups=self.max_workgroups, power_weight=self.power_weight,
                                       terms=terms, use_skip_connection=self.use_skip_connection, shared_nets=self.shared_nets)
        return self._update(vars, loss, grads, terms)

    def step_varlen(self, wavs, mels, z=None, seeds=None):
        """One step on one packed batch of utterances of different lengths (loss_and_grad_varlen: lists of [T_i] wavs and
        [1 + T_i / hop, n_mels] mels; `seeds`: one noise seed per utterance); returns the loss BEFORE the update."""
        vars = self._bind(packed=True)
        terms: Dict[str, torch.Tensor] = {}
        loss, _, grads = loss_and_grad_varlen(self.model, wavs, mels, z=z, seeds=seeds, max_workgroups=self.max_workgroups,
                                              power_weight=self.power_weight, terms=terms, use_skip_connection=self.use_skip_connection,
                                              shared_nets=self.shared_nets)
        return self._update(vars, loss, grads, terms)

    def _update(self, vars, loss, grads, terms):
        self.terms = terms
        if self.fused:
            self._fused_update(vars, grads)
        else:
            self.state = adam_ema_update(vars, [grads[n] for n in self.names], self.state, self.lr, self.beta1, self.beta2, ADAM_EPS, self.ema_decay)
        self.store.touch()
        self._vars_version = self.store.version
        return loss

    # -- the fused path: one pack launch, (a replicated trainer's all-reduce,) one Adam + EMA launch ---------------------------------
    def _arenas(self, vars) -> _Arenas:
        """The arenas over the store's variables; made at the first use, their table of addresses rebuilt if the store has changed
        behind the trainer's back (an assign replaces a variable's tensor)."""
        if self.arenas is None:
            self.arenas = _Arenas(self.names, vars, self.ema_decay is not None)
        elif self._vars_version != self.store.version:
            self.arenas.vars = _Tables([_arena_tensor(v, n) for n, v in zip(self.names, vars)], self.arenas.layout.offsets,
                                       self.arenas.layout.counts, self.arenas.device)
        self._vars_version = self.store.version
        return self.arenas

    def _fused_state(self, vars, t):
        """state whose 'm', 'v' and 'shadow' are views into the arenas."""
        ar = self._arenas(vars)
        lay = ar.layout
        return {'t': t, 'm': lay.views(ar.m), 'v': lay.views(ar.v), 'shadow': lay.views(ar.shadow) if ar.shadow is not None else None}

    def _reduce(self, arena) -> float:
        """What happens to the gradient arena between the pack and the optimiser; returns grad_scale.  One process: nothing."""
        return 1.0

    def _fused_update(self, vars, grads):
        ar = self._arenas(vars)
        if self.state is None:
            ar.m.zero_()
            ar.v.zero_()
            if ar.shadow is not None:
                ar.pack(ar.vars, ar.shadow)                  # the shadows start at the initial values
            self.state = self._fused_state(vars, 0)
        ar.pack_grads(grads)
        scale = self._reduce(ar.grad)
        self.state['t'] += 1
        t = self.state['t']
        lr_t = self.lr * math.sqrt(1.0 - self.beta2 ** t) / (1.0 - self.beta1 ** t)
        ar.adam_ema(lr_t, self.beta1, self.beta2, ADAM_EPS, self.ema_decay, scale)

    def gradients(self) -> Dict[str, torch.Tensor]:
        """A fused trainer's gradient arena by name, as the last step left it (views; in a replicated trainer: the SUM over the ranks)."""
        return {} if self.arenas is None else dict(zip(self.names, self.arenas.layout.views(self.arenas.grad)))

    @property
    def steps(self) -> int:
        return 0 if self.state is None else self.state['t']

    def shadows(self) -> Dict[str, torch.Tensor]:
        return {} if self.state is None or self.state['shadow'] is None else dict(zip(self.names, self.state['shadow']))

    def save(self, path: str) -> None:
        """An .npz under TensorFlow's names: the variables, <name>/ExponentialMovingAverage, <name>/Adam (m), <name>/Adam_1 (v),
        beta1_power and beta2_power (beta^(t + 1), as AdamOptimizer keeps them after t steps)."""
        vars = self._bind()
        out = {n: v.detach().cpu().numpy() for n, v in zip(self.names, vars)}
        t = self.steps
        if self.state is not None:
            for n, m, v in zip(self.names, self.state['m'], self.state['v']):
                out[n + '/Adam'], out[n + '/Adam_1'] = m.cpu().numpy(), v.cpu().numpy()
        if self.ema_decay is not None:
            shadows = self.shadows()
            for n, v in zip(self.names, vars):           # (before the first step a shadow is the variable itself)
                out[n + EMA_SUFFIX] = shadows.get(n, v).detach().cpu().numpy()
        out['beta1_power'] = np.float64(self.beta1 ** (t + 1))
        out['beta2_power'] = np.float64(self.beta2 ** (t + 1))
        out['global_step'] = np.int64(t)
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'wb') as f:
            np.savez(f, **out)

    def load(self, path: str) -> int:
        """Resume from a file `save` wrote (by either path, fused or not); returns the step count."""
        vars = self._bind()
        with np.load(path) as zf:
            data = {k: zf[k] for k in zf.files}
        for n in self.names:
            if n not in data:
                raise KeyError('%s has no variable %s' % (path, n))
        t = int(data['global_step']) if 'global_step' in data else int(round(math.log(float(data['beta1_power'])) / math.log(self.beta1))) - 1
        if self.fused:
            # every arena is laid out on the host and uploaded whole; the variables come out of theirs by one unpack launch
            ar = self._arenas(vars)
            lay = ar.layout

            def upload(arena, key):
                flat = np.zeros(lay.total, dtype=np.float32)
                for n, o, c in zip(lay.names, lay.offsets, lay.counts):
                    flat[o:o + c] = np.asarray(data[key(n)], dtype=np.float32).reshape(-1)
                arena.copy_(torch.from_numpy(flat))

            upload(ar.grad, lambda n: n)
            ar.pack(ar.vars, ar.grad, unpack=True)
            ar.grad.zero_()
            if t > 0:
                upload(ar.m, lambda n: n + '/Adam')
                upload(ar.v, lambda n: n + '/Adam_1')
                if ar.shadow is not None:
                    upload(ar.shadow, lambda n: n + EMA_SUFFIX if n + EMA_SUFFIX in data else n)
            self.state = self._fused_state(vars, t) if t > 0 else None
        else:
            put = lambda a, like: torch.as_tensor(np.asarray(a), dtype=like.dtype).reshape(like.shape).to(like.device)
            for n, v in zip(self.names, vars):
                v.copy_(put(data[n], v))
            if t > 0:
                self.state = {'t': t, 'm': [put(data[n + '/Adam'], v) for n, v in zip(self.names, vars)],
                              'v': [put(data[n + '/Adam_1'], v) for n, v in zip(self.names, vars)],
                              'shadow': [put(data.get(n + EMA_SUFFIX, data[n]), v) for n, v in zip(self.names, vars)] if self.ema_decay is not None else None}
            else:
                self.state = None
        self.store.touch()
        self._vars_version = self.store.version
        return t


class DataParallelTrainer(Trainer):
    """The reference's replicated trainer (train.py:66-69, tensorpack's SyncMultiGPUTrainerReplicated): one process and one replica of
    the model per GPU, a fused Trainer on every rank.  `group`: a torch.distributed process group (None: the default group, which must
    be initialised).

    When the variables are bound, rank 0's go through pack -> broadcast -> unpack, so the replicas start identical.  `step` /
    `step_varlen` take the rank's LOCAL batch; after the pack ONE all-reduce (SUM) runs over the gradient arena and the optimiser launch
    reads the sum times 1 / world, so every rank applies the same update and the replicas stay bit-identical.  That is the plain mean of
    the ranks' gradients, as tensorpack forms it: with equal local batch sizes it is the gradient of the mean loss of the global batch;
    with packed batches of unequal total length it is NOT (each rank's loss is a mean over its own samples) -- the ranks are weighted
    equally, not the samples.  The returned loss is the local one; mean_loss() all-reduces it on request.

    Under the `nccl` backend (RCCL) the collectives run on the device arena; under any other (gloo) they go through a pinned host copy.
    Before a uniform step the trainer sets model.noise_offset = noise_offset(step, world, rank, N, T): with one noise_seed on every rank
    the ranks draw the counters that one process training the concatenated batch would.  A packed step takes distinct per-utterance
    `seeds` from the caller.  save() writes on rank 0 only; load() reads on every rank."""

    def __init__(self, model, group=None, **kw):
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            raise PwvError('DataParallelTrainer needs an initialised torch.distributed process group')
        kw.pop('fused', None)
        super().__init__(model, fused=True, **kw)
        self.group = group
        self.world, self.rank = dist.get_world_size(group), dist.get_rank(group)
        self._host = None
        self._local_loss = None

    def _host_copy(self, arena):
        import torch.distributed as dist
        if arena.is_cuda and dist.get_backend(self.group) != 'nccl' and self._host is None:
            self._host = torch.empty(arena.numel(), dtype=torch.float32, pin_memory=True)
        return self._host

    def _bind(self, packed=False):
        first = self.names is None
        vars = super()._bind(packed)
        if first:
            ar = self._arenas(vars)
            ar.pack(ar.vars, ar.grad)
            broadcast_(ar.grad, 0, self.group, self._host_copy(ar.grad))
            ar.pack(ar.vars, ar.grad, unpack=True)
            ar.grad.zero_()
            self.store.touch()
            self._vars_version = self.store.version
        return vars

    def _reduce(self, arena) -> float:
        allreduce_sum_(arena, self.group, self._host_copy(arena))
        return 1.0 / self.world

    def step(self, wav, mel, z=None):
        self._bind()
        if z is None:
            self.model.noise_offset = noise_offset(self.steps, self.world, self.rank, int(mel.shape[0]), int(self.model.length))
        self._local_loss = super().step(wav, mel, z=z)
        return self._local_loss

    def step_varlen(self, wavs, mels, z=None, seeds=None):
        self._local_loss = super().step_varlen(wavs, mels, z=z, seeds=seeds)
        return self._local_loss

    def mean_loss(self):
        """The mean over the ranks of the last step's local losses (one all-reduce of a scalar); a device scalar."""
        if self._local_loss is None:
            raise PwvError('mean_loss: no step has run')
        total = self._local_loss.detach().clone().reshape(1)
        allreduce_sum_(total, self.group)
        return total[0] / self.world

    def save(self, path: str) -> None:
        self._bind()                    # (a collective the first time: every rank calls save, rank 0 writes)
        if self.rank == 0:
            super().save(path)


MAX_RANKS = 8               # the reference's largest job (hparams ema/*: num_gpu 8), one node


def _spawn_ranks(n, argv):
    """`n` fresh child processes, one rank each (`python -m pwv_amd.train` + argv under RANK / LOCAL_RANK / WORLD_SIZE and a rendezvous
    on a free local port): no process that has opened a GPU is replaced or forked.  Rank 0's output is this process's.  Returns the
    first non-zero exit code, else 0; when a rank fails the others are ended, since they would wait in a collective for ever."""
    import socket
    import subprocess
    import time
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port),
                   PYTHONPATH=root + os.pathsep + os.environ.get('PYTHONPATH', ''))
        procs.append(subprocess.Popen([sys.executable, '-m', 'pwv_amd.train'] + list(argv), env=env,
                                      stdout=None if r == 0 else subprocess.DEVNULL))
    code = 0
    try:
        live = list(procs)
        while live and code == 0:
            for p in list(live):
                rc = p.poll()
                if rc is not None:
                    live.remove(p)
                    code = code or rc
            if live and code == 0:
                time.sleep(0.05)
    finally:
        for p in procs:
            if p.poll() is None:
                p.terminate()
        for p in procs:
            try:
                p.wait(timeout=30)
            except subprocess.TimeoutExpired:
                p.kill()
                p.wait()
    return code


def _ranks_wanted(gpus) -> int:
    """How many ranks train() runs: `gpus` if given, else hp.train.num_gpu; refused beyond the visible devices and beyond MAX_RANKS.
    PWV_TRAIN_DRYRUN_ONE_GPU=1 (a test hook, like bench.py's PWV_BENCH_DRYRUN_ONE_GPU): the ranks share GPU 0 and meet over gloo."""
    n = int(gpus) if gpus is not None else int(hp.train.get('num_gpu', 1) or 1)
    if n < 1:
        raise PwvError('training refused: num_gpu %d must be >= 1' % n)
    if n > 1 and os.environ.get('PWV_TRAIN_DRYRUN_ONE_GPU') != '1':
        visible = torch.cuda.device_count()
        if n > visible:
            raise PwvError('training refused: num_gpu %d exceeds the %d visible device(s); one rank trains on one GPU' % (n, visible))
    if n > MAX_RANKS:
        raise PwvError('training refused: num_gpu %d exceeds the %d ranks of one node this trainer starts' % (n, MAX_RANKS))
    return n


# ---- train.py:25-71 on one GPU ------------------------------------------------------------------------------------------------------
def _synthetic_wavs(n_items: int, length: int, seed: int) -> np.ndarray:
    """Seeded stand-ins for a wav dataset: a few decaying harmonics over noise, |x| < 1."""
    rng = np.random.RandomState(seed)
    t = np.arange(length) / float(hp.signal.sr)
    out = np.zeros((n_items, length), dtype=np.float32)
    for i in range(n_items):
        f0 = rng.uniform(90, 300)
        x = sum(rng.uniform(0.05, 0.3) / k * np.sin(2 * np.pi * f0 * k * t + rng.uniform(0, 6.28)) for k in range(1, 6))
        out[i] = (x + 0.02 * rng.randn(length)).astype(np.float32)
    return np.clip(out, -0.99, 0.99)


def _dataset(length: int, seed: int, varlen: bool = False) -> List[np.ndarray]:
    """The training split (data_load.py:22-25: the first dataset_ratio share of the files) as trimmed wavs of at least `length` samples;
    `varlen`: as long as they are (nothing is padded; files too short for one hop or for the mel front-end's n_fft / 2 < L are left
    out), the stand-ins of seeded, differing lengths between one and four times `length`."""
    if hp.data_path == 'synthetic':
        if varlen:
            rng = np.random.RandomState(seed + 1)
            return [_synthetic_wavs(1, int(rng.randint(length, 4 * length + 1)), seed + 2 + i)[0] for i in range(8)]
        return list(_synthetic_wavs(8, 4 * length, seed))
    from .audio_frontend import fix_length, read_wav, trim_wav
    files = sorted(glob.glob(hp.data_path))
    if not files:
        raise FileNotFoundError('no input files match data_path %r (use data_path: synthetic for seeded stand-ins)' % hp.data_path)
    files = files[:max(int(len(files) * hp.train.dataset_ratio), 1)]
    wavs = [trim_wav(read_wav(f, hp.signal.sr)).astype(np.float32) for f in files]
    if varlen:
        hop = int(hp.signal.hop_length)
        wavs = [w for w in wavs if len(w) >= hop and len(w) // hop * hop > int(hp.signal.n_fft) // 2]
        if not wavs:
            raise ValueError('no file of data_path %r is long enough (one hop of %d samples, more than n_fft / 2 = %d)'
                             % (hp.data_path, hop, int(hp.signal.n_fft) // 2))
        return wavs
    return [fix_length(w, length) if len(w) < length else w for w in wavs]


def train(case='default', ckpt=None, steps=None, seed=0, varlen=False, gpus=None):
    """train.py:25-71: per step a seeded random crop of hp.signal.length samples per item (data_load.py:46-50), its mel from
    the device front-end, one Trainer.step; prints loss/likelihood per step (with train.weight_power_loss > 0 the power loss is trained
    too, and the line carries loss/likelihood, loss/power and loss/total); saves into hp.logdir (PWV_LOGDIR overrides) every
    train.save_per_epoch * train.steps_per_epoch steps and at the end.  `ckpt` names a file in the log directory to resume from (default:
    the newest .npz there).  `varlen` (--varlen): every step trains ONE PACKED BATCH of batch_size files at their own lengths -- each cut
    to a whole number of hops and to at most train.varlen_max_length samples (default 4 * signal.length; a longer file is cut at a seeded
    offset), nothing padded (Trainer.step_varlen).

    Data-parallel (train.py:66-69): `gpus` (--gpus N), else hp.train.num_gpu, ranks -- at most 8, never more than the visible devices.
    Under a launcher (WORLD_SIZE set) this process is one rank and joins the group; otherwise N > 1 starts N fresh child processes, one
    per GPU.  Every rank runs a DataParallelTrainer on its own batch of train.batch_size items (batch_size is per rank, as with
    tensorpack's towers), its crops drawn from RandomState([seed, step base, rank]); rank 0 prints its local loss and saves."""
    hp.set_hparam_yaml(case)
    power_weight = float(hp.train.get('weight_power_loss', 0) or 0)
    power_weight = power_weight if power_weight > 0 else None
    use_skip = True if hp.model.use_skip_connection else None       # the case's architecture is what the loop asks for
    shared = True if hp.model.get('shared_nets') else None
    why = refusal(power_weight=power_weight, use_skip_connection=use_skip, shared_nets=shared)
    if why:
        raise PwvError('training refused: ' + why)
    launched = 'WORLD_SIZE' in os.environ
    world = int(os.environ['WORLD_SIZE']) if launched else _ranks_wanted(gpus)
    if not launched and world > 1:
        argv = [str(case), '--steps=%d' % int(steps)] if steps is not None else [str(case)]
        argv += ['--seed=%d' % int(seed)] + (['--ckpt=%s' % ckpt] if ckpt else []) + (['--varlen'] if varlen and varlen != 'False' else [])
        code = _spawn_ranks(world, argv)
        if code:
            raise PwvError('data-parallel training failed: a rank exited with status %d' % code)
        logdir = os.environ.get('PWV_LOGDIR', hp.logdir)
        return (sorted(glob.glob(os.path.join(logdir, '*.npz')), key=os.path.getmtime) or [None])[-1]
    if not torch.cuda.is_available():
        raise RuntimeError('train() needs an MI355X: the HIP path has no CPU fallback')
    rank = int(os.environ.get('RANK', '0')) if launched else 0
    if world > 1:
        import torch.distributed as dist
        one_gpu = os.environ.get('PWV_TRAIN_DRYRUN_ONE_GPU') == '1'
        torch.cuda.set_device(0 if one_gpu else int(os.environ.get('LOCAL_RANK', rank)))
    device = torch.device('cuda', torch.cuda.current_device())
    if world > 1:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        if one_gpu:
            dist.init_process_group(backend='gloo')
        else:
            dist.init_process_group(backend='nccl', device_id=device)       # 'nccl' is RCCL on ROCm
    try:
        return _train_rank(power_weight, device, seed, steps, ckpt, varlen, world, rank, use_skip, shared)
    finally:
        if world > 1:
            dist.destroy_process_group()


def _train_rank(power_weight, device, seed, steps, ckpt, varlen, world, rank, use_skip=None, shared=None):
    """The loop of train() in one process: the only rank, or one of `world`."""
    from .audio_frontend import wav_to_mel_device
    from .models import IAFVocoder
    from .variables import reset_default_store
    say = print if rank == 0 else (lambda *a: None)
    logdir = os.environ.get('PWV_LOGDIR', hp.logdir)
    seed = int(seed)
    length, batch = int(hp.signal.length), int(hp.train.batch_size)
    steps = int(steps) if steps is not None else int(hp.train.num_epochs) * int(hp.train.steps_per_epoch)
    store = reset_default_store(device=device)
    model = IAFVocoder(batch_size=batch, length=length, store=store, precision='f32')
    model.noise_seed = seed
    kw = dict(power_weight=power_weight, use_skip_connection=use_skip, shared_nets=shared)
    trainer = DataParallelTrainer(model, **kw) if world > 1 else Trainer(model, **kw)
    path = os.path.join(logdir, ckpt) if ckpt else (sorted(glob.glob(os.path.join(logdir, '*.npz')), key=os.path.getmtime) or [None])[-1]
    if path and os.path.exists(path):
        say('resumed from %s at step %d' % (path, trainer.load(path)))
    varlen = bool(varlen) and varlen != 'False'
    wavs = _dataset(length, seed, varlen)
    hop = int(hp.signal.hop_length)
    max_len = max(int(hp.train.get('varlen_max_length', 0) or 4 * length) // hop * hop, hop)
    rng = np.random.RandomState([seed, trainer.steps, rank]) if world > 1 else np.random.RandomState(seed + trainer.steps)
    every = max(int(hp.train.save_per_epoch) * int(hp.train.steps_per_epoch), 1)
    saved_at = None
    for _ in range(steps):
        if varlen:
            pieces = []
            for b in range(batch):
                w = wavs[rng.randint(len(wavs))]
                n = min(len(w) // hop * hop, max_len)
                at = rng.randint(len(w) - n + 1)
                pieces.append(torch.from_numpy(np.ascontiguousarray(w[at:at + n])).to(device))
            # (replicas: one distinct noise seed per utterance of the job, drawn from the rank's own stream)
            seeds = [int(rng.randint(1 << 31)) * MAX_RANKS + rank for _ in pieces] if world > 1 else None
            loss = trainer.step_varlen(pieces, [wav_to_mel_device(p.unsqueeze(0))[0] for p in pieces], seeds=seeds)
        else:
            crop = np.empty((batch, length), dtype=np.float32)
            for b in range(batch):
                w = wavs[rng.randint(len(wavs))]
                at = rng.randint(len(w) - length + 1)
                crop[b] = w[at:at + length]
            wav = torch.from_numpy(crop).to(device)
            loss = trainer.step(wav, wav_to_mel_device(wav))
        if rank != 0:
            pass
        elif power_weight is None:
            print('step %d loss/likelihood %.6f' % (trainer.steps, float(loss)))
        else:
            print('step %d loss/likelihood %.6f loss/power %.6f loss/total %.6f'
                  % (trainer.steps, float(trainer.terms['likelihood']), float(trainer.terms['power']), float(loss)))
        if trainer.steps % every == 0:
            saved_at = os.path.join(logdir, 'model-%d.npz' % trainer.steps)
            trainer.save(saved_at)
    final = os.path.join(logdir, 'model-%d.npz' % trainer.steps)
    if saved_at != final:
        trainer.save(final)
    say('saved %s' % final)
    return final


if __name__ == '__main__':
    from .generate import _fire
    _fire(train, sys.argv[1:])
