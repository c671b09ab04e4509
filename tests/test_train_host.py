"""CPU: training (pwv_amd/train.py, include/pwv_hip_train.h, csrc/pwv_train.hip) -- the float64 yardstick of the GPU tests against finite
differences, TensorFlow's Adam + the EMA against a numpy restatement, the checkpoint round trip, the refusals, the C struct and the
kernels' resources.  Nothing here needs a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import train_oracle as TO
from tests.util import kernel_resources, set_hparams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_float64_gradient_agrees_with_finite_differences():
    """Three random entries of each of five variables, central differences in float64 with h = 1e-6: the loss is piecewise smooth (ReLU,
    |.|) with curvature O(1), so the difference quotient is within h^2 + eps / h ~ 1e-9 of the derivative unless a kink lies inside
    the step; the bar, 1e-6 of the variable's largest gradient entry + 1e-9, is three orders above that and far below any wrong term."""
    cfg, w, mel, z, wav = TO.problem()
    g64 = TO.reference()['g64']
    names = ['iaf_vocoder/iaf0/scalar/dilated_stack/layer2/filter', 'iaf_vocoder/iaf1/shifter/dilated_stack/layer1/gc_gate',
             'iaf_vocoder/cond/dense', 'iaf_vocoder/iaf1/scalar/causal_layer/filter', 'iaf_vocoder/iaf0/shifter/postprocessing/postprocess1']
    rng = np.random.RandomState(0)
    h = 1e-6
    for name in names:
        base = w[name].astype(np.float64)
        for _ in range(3):
            idx = tuple(rng.randint(s) for s in base.shape)
            vals = []
            for sgn in (1, -1):
                W = dict(w)
                W[name] = base.copy()
                W[name][idx] += sgn * h
                vals.append(TO.loss_only(W, mel, z, wav, cfg))
            fd = (vals[0] - vals[1]) / (2 * h)
            assert abs(fd - g64[name][idx]) <= 1e-6 * np.abs(g64[name]).max() + 1e-9, (name, idx, fd, g64[name][idx])


def test_yardstick_counts():
    """149 variables with a gradient, 32 without: skip / skip_bias of every layer but the last, dense / dense_bias of the last."""
    g64 = TO.reference()['g64']
    none = sorted(k for k, v in g64.items() if v is None)
    assert len(g64) - len(none) == 149 and len(none) == 32
    assert all(re.search(r'layer[0-2]/skip(_bias)?$|layer3/dense(_bias)?$', k) for k in none)
    assert TO.reference()['E32'] < 1e-5


@pytest.mark.parametrize('dtype, tol', [(torch.float64, 1e-13), (torch.float32, 2e-6)])
def test_adam_ema_update_matches_numpy(dtype, tol):
    """Three steps on CPU tensors against the formulas in numpy float64 (tolerance: float64 round-off over three steps / a few float32
    ulps of O(1) variables); t, m, v and the shadows move."""
    from pwv_amd.train import adam_ema_update
    rng = np.random.RandomState(1)
    shapes = [(2, 64, 64), (64,), (1, 80, 64)]
    W = {i: rng.randn(*s) for i, s in enumerate(shapes)}
    if dtype == torch.float32:
        W = {i: a.astype(np.float32).astype(np.float64) for i, a in W.items()}
    m = {i: np.zeros_like(a) for i, a in W.items()}
    v = {i: np.zeros_like(a) for i, a in W.items()}
    sh = {i: a.copy() for i, a in W.items()}
    vars = [torch.from_numpy(W[i].copy()).to(dtype) for i in W]
    first = [x.clone() for x in vars]
    state = None
    for t in range(1, 4):
        grads = {i: rng.randn(*s) * 10.0 ** rng.randint(-4, 1) for i, s in enumerate(shapes)}
        if dtype == torch.float32:
            grads = {i: a.astype(np.float32).astype(np.float64) for i, a in grads.items()}
        TO.adam_ema_numpy(W, m, v, sh, grads, t, lr=1e-3, beta2=0.99, decay=0.9)
        state = adam_ema_update(vars, [torch.from_numpy(grads[i]).to(dtype) for i in grads], state, 1e-3, 0.9, 0.99, 1e-8, 0.9)
        assert state['t'] == t
    for i in W:
        assert np.abs(vars[i].double().numpy() - W[i]).max() <= tol
        assert np.abs(state['shadow'][i].double().numpy() - sh[i]).max() <= tol
        assert np.abs(state['m'][i].double().numpy() - m[i]).max() <= tol * 10 and np.abs(state['v'][i].double().numpy() - v[i]).max() <= tol * 100
        assert not torch.equal(vars[i], first[i]) and not torch.equal(state['shadow'][i], first[i]) and not torch.equal(state['shadow'][i], vars[i])
        assert float(state['m'][i].abs().max()) > 0 and float(state['v'][i].abs().max()) > 0
    no_ema = adam_ema_update([first[1].clone()], [torch.ones(64, dtype=dtype)], None, 1e-3)
    assert no_ema['shadow'] is None and no_ema['t'] == 1


def _cpu_trainer(tmp_path, steps=2):
    """A Trainer over a CPU store of the small model whose optimiser state comes from adam_ema_update on seeded stand-in gradients (the
    kernels need a GPU; the optimiser, the store and the checkpoint do not)."""
    from pwv_amd import train as TR
    from pwv_amd.models import IAFVocoder
    from pwv_amd.variables import VariableStore
    cfg, w, _, _, _ = TO.problem()
    set_hparams(cfg)
    store = VariableStore(device='cpu')
    store.load_dict(w)
    tr = TR.Trainer(IAFVocoder(TO.N, TO.T, store=store, precision='f32'), lr=1e-2, ema_decay=0.5)
    vars = tr._bind()
    rng = np.random.RandomState(2)
    for _ in range(steps):
        grads = [torch.from_numpy(rng.randn(*v.shape).astype(np.float32)) for v in vars]
        tr.state = TR.adam_ema_update(vars, grads, tr.state, tr.lr, tr.beta1, tr.beta2, TR.ADAM_EPS, tr.ema_decay)
        store.touch()
    return tr, store, w


def test_save_round_trips_the_shadows_and_ignores_the_adam_slots(tmp_path):
    from pwv_amd import train as TR
    from pwv_amd.models import IAFVocoder
    from pwv_amd.variables import VariableStore
    tr, store, w = _cpu_trainer(tmp_path)
    version = store.version
    store.touch()
    assert store.version == version + 1
    assert sorted(tr.names) == sorted(w)                    # every variable of the oracle's list, and nothing else, is trained
    path = str(tmp_path / 'model-2.npz')
    tr.save(path)
    with np.load(path) as z:
        keys = set(z.files)
        assert float(z['beta1_power']) == pytest.approx(0.9 ** 3) and float(z['beta2_power']) == pytest.approx(tr.beta2 ** 3)
    for n in tr.names:
        assert {n, n + '/ExponentialMovingAverage', n + '/Adam', n + '/Adam_1'} <= keys
    shadows = tr.shadows()
    for use_ema in (True, False):
        fresh = VariableStore(device='cpu')
        assert fresh.load_checkpoint(path, use_ema=use_ema) == len(tr.names)
        assert sorted(fresh.vars) == sorted(tr.names)       # no <name>/Adam, beta1_power, ... became a variable
        for n in tr.names:
            want = shadows[n] if use_ema else store.vars[n]
            assert torch.equal(fresh.vars[n], want), n
        assert not fresh.ema_missing()
    n0 = tr.names[0]
    assert not torch.equal(shadows[n0], store.vars[n0])
    # resume: the state comes back bit for bit
    cfg = TO.problem()[0]
    set_hparams(cfg)
    store2 = VariableStore(device='cpu')
    store2.load_dict(w)
    tr2 = TR.Trainer(IAFVocoder(TO.N, TO.T, store=store2, precision='f32'), lr=1e-2, ema_decay=0.5)
    assert tr2.load(path) == 2 and tr2.steps == 2
    for key in ('m', 'v', 'shadow'):
        assert all(torch.equal(a, b) for a, b in zip(tr.state[key], tr2.state[key]))
    assert all(torch.equal(store.vars[n], store2.vars[n]) for n in tr.names)


REFUSALS = [
    ('transposed', dict(cond_upsample_method='transposed_conv'), {}, 'transposed'),
    ('normalize_cond', dict(normalize_cond='bn'), {}, 'normalize_cond'),
    ('bn', dict(normalize_wavenet='bn'), {}, "'bn'"),
    ('in', dict(normalize_wavenet='in'), {}, "'in'"),
    ('flow_norm', dict(normalize='bn'), {}, 'normalize'),
    ('skip', dict(use_skip_connection=True), {}, 'skip accumulation'),
    ('shared', dict(shared_nets=True), {}, 'shared'),
    ('shape', dict(residual_channels=32), {}, 'fused shape'),
    ('width', dict(filter_width=3), {}, 'fused shape'),
    ('f16x3', {}, dict(precision='f16x3'), 'f16x3'),
    ('f16', {}, dict(precision='f16'), "'f16'"),
    ('packed', {}, dict(packed=True), 'packed'),
    ('streaming', {}, dict(streaming=True), 'streaming'),
    ('power', {}, dict(power=0.0005), 'weight_power_loss'),
]


@pytest.mark.parametrize('case', REFUSALS, ids=[c[0] for c in REFUSALS])
def test_loss_and_grad_refuses_what_is_out_of_scope(case):
    """Each configuration outside the scope is refused with a PwvError that names it, before a device is touched (CPU tensors)."""
    from pwv_amd import train as TR
    from pwv_amd._lib import PwvError
    from pwv_amd.hparam import hparam as hp
    from pwv_amd.models import IAFVocoder
    from pwv_amd.variables import VariableStore
    _, cfg_kw, extra, word = case
    base = TO.small_cfg()
    cfg = type(base)(dilations=base.dilations, n_iaf=2, hop_length=16, **cfg_kw)
    set_hparams(cfg)
    if 'power' in extra:
        hp.train.weight_power_loss = extra['power']
    model = IAFVocoder(TO.N, TO.T, store=VariableStore(device='cpu'), precision=extra.get('precision', 'f32'))
    wav, mel = torch.zeros(TO.N, TO.T), torch.zeros(TO.N, 1 + TO.T // 16, 80)
    if extra.get('packed'):
        wav, mel = [wav[0], wav[1, :96]], [mel[0], mel[1, :7]]
    if extra.get('streaming'):
        class Stream(object):
            def push(self, chunk):
                pass
        mel = Stream()
    with pytest.raises(PwvError, match=re.escape(word)):
        TR.loss_and_grad(model, wav, mel)
    with pytest.raises(PwvError, match='training refused'):
        TR.loss_and_grad(model, wav, mel)
    set_hparams(base)
    assert TR.refusal(IAFVocoder(TO.N, TO.T, store=VariableStore(device='cpu'))) is None


def test_train_args_layout_matches_ctypes(tmp_path):
    """The C compiler's size and offsets of pwv_train_args (gcc -std=c99 -pedantic -Werror) against the ctypes mirror; the header declares
    exactly _lib.TRAIN_SYMBOLS, the built library exports them, and pwv_hip.h keeps its version."""
    import subprocess
    from pwv_amd import _lib
    _lib.build_library()
    fields = [n for n, _ in _lib.TrainArgs._fields_]
    c_name = lambda f: 'in' if f == 'in_' else f
    probe = ['sizeof(pwv_train_args)'] + ['offsetof(pwv_train_args, %s)' % c_name(f) for f in fields] + ['(size_t)PWV_TRAIN_LAST', '(size_t)PWV_HIP_VERSION']
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "pwv_hip_train.h"\nint main(void){ printf("%s\\n", %s); return 0; }\n'
           % (' '.join(['%zu'] * len(probe)), ', '.join(probe)))
    c, exe = str(tmp_path / 't.c'), str(tmp_path / 't')
    with open(c, 'w') as f:
        f.write(src)
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Wextra', '-pedantic', '-Werror', '-I' + os.path.join(ROOT, 'include'), c, '-o', exe])
    got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    assert got == [ctypes.sizeof(_lib.TrainArgs)] + [getattr(_lib.TrainArgs, f).offset for f in fields] + [_lib.TRAIN_LAST, 301]
    assert _lib.TrainArgs().struct_size == ctypes.sizeof(_lib.TrainArgs)
    code = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'pwv_hip_train.h')).read(), flags=re.S)
    assert sorted(set(re.findall(r'\b(pwv_[a-z0-9_]+)\s*\(', code))) == sorted(_lib.TRAIN_SYMBOLS)
    taken = set(_lib.EXPORTED_SYMBOLS) | set(_lib.EXTENSION_SYMBOLS) | set(_lib.LIVE_TICK_SYMBOLS) | set(_lib.SCORE_SYMBOLS)
    assert not set(_lib.TRAIN_SYMBOLS) & taken and len(_lib.EXPORTED_SYMBOLS) == 52
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(raw, name) for name in _lib.TRAIN_SYMBOLS)
    assert os.path.join(os.path.dirname(_lib.__file__), 'csrc', 'pwv_train.hip') in _lib.CSRC


def test_train_calls_refuse_bad_arguments_on_the_host():
    """struct_size, shapes and NULL pointers are refused with PWV_EINVAL and a message that names the field, before a device is touched."""
    from pwv_amd import _lib
    lib = _lib.build_library() and ctypes.CDLL(_lib.LIB_PATH)
    lib.pwv_last_error.restype = ctypes.c_char_p
    lib.pwv_train_workspace_bytes.restype = ctypes.c_size_t

    def refused(name, a, word):
        assert getattr(lib, name)(ctypes.byref(a), None) == -1
        assert word in lib.pwv_last_error().decode(), lib.pwv_last_error()

    a = _lib.TrainArgs(N=2, T=208, dilation=1, next_dilation=1, cond_hop=16, cond_offset=8, cond_frames=14, proj_row_stride=128, d_proj_row_stride=128,
                       max_workgroups=3)
    assert lib.pwv_train_workspace_bytes(ctypes.byref(a)) == 3 * (64 * 128 + 128 + 128 * 128 + 128 + 128 + 1) * 4
    refused('pwv_train_layer_bwd_f32', a, 'NULL')
    refused('pwv_train_head_bwd_f32', a, 'NULL')
    refused('pwv_train_front_bwd_f32', a, 'NULL')
    a.struct_size -= 8
    refused('pwv_train_layer_fwd_f32', a, 'struct_size')
    assert lib.pwv_train_workspace_bytes(ctypes.byref(a)) == 0
    b = _lib.TrainArgs(N=0, T=208)
    refused('pwv_train_front_fwd_f32', b, 'N = 0')
    c = _lib.TrainArgs(N=2, T=208, dilation=0, cond_hop=16, cond_frames=14, proj_row_stride=128)
    refused('pwv_train_layer_fwd_f32', c, 'dilation')
    c.dilation, c.cond_frames = 1, 12
    refused('pwv_train_layer_fwd_f32', c, 'cond_frames')


def test_train_kernel_resources():
    """The compiler's resource remarks (gfx950 device code) for every kernel of csrc/pwv_train.hip: no scratch, no spilled register, LDS
    within the 64 KiB a workgroup may declare statically."""
    res = kernel_resources('pwv_train.hip')
    names = ' '.join(res)
    for k in ('train_front_fwd_kernel', 'train_layer_fwd_kernel', 'train_head_fwd_kernel', 'train_head_bwd_kernel', 'train_layer_bwd_kernel<true>',
              'train_layer_bwd_kernel<false>', 'train_front_bwd_kernel', 'train_reduce_kernel'):
        assert k in names, (k, names)
    for name, r in res.items():
        assert r['scratch'] == 0 and r['vgpr_spills'] == 0 and r['sgpr_spills'] == 0 and not r['dynamic_stack'], (name, r)
        assert r['lds'] <= 64 * 1024, (name, r)
