"""CPU: the loss head of training (include/pwv_hip_train_loss.h, csrc/pwv_train_loss.hip, train.loss_and_grad(power_weight=...)) -- the
gradient formula of the header against float64 autograd, the C struct against its ctypes mirror, the header's symbols, every host-side
refusal of the C call, the opt-in of train.py and the kernels' resources.  Nothing here needs a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import train_oracle as TO
from tests import train_power_oracle as PO
from tests.util import kernel_resources, set_hparams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES, case = PO.SHAPES, PO.case


@pytest.mark.parametrize('T, win, hop', SHAPES)
def test_gradient_formula_matches_float64_autograd(T, win, hop):
    """The analytic gradient of the header (direct sums in numpy float64) against float64 autograd of framing + torch.fft.rfft: 1e-12 of the
    largest entry; exact zeros where no frame covers a sample, and there are such samples where the shape was chosen for them."""
    pred, y = case(T)
    got, want = PO.power_grad_numpy(pred, y, win, hop), PO.power_grad_autograd(pred, y, win, hop, torch.float64)
    assert got.shape == want.shape == (2, T)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    F = PO.frame_count(T, win, hop)
    covered = np.zeros(T, dtype=bool)
    for f in range(F):
        covered[f * hop:f * hop + win] = True
    assert F == {(208, 48, 16): 11, (208, 48, 20): 9, (100, 16, 24): 4, (208, 64, 16): 10, (1200, 400, 80): 11, (210, 48, 20): 9}[(T, win, hop)]
    assert (got[:, ~covered] == 0).all() and (want[:, ~covered] == 0).all()
    assert (~covered).any() == ((T, win, hop) in ((210, 48, 20), (100, 16, 24)))
    if hop > win:
        assert not covered[win:hop].any()          # a gap between two frames


def test_power_loss_torch_matches_the_score_restatement():
    """The differentiable restatement gives the mean that score.score_reference's table gives (power_sum / terms over the batch)."""
    from pwv_amd.score import score_reference
    for T, win, hop in SHAPES:
        pred, y = case(T)
        t = score_reference(pred, y, win, hop)
        got = float(PO.power_loss_torch(torch.from_numpy(pred), torch.from_numpy(y), win, hop, torch.float64))
        assert abs(got - t[:, 2].sum() / t[:, 3].sum()) <= 1e-12 * got


def test_train_loss_args_layout_matches_ctypes(tmp_path):
    """The C compiler's size and offsets of pwv_train_loss_args (gcc -std=c99 -pedantic -Werror) against the ctypes mirror; the header
    declares exactly _lib.TRAIN_LOSS_SYMBOLS, disjoint from the older lists, the built library exports them, pwv_hip.h keeps its version."""
    import subprocess
    from pwv_amd import _lib
    _lib.build_library()
    fields = [n for n, _ in _lib.TrainLossArgs._fields_]
    assert fields == ['struct_size', 'out', 'y', 'n', 'T', 'win_length', 'hop_length', 'weight_l1', 'weight_power', 'd_out', 'result', 'workspace',
                      'workspace_bytes']
    probe = (['sizeof(pwv_train_loss_args)'] + ['offsetof(pwv_train_loss_args, %s)' % f for f in fields]
             + ['(size_t)PWV_SCORE_MAX_WIN', '(size_t)PWV_SCORE_TILE', '(size_t)PWV_HIP_VERSION'])
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "pwv_hip_train_loss.h"\nint main(void){ printf("%s\\n", %s); return 0; }\n'
           % (' '.join(['%zu'] * len(probe)), ', '.join(probe)))
    c, exe = str(tmp_path / 't.c'), str(tmp_path / 't')
    with open(c, 'w') as f:
        f.write(src)
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Wextra', '-pedantic', '-Werror', '-I' + os.path.join(ROOT, 'include'), c, '-o', exe])
    got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    assert got == ([ctypes.sizeof(_lib.TrainLossArgs)] + [getattr(_lib.TrainLossArgs, f).offset for f in fields]
                   + [_lib.SCORE_MAX_WIN, _lib.SCORE_TILE, 301])
    assert _lib.TrainLossArgs().struct_size == ctypes.sizeof(_lib.TrainLossArgs) and _lib.HEADER_VERSION == 301


def test_header_declares_exactly_the_new_symbols():
    from pwv_amd import _lib
    _lib.build_library()
    code = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'pwv_hip_train_loss.h')).read(), flags=re.S)
    assert sorted(set(re.findall(r'\b(pwv_[a-z0-9_]+)\s*\(', code))) == sorted(_lib.TRAIN_LOSS_SYMBOLS) \
        == ['pwv_train_loss_f32', 'pwv_train_loss_workspace_bytes']
    taken = set(_lib.EXPORTED_SYMBOLS) | set(_lib.EXTENSION_SYMBOLS) | set(_lib.LIVE_TICK_SYMBOLS) | set(_lib.SCORE_SYMBOLS) | set(_lib.TRAIN_SYMBOLS)
    assert not set(_lib.TRAIN_LOSS_SYMBOLS) & taken and len(_lib.EXPORTED_SYMBOLS) == 52 and len(_lib.TRAIN_SYMBOLS) == 7
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(raw, name) for name in _lib.TRAIN_LOSS_SYMBOLS)
    raw.pwv_version.restype = ctypes.c_int
    assert raw.pwv_version() == 301
    assert os.path.join(os.path.dirname(_lib.__file__), 'csrc', 'pwv_train_loss.hip') in _lib.CSRC
    assert '#define PWV_HIP_VERSION 301' in open(os.path.join(ROOT, 'include', 'pwv_hip.h')).read()


def _args(n=2, T=1200, win=400, hop=80, wl1=1.0, wp=0.0005):
    """A pwv_train_loss_args the library accepts up to its launch: every device pointer a number that is never dereferenced on the host."""
    from pwv_amd import _lib
    a = _lib.TrainLossArgs(n=n, T=T, win_length=win, hop_length=hop, weight_l1=wl1, weight_power=wp)
    a.out = a.y = a.d_out = a.result = a.workspace = 4096
    a.workspace_bytes = 1 << 40
    return a


def test_workspace_bytes_follow_the_layout(built_lib):
    """n F power partials + n ceil(T / TILE) L1 partials + n F win frame gradients, one double each; no frames in the L1-only modes."""
    from pwv_amd import _lib
    for n, T, win, hop, wp in ((2, 1200, 400, 80, 1.0), (2, 208, 48, 20, 0.5), (8, 4000, 400, 80, 0.0005), (3, 100, 16, 24, 1.0), (2, 1200, 400, 80, 0.0),
                               (2, 1200, 0, 80, 1.0), (1, 5, 400, 80, 0.0), (1, 1024, 1024, 1, 1.0), (1, 1025, 1, 1, 1.0)):
        F = PO.frame_count(T, win, hop) if wp > 0 and win > 0 else 0
        want = 8 * (n * F + n * ((T + _lib.SCORE_TILE - 1) // _lib.SCORE_TILE) + n * F * win)
        assert built_lib.pwv_train_loss_workspace_bytes(ctypes.byref(_args(n, T, win, hop, 1.0, wp))) == want, (n, T, win, hop, wp)
    assert built_lib.pwv_train_loss_workspace_bytes(None) == 0


def test_train_loss_refusals_no_gpu(built_lib):
    """Every refusal of pwv_train_loss_f32 returns -1 (PWV_EINVAL) with its field named and gives the workspace size 0, before anything
    touches a device (this process has none)."""
    def refused(a, word, sized=True):
        code = built_lib.pwv_train_loss_f32(ctypes.byref(a), None)
        msg = built_lib.pwv_last_error()
        assert code == -1 and word in msg and b'pwv_train_loss_f32' in msg, (code, word, msg)
        if sized:
            assert built_lib.pwv_train_loss_workspace_bytes(ctypes.byref(a)) == 0 and word in built_lib.pwv_last_error()

    assert built_lib.pwv_train_loss_f32(None, None) == -1 and b'NULL' in built_lib.pwv_last_error()
    a = _args()
    a.struct_size = 0
    refused(a, b'struct_size')
    a.struct_size = ctypes.sizeof(a) - 8
    refused(a, b'struct_size')
    for n in (0, -1):
        refused(_args(n=n), b': n ')
    for T in (0, -5):
        refused(_args(T=T), b': T ')
    for hop in (0, -80):
        refused(_args(hop=hop), b'hop_length')
    from pwv_amd import _lib
    for win in (_lib.SCORE_MAX_WIN + 1, 4096, -1):
        refused(_args(win=win, T=8000), b'win_length')
    refused(_args(T=399), b'win_length')                       # weight_power > 0 and no frame
    refused(_args(T=399), b': T ')
    for bad in (-1.0, float('inf'), float('-inf'), float('nan')):
        refused(_args(wl1=bad), b'weight_l1')
        refused(_args(wp=bad), b'weight_power')
    refused(_args(n=3, T=1 << 30), b'n T')                     # beyond int32
    refused(_args(n=1 << 16, T=1 << 15), b'int32')
    # the pointers and the workspace are the call's alone: the size is still answered
    for field in ('out', 'y', 'd_out', 'result', 'workspace'):
        a = _args()
        setattr(a, field, None)
        refused(a, b'NULL pointer', sized=False)
        refused(a, (': %s ' % field).encode(), sized=False)
        assert built_lib.pwv_train_loss_workspace_bytes(ctypes.byref(a)) > 0
    a = _args()
    a.workspace_bytes = built_lib.pwv_train_loss_workspace_bytes(ctypes.byref(a)) - 1
    refused(a, b'workspace_bytes', sized=False)
    a.workspace_bytes = 0
    refused(a, b'workspace_bytes', sized=False)
    # what is NOT refused, up to the launch: the L1 alone on an utterance shorter than a window, and the largest window
    for ok in (_args(T=399, wp=0.0), _args(T=399, win=0), _args(T=1024, win=_lib.SCORE_MAX_WIN)):
        assert built_lib.pwv_train_loss_workspace_bytes(ctypes.byref(ok)) > 0


def _cpu_model(length=TO.T):
    from pwv_amd.models import IAFVocoder
    from pwv_amd.variables import VariableStore
    set_hparams(TO.small_cfg())
    return IAFVocoder(TO.N, length, store=VariableStore(device='cpu'), precision='f32')


def test_bare_call_still_refuses_and_the_opt_in_is_checked():
    """hp.train.weight_power_loss = 0.0005 without power_weight is refused as before, the message now pointing at power_weight; with
    power_weight the hparams line is not consulted; power_weight > 0 on a model shorter than a window is refused naming both; a negative
    or non-finite power_weight is refused.  CPU tensors: every refusal comes before a device is touched."""
    from pwv_amd import train as TR
    from pwv_amd._lib import PwvError
    from pwv_amd.hparam import hparam as hp
    model = _cpu_model()
    wav, mel = torch.zeros(TO.N, TO.T), torch.zeros(TO.N, 1 + TO.T // 16, 80)
    hp.train.weight_power_loss = 0.0005
    with pytest.raises(PwvError, match='training refused.*weight_power_loss.*power_weight'):
        TR.loss_and_grad(model, wav, mel)
    assert 'weight_power_loss' in TR.refusal(model) and 'weight_power_loss' in TR.refusal()
    assert TR.refusal(power_weight=0.0005) is None and TR.refusal(model, power_weight=0.0) is None       # the hparams line is not consulted
    with pytest.raises(PwvError, match='weight_power_loss'):
        TR.Trainer(model)._bind()
    assert hp.signal.win_length == 400 and model.length == 208
    for call in (lambda: TR.loss_and_grad(model, wav, mel, power_weight=0.0005), lambda: TR.Trainer(model, power_weight=0.0005)._bind()):
        with pytest.raises(PwvError, match='training refused') as e:
            call()
        assert 'power_weight' in str(e.value) and 'length 208' in str(e.value) and 'win_length 400' in str(e.value)
    assert TR.refusal(model, power_weight=0.0) is None                    # weight 0 forms no frame
    hp.signal.win_length = 48
    assert TR.refusal(model, power_weight=0.0005) is None
    for bad in (-1.0, float('nan'), float('inf')):
        assert 'power_weight' in TR.refusal(model, power_weight=bad)
    hp.train.weight_power_loss = 0.0
    assert TR.refusal(model) is None
    tr = TR.Trainer(model, power_weight=0.25)
    assert tr.power_weight == 0.25 and tr.terms == {} and TR.Trainer(model).power_weight is None
    set_hparams(TO.small_cfg())


def test_small_power_case_is_small_plus_the_weight():
    """hparams: train/small_power = train/small + train.weight_power_loss 0.0005; 800 samples at win 400 / hop 80 are 6 frames."""
    from pwv_amd import train as TR
    from pwv_amd.hparam import hparam as hp

    def plain(d):
        return {k: plain(v) for k, v in d.items()} if isinstance(d, dict) else d

    hp.set_hparam_yaml('train/small')
    small = plain(dict(hp))
    assert TR.refusal() is None
    hp.set_hparam_yaml('train/small_power')
    power = plain(dict(hp))
    assert power['train']['weight_power_loss'] == 0.0005 and small['train']['weight_power_loss'] == 0
    assert 'weight_power_loss' in TR.refusal() and TR.refusal(power_weight=0.0005) is None
    assert PO.frame_count(int(hp.signal.length), int(hp.signal.win_length), int(hp.signal.hop_length)) == 6
    for d in (small, power):
        d['train'] = {k: v for k, v in d['train'].items() if k != 'weight_power_loss'}
        for k in [k for k in d if 'logdir' in k or k == 'case']:
            del d[k]
    assert small == power
    hp.set_hparam_yaml('default')


def test_train_loss_kernel_resources():
    """The compiler's resource remarks (gfx950 device code) for the four kernels of csrc/pwv_train_loss.hip, the uniform and the packed
    instances of the loss head: no scratch, no spilled register; the largest dynamic LDS request, at win = nfft = 1024, fits the 64 KiB
    a workgroup may ask for."""
    res = kernel_resources('pwv_train_loss.hip')
    assert len(res) == 4, sorted(res)
    for k in ('loss_frames_kernel', 'loss_gather_kernel', 'loss_frames_varlen_kernel', 'loss_gather_varlen_kernel'):
        assert any(k in n for n in res), (k, sorted(res))
    for name, r in res.items():
        assert r['scratch'] == 0 and r['vgpr_spills'] == 0 and r['sgpr_spills'] == 0 and not r['dynamic_stack'], (name, r)
    assert 8 * (256 + 2 * 1024 + 2 * 513 + 2 * 1024) <= 64 * 1024
