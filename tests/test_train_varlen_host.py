"""CPU: training on packed batches (include/pwv_hip_train_varlen.h, csrc/pwv_train_varlen.hip, train.loss_and_grad_varlen) -- the C
structs against their ctypes mirrors, the header's symbols, every host refusal, the kernels' resources, and the Python caller's own
checks.  Nothing here needs a GPU."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from tests import train_oracle as TO
from tests import train_varlen_oracle as VO
from tests.util import kernel_resources, set_hparams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD_PART = 64 * 128 + 128 + 128 * 128 + 128 + 128 + 1


def _probe(tmp_path, struct, fields):
    c_name = lambda f: 'in' if f == 'in_' else f
    probe = ['sizeof(%s)' % struct] + ['offsetof(%s, %s)' % (struct, c_name(f)) for f in fields] + ['(size_t)PWV_HIP_VERSION']
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "pwv_hip_train_varlen.h"\nint main(void){ printf("%s\\n", %s); return 0; }\n'
           % (' '.join(['%zu'] * len(probe)), ', '.join(probe)))
    c, exe = str(tmp_path / (struct + '.c')), str(tmp_path / struct)
    with open(c, 'w') as f:
        f.write(src)
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Wextra', '-pedantic', '-Werror', '-I' + os.path.join(ROOT, 'include'), c, '-o', exe])
    return [int(x) for x in subprocess.check_output([exe]).decode().split()]


def test_varlen_args_layouts_match_ctypes(tmp_path):
    """The C compiler's size and offsets of both new structs (gcc -std=c99 -pedantic -Werror) against the ctypes mirrors;
    pwv_train_varlen_args is pwv_train_args followed by the packed batch."""
    from pwv_amd import _lib
    for struct, mirror in (('pwv_train_varlen_args', _lib.TrainVarlenArgs), ('pwv_train_loss_varlen_args', _lib.TrainLossVarlenArgs)):
        fields = [n for n, _ in mirror._fields_]
        assert _probe(tmp_path, struct, fields) == [ctypes.sizeof(mirror)] + [getattr(mirror, f).offset for f in fields] + [301]
        assert mirror().struct_size == ctypes.sizeof(mirror)
    old = [n for n, _ in _lib.TrainArgs._fields_]
    new = [n for n, _ in _lib.TrainVarlenArgs._fields_]
    assert new == old + ['cu_rows', 'cu_frames', 'n', 'rows', 'proj_rows']
    assert all(getattr(_lib.TrainVarlenArgs, f).offset == getattr(_lib.TrainArgs, f).offset for f in old)
    assert [n for n, _ in _lib.TrainLossVarlenArgs._fields_] == ['struct_size', 'out', 'y', 'cu_rows', 'n', 'rows', 'win_length', 'hop_length',
                                                                 'weight_l1', 'weight_power', 'd_out', 'result', 'workspace', 'workspace_bytes']


def test_header_declares_exactly_the_new_symbols():
    """include/pwv_hip_train_varlen.h declares exactly _lib.TRAIN_VARLEN_SYMBOLS, the library exports them, and the older lists are what
    they were and disjoint from the new one."""
    from pwv_amd import _lib
    _lib.build_library()
    code = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'pwv_hip_train_varlen.h')).read(), flags=re.S)
    assert sorted(set(re.findall(r'\b(pwv_[a-z0-9_]+)\s*\(', code))) == sorted(_lib.TRAIN_VARLEN_SYMBOLS) == [
        'pwv_train_loss_varlen_f32', 'pwv_train_loss_varlen_workspace_bytes', 'pwv_train_varlen_front_bwd_f32', 'pwv_train_varlen_front_fwd_f32',
        'pwv_train_varlen_layer_bwd_f32', 'pwv_train_varlen_layer_fwd_f32']
    older = [_lib.EXPORTED_SYMBOLS, _lib.EXTENSION_SYMBOLS, _lib.LIVE_TICK_SYMBOLS, _lib.SCORE_SYMBOLS, _lib.TRAIN_SYMBOLS, _lib.TRAIN_LOSS_SYMBOLS]
    assert [len(s) for s in older] == [52, 1, 2, 2, 7, 2]
    assert _lib.TRAIN_SYMBOLS == ('pwv_train_workspace_bytes', 'pwv_train_front_fwd_f32', 'pwv_train_layer_fwd_f32', 'pwv_train_head_fwd_f32',
                                  'pwv_train_head_bwd_f32', 'pwv_train_layer_bwd_f32', 'pwv_train_front_bwd_f32')
    assert _lib.TRAIN_LOSS_SYMBOLS == ('pwv_train_loss_workspace_bytes', 'pwv_train_loss_f32')
    taken = set().union(*older)
    assert len(taken) == 66 and not set(_lib.TRAIN_VARLEN_SYMBOLS) & taken
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(raw, name) for name in _lib.TRAIN_VARLEN_SYMBOLS)
    raw.pwv_version.restype = ctypes.c_int
    assert raw.pwv_version() == 301 and '#define PWV_HIP_VERSION 301' in open(os.path.join(ROOT, 'include', 'pwv_hip.h')).read()
    assert os.path.join(os.path.dirname(_lib.__file__), 'csrc', 'pwv_train_varlen.hip') in _lib.CSRC
    for header, symbols in (('pwv_hip_train.h', _lib.TRAIN_SYMBOLS), ('pwv_hip_train_loss.h', _lib.TRAIN_LOSS_SYMBOLS)):
        code = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', header)).read(), flags=re.S)
        assert sorted(set(re.findall(r'\b(pwv_[a-z0-9_]+)\s*\(', code))) == sorted(symbols)


def _args(**kw):
    """A pwv_train_varlen_args the library accepts up to its launch: every device pointer a number that is never dereferenced on the host."""
    from pwv_amd import _lib
    a = _lib.TrainVarlenArgs(dilation=1, next_dilation=1, cond_hop=16, cond_offset=8, proj_row_stride=128, d_proj_row_stride=128, max_workgroups=3,
                             n=4, rows=416, proj_rows=30)
    for f in ('in_', 'x', 'x_out', 'proj', 'causal_filter', 'filter', 'gate', 'dense', 'u_next', 'v_next', 'd_o', 'd_proj', 'd_causal_filter',
              'd_filter', 'd_gate', 'd_dense', 'workspace', 'cu_rows', 'cu_frames'):
        setattr(a, f, 4096)
    a.u, a.v = 8192, 12288
    a.workspace_bytes = 1 << 40
    for k, v in kw.items():
        setattr(a, k, v)
    return a


ENTRIES = ('pwv_train_varlen_front_fwd_f32', 'pwv_train_varlen_layer_fwd_f32', 'pwv_train_varlen_layer_bwd_f32', 'pwv_train_varlen_front_bwd_f32')


def test_varlen_calls_refuse_bad_arguments_on_the_host(built_lib):
    """Every refusal of the four packed entry points returns -1 (PWV_EINVAL) with its field named, before anything touches a device
    (this process has none)."""
    from pwv_amd import _lib
    lib = built_lib

    def refused(name, a, word):
        code = getattr(lib, name)(ctypes.byref(a) if a is not None else None, None)
        msg = lib.pwv_last_error().decode()
        assert code == -1 and word in msg and name in msg, (name, code, word, msg)

    for name in ENTRIES:
        refused(name, None, 'NULL')
        refused(name, _args(cu_rows=None), 'cu_rows')
        refused(name, _args(cu_frames=None), 'cu_frames')
        refused(name, _args(n=0), 'n = 0')
        refused(name, _args(n=-1), 'n = -1')
        refused(name, _args(rows=3), 'rows = 3')
        refused(name, _args(rows=2 ** 31 - 64), 'rows')
        refused(name, _args(rows=2 ** 31 - 1), 'beyond int32')
        refused(name, _args(proj_rows=3), 'proj_rows = 3')
        refused(name, _args(cond_hop=0), 'cond_hop')
        a = _args()
        a.struct_size -= 8
        refused(name, a, 'struct_size')
        a.struct_size = ctypes.sizeof(_lib.TrainArgs)           # (the uniform struct is no packed one)
        refused(name, a, 'struct_size')
    for name in ENTRIES[1:3]:
        refused(name, _args(dilation=0), 'dilation')
        refused(name, _args(proj_row_stride=64), 'proj_row_stride')
        refused(name, _args(x=None), 'NULL')
    refused(ENTRIES[0], _args(in_=None), 'NULL')
    refused(ENTRIES[2], _args(workspace=None), 'workspace')
    refused(ENTRIES[3], _args(workspace=None), 'workspace')
    refused(ENTRIES[2], _args(workspace_bytes=3 * (128 * 128 + 64 * 64 + 64) * 4 - 1), 'workspace_bytes')
    refused(ENTRIES[3], _args(workspace_bytes=3 * 128 * 4 - 1), 'workspace_bytes')
    refused(ENTRIES[2], _args(d_proj_row_stride=64), 'd_proj_row_stride')
    refused(ENTRIES[2], _args(u=4096), 'alias')
    # the workspace of pwv_hip_train.h at N = 1, T = rows serves the packed calls
    flat = _lib.TrainArgs(N=1, T=416, max_workgroups=3)
    assert lib.pwv_train_workspace_bytes(ctypes.byref(flat)) == 3 * HEAD_PART * 4


def _loss_args(**kw):
    from pwv_amd import _lib
    a = _lib.TrainLossVarlenArgs(n=4, rows=416, win_length=48, hop_length=16, weight_l1=1.0, weight_power=0.5)
    a.out = a.y = a.cu_rows = a.d_out = a.result = a.workspace = 4096
    a.workspace_bytes = 1 << 40
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_varlen_loss_refusals_and_workspace(built_lib):
    """Every refusal of pwv_train_loss_varlen_f32 names its field and gives the workspace size 0; the workspace is rows / hop + n frame
    slots (a partial and win gradient values each) + rows / TILE + n tile slots, one double each, and no frame slot in the L1-only modes."""
    from pwv_amd import _lib
    lib = built_lib

    def refused(a, word, sized=True):
        code = lib.pwv_train_loss_varlen_f32(ctypes.byref(a) if a is not None else None, None)
        msg = lib.pwv_last_error().decode()
        assert code == -1 and word in msg and 'pwv_train_loss_varlen_f32' in msg, (code, word, msg)
        if sized and a is not None:
            assert lib.pwv_train_loss_varlen_workspace_bytes(ctypes.byref(a)) == 0 and word in lib.pwv_last_error().decode()

    refused(None, 'NULL')
    a = _loss_args()
    a.struct_size -= 8
    refused(a, 'struct_size')
    a = _loss_args()
    a.struct_size += 8
    refused(a, 'struct_size')
    refused(_loss_args(n=0), ': n ')
    refused(_loss_args(rows=3), 'rows 3')
    refused(_loss_args(rows=2 ** 31 - 64), 'rows')
    refused(_loss_args(hop_length=0), 'hop_length')
    refused(_loss_args(win_length=-1), 'win_length')
    refused(_loss_args(win_length=_lib.SCORE_MAX_WIN + 1), 'win_length')
    refused(_loss_args(weight_l1=-1.0), 'weight_l1')
    refused(_loss_args(weight_power=float('inf')), 'weight_power')
    refused(_loss_args(weight_power=float('nan')), 'weight_power')
    for f in ('out', 'y', 'cu_rows', 'd_out', 'result', 'workspace'):
        refused(_loss_args(**{f: None}), f, sized=False)
    slots = lambda rows, n, win, hop: (rows // hop + n) * (1 + win) + rows // _lib.SCORE_TILE + n
    for rows, n, win, hop, wp in ((416, 4, 48, 16, 0.5), (32000, 8, 400, 80, 0.0005), (5000, 3, 1024, 1, 1.0), (416, 4, 48, 16, 0.0), (416, 4, 0, 16, 1.0)):
        want = 8 * (slots(rows, n, win, hop) if win > 0 and wp > 0 else rows // _lib.SCORE_TILE + n)
        a = _loss_args(rows=rows, n=n, win_length=win, hop_length=hop, weight_power=wp)
        assert lib.pwv_train_loss_varlen_workspace_bytes(ctypes.byref(a)) == want, (rows, n, win, hop, wp)
        a.workspace_bytes = want - 1
        refused(a, 'workspace_bytes', sized=False)
    assert lib.pwv_train_loss_varlen_workspace_bytes(None) == 0


def test_varlen_kernel_resources():
    """The compiler's resource remarks (gfx950 device code) for every kernel of csrc/pwv_train_varlen.hip and for the re-instantiated
    uniform kernels of csrc/pwv_train.hip: no scratch, no spilled register, LDS within the 64 KiB a workgroup may declare statically;
    the loss head's largest dynamic LDS request, at win = nfft = 1024, fits too (its packed kernels are csrc/pwv_train_loss.hip's:
    tests/test_train_power_host.py)."""
    res = kernel_resources('pwv_train_varlen.hip')
    names = ' '.join(res)
    for k in ('train_front_fwd_varlen_kernel', 'train_layer_fwd_varlen_kernel', 'train_layer_bwd_varlen_kernel<true>',
              'train_layer_bwd_varlen_kernel<false>', 'train_front_bwd_varlen_kernel'):
        assert k in names, (k, names)
    assert len(res) == 5
    uniform = kernel_resources('pwv_train.hip')
    assert len(uniform) == 8
    for name, r in list(res.items()) + list(uniform.items()):
        assert r['scratch'] == 0 and r['vgpr_spills'] == 0 and r['sgpr_spills'] == 0 and not r['dynamic_stack'], (name, r)
        assert r['lds'] <= 64 * 1024, (name, r)
    assert 8 * (256 + 2 * 1024 + 2 * 513 + 2 * 1024) <= 64 * 1024
    # the packed kernels hold the unit's places in LDS: 33 rows x (t, T_i, P row, first row of the frame)
    by = lambda d, k: next(r for n, r in d.items() if k in n)
    for a, b in (('train_layer_fwd_kernel', 'train_layer_fwd_varlen_kernel'), ('train_front_bwd_kernel', 'train_front_bwd_varlen_kernel'),
                 ('train_layer_bwd_kernel<false>', 'train_layer_bwd_varlen_kernel<false>')):
        assert 0 < by(res, b)['lds'] - by(uniform, a)['lds'] <= 4 * 33 * 4 + 16, (a, b)


# ---- the Python caller ----------------------------------------------------------------------------------------------------------------
def _cpu_model():
    from pwv_amd.models import IAFVocoder
    from pwv_amd.variables import VariableStore
    set_hparams(TO.small_cfg())
    return IAFVocoder(1, 208, store=VariableStore(device='cpu'), precision='f32')


def _cpu_batch(lengths=tuple(VO.LENGTHS)):
    return [torch.zeros(T) for T in lengths], [torch.zeros(1 + T // 16, 80) for T in lengths]


def test_loss_and_grad_varlen_checks_its_lists():
    """A length that is not a multiple of hop, a mel of the wrong frame count and mismatched list lengths are ValueErrors that name the
    utterance, before a device is touched (CPU tensors)."""
    from pwv_amd import train as TR
    model = _cpu_model()
    wavs, mels = _cpu_batch()
    bad = list(wavs)
    bad[2] = torch.zeros(50)
    with pytest.raises(ValueError, match=r'wavs\[2\].*multiple of hop_length 16'):
        TR.loss_and_grad_varlen(model, bad, mels)
    bad[2] = torch.zeros(8)
    with pytest.raises(ValueError, match=r'wavs\[2\]'):
        TR.loss_and_grad_varlen(model, bad, mels)
    bad_mels = list(mels)
    bad_mels[1] = torch.zeros(3, 80)
    with pytest.raises(ValueError, match=r'mels\[1\].*\[2, 80\]'):
        TR.loss_and_grad_varlen(model, wavs, bad_mels)
    with pytest.raises(ValueError, match='wavs holds 4 utterances, mels 3'):
        TR.loss_and_grad_varlen(model, wavs, mels[:3])
    with pytest.raises(ValueError, match='z must be a list of 4'):
        TR.loss_and_grad_varlen(model, wavs, mels, z=[torch.zeros(208, 1)])
    with pytest.raises(ValueError, match='seeds holds 2 values'):
        TR.loss_and_grad_varlen(model, wavs, mels, seeds=[1, 2])
    with pytest.raises(ValueError, match='non-empty lists'):
        TR.loss_and_grad_varlen(model, torch.zeros(2, 208), torch.zeros(2, 14, 80))


def test_loss_and_grad_still_refuses_lists_and_varlen_refuses_the_rest():
    """loss_and_grad keeps refusing a list with "packed inputs"; loss_and_grad_varlen refuses what `refusal` names, and a power weight
    with no utterance as long as win_length, by name."""
    from pwv_amd import train as TR
    from pwv_amd._lib import PwvError
    from pwv_amd.hparam import hparam as hp
    from pwv_amd.models import IAFVocoder
    from pwv_amd.variables import VariableStore
    model = _cpu_model()
    wavs, mels = _cpu_batch()
    with pytest.raises(PwvError, match='packed inputs'):
        TR.loss_and_grad(model, wavs, mels)
    assert 'packed inputs' in TR.refusal(model, wavs, mels)
    hp.signal.win_length = 400
    with pytest.raises(PwvError, match=r'training refused: power_weight 0.5 > 0 with no utterance as long as signal.win_length 400'):
        TR.loss_and_grad_varlen(model, wavs, mels, power_weight=0.5)
    with pytest.raises(PwvError, match='power_weight'):
        TR.loss_and_grad_varlen(model, wavs, mels, power_weight=-1.0)
    assert TR.refusal(model, power_weight=0.5) and TR.refusal(model, power_weight=0.5, packed=True) is None
    f16 = IAFVocoder(1, 208, store=VariableStore(device='cpu'), precision='f16x3')
    with pytest.raises(PwvError, match='f16x3'):
        TR.loss_and_grad_varlen(f16, wavs, mels)
    hp.model.use_skip_connection = True
    with pytest.raises(PwvError, match='skip accumulation'):
        TR.loss_and_grad_varlen(model, wavs, mels)
    hp.set_hparam_yaml('default')


def test_small_varlen_case_and_the_stand_ins():
    """hparams/hparams.yaml has train/small_varlen; with --varlen the seeded stand-ins differ in length, are at least signal.length long and
    the same for the same seed."""
    from pwv_amd import train as TR
    from pwv_amd.hparam import hparam as hp
    hp.set_hparam_yaml('train/small_varlen')
    assert hp.data_path == 'synthetic' and int(hp.train.varlen_max_length) == 1600 and TR.refusal() is None
    length = int(hp.signal.length)
    a, b = TR._dataset(length, 4, varlen=True), TR._dataset(length, 4, varlen=True)
    assert len(set(len(w) for w in a)) > 1 and min(len(w) for w in a) >= length > int(hp.signal.n_fft) // 2
    assert all((x == y).all() for x, y in zip(a, b))
    assert [len(w) for w in TR._dataset(length, 4)] == [4 * length] * 8
    hp.set_hparam_yaml('default')
