"""CPU: training the skip-connection architecture (include/pwv_hip_train_skip.h, csrc/pwv_train_skip.hip, train.refusal and the skip
branch of train.py) -- the C struct against its ctypes mirror, the header's symbols, every host refusal, the kernels' resources, the
table of what `refusal` lets through, the oracle against central differences, and the hparams case.  Nothing here needs a GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import train_oracle as TO
from tests import train_skip_oracle as SO
from tests.util import kernel_resources, set_hparams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYER_PART = 128 * 128 + 64 * 64 + 64
HEAD_PART = 64 * 128 + 128 + 128 * 128 + 128 + 128 + 1
SKIP_PART = LAYER_PART + 64 * 128
OWN = ['skip_sum', 'd_skip_sum', 'd_skip_sum_out', 'd_skip', 'd_skip_bias', 'skip_accumulate', 'cu_rows', 'cu_frames', 'n', 'rows', 'proj_rows']


def test_skip_args_layout_matches_ctypes(tmp_path):
    """The C compiler's size and offsets of pwv_train_skip_args (gcc -std=c99 -pedantic -Werror) against the ctypes mirror: the embedded
    pwv_train_args first, then the skip fields and the packed tables."""
    from pwv_amd import _lib
    mirror = _lib.TrainSkipArgs
    assert [n for n, _ in mirror._fields_] == ['train'] + OWN and sorted(mirror.OWN) == sorted(OWN)
    old = [n for n, _ in _lib.TrainArgs._fields_]
    probe = (['sizeof(pwv_train_skip_args)', 'offsetof(pwv_train_skip_args, train)'] + ['offsetof(pwv_train_skip_args, %s)' % f for f in OWN]
             + ['offsetof(pwv_train_skip_args, train.%s)' % ('in' if f == 'in_' else f) for f in old]
             + ['sizeof(pwv_train_args)', 'sizeof(pwv_train_varlen_args)', '(size_t)PWV_HIP_VERSION'])
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "pwv_hip_train_skip.h"\nint main(void){ printf("%s\\n", %s); return 0; }\n'
           % (' '.join(['%zu'] * len(probe)), ', '.join(probe)))
    c, exe = str(tmp_path / 'skip.c'), str(tmp_path / 'skip')
    with open(c, 'w') as f:
        f.write(src)
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Wextra', '-pedantic', '-Werror', '-I' + os.path.join(ROOT, 'include'), c, '-o', exe])
    got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    assert got == ([ctypes.sizeof(mirror), mirror.train.offset] + [getattr(mirror, f).offset for f in OWN]
                   + [getattr(_lib.TrainArgs, f).offset for f in old]
                   + [ctypes.sizeof(_lib.TrainArgs), ctypes.sizeof(_lib.TrainVarlenArgs), 301])
    assert mirror.train.offset == 0 and mirror().train.struct_size == ctypes.sizeof(mirror) > ctypes.sizeof(_lib.TrainVarlenArgs)
    a = mirror(N=3, d_skip=64, skip_sum=128, rows=5)           # a name the two structs share goes to the new field
    assert (a.train.N, a.d_skip, a.train.d_skip, a.skip_sum, a.rows) == (3, 64, None, 128, 5)


def test_header_declares_exactly_the_new_symbols():
    """include/pwv_hip_train_skip.h declares exactly _lib.TRAIN_SKIP_SYMBOLS, the library exports them, the older lists are what they
    were, and pwv_hip.h keeps its version."""
    from pwv_amd import _lib
    _lib.build_library()
    code = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'pwv_hip_train_skip.h')).read(), flags=re.S)
    assert sorted(set(re.findall(r'\b(pwv_[a-z0-9_]+)\s*\(', code))) == sorted(_lib.TRAIN_SKIP_SYMBOLS) == [
        'pwv_train_skip_head_bwd_f32', 'pwv_train_skip_head_fwd_f32', 'pwv_train_skip_layer_bwd_f32', 'pwv_train_skip_layer_fwd_f32',
        'pwv_train_skip_workspace_bytes']
    older = [_lib.EXPORTED_SYMBOLS, _lib.EXTENSION_SYMBOLS, _lib.LIVE_TICK_SYMBOLS, _lib.SCORE_SYMBOLS, _lib.TRAIN_SYMBOLS, _lib.TRAIN_LOSS_SYMBOLS,
             _lib.TRAIN_VARLEN_SYMBOLS, _lib.TRAIN_COND_SYMBOLS, _lib.TRAIN_OPT_SYMBOLS]
    assert [len(s) for s in older] == [52, 1, 2, 2, 7, 2, 6, 3, 3]
    assert not set(_lib.TRAIN_SKIP_SYMBOLS) & set().union(*older)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(raw, name) for name in _lib.TRAIN_SKIP_SYMBOLS)
    raw.pwv_version.restype = ctypes.c_int
    assert raw.pwv_version() == 301 and '#define PWV_HIP_VERSION 301' in open(os.path.join(ROOT, 'include', 'pwv_hip.h')).read()
    assert os.path.join(os.path.dirname(_lib.__file__), 'csrc', 'pwv_train_skip.hip') in _lib.CSRC


def _args(packed=False, **kw):
    """A pwv_train_skip_args the library accepts up to its launch: every device pointer a number that is never dereferenced on the host."""
    from pwv_amd import _lib
    a = _lib.TrainSkipArgs(N=2, T=200, dilation=1, next_dilation=1, max_workgroups=3, cond_hop=16, cond_offset=8, cond_frames=13,
                           proj_row_stride=128, d_proj_row_stride=128)
    for f in ('x', 'x_out', 'proj', 'filter', 'gate', 'dense', 'skip', 'post1', 'post2', 'y', 'd_out', 'u_next', 'v_next', 'd_proj', 'd_filter',
              'd_gate', 'd_dense', 'workspace', 'skip_sum', 'd_skip_sum', 'd_skip_sum_out', 'd_skip'):
        a.set(**{f: 4096})
    a.set(u=8192, v=12288, workspace_bytes=1 << 40)
    if packed:
        a.set(cu_rows=4096, cu_frames=4096, n=2, rows=400, proj_rows=27, N=0, T=0, cond_frames=0)
    return a.set(**kw)


LAYER_FWD, HEAD_FWD, HEAD_BWD, LAYER_BWD = ('pwv_train_skip_layer_fwd_f32', 'pwv_train_skip_head_fwd_f32', 'pwv_train_skip_head_bwd_f32',
                                            'pwv_train_skip_layer_bwd_f32')


def test_skip_calls_refuse_bad_arguments_on_the_host(built_lib):
    """Every refusal of the four entry points returns -1 (PWV_EINVAL) with its field named, before anything touches a device (this
    process has none); the workspace is grid x max(head partial, layer partial + 64 x 128) floats."""
    from pwv_amd import _lib
    lib = built_lib

    def refused(name, a, word):
        code = getattr(lib, name)(ctypes.byref(a) if a is not None else None, None)
        msg = lib.pwv_last_error().decode()
        assert code == -1 and word in msg and name in msg, (name, code, word, msg)

    for name in (LAYER_FWD, HEAD_FWD, HEAD_BWD, LAYER_BWD):
        refused(name, None, 'NULL')
        refused(name, _args(N=0), 'N = 0')
        refused(name, _args(T=2 ** 30), 'beyond int32')
        refused(name, _args(max_workgroups=-1), 'max_workgroups')
        for packed in (False, True):
            a = _args(packed)
            a.train.struct_size = ctypes.sizeof(_lib.TrainVarlenArgs)      # (neither older struct is a skip one)
            refused(name, a, 'train.struct_size')
        refused(name, _args(True, n=0), 'n = 0')
        refused(name, _args(True, rows=1), 'rows = 1')
        refused(name, _args(True, max_workgroups=-1), 'max_workgroups')
    for name in (LAYER_FWD, LAYER_BWD):
        refused(name, _args(x=None), 'NULL')
        refused(name, _args(proj=None), 'proj')
        refused(name, _args(dilation=0), 'dilation')
        refused(name, _args(form=2), 'form')
        refused(name, _args(cond_hop=0), 'cond_hop')
        refused(name, _args(cond_frames=12), 'cond_frames 12')
        refused(name, _args(proj_row_stride=64), 'proj_row_stride')
        refused(name, _args(skip=None), 'train.skip is a NULL')
        refused(name, _args(dense=None), 'dense')
        refused(name, _args(True, cu_frames=None), 'cu_frames')
        refused(name, _args(True, proj_rows=1), 'proj_rows')
    refused(LAYER_FWD, _args(skip_sum=None), 'skip_sum is a NULL')
    refused(LAYER_FWD, _args(x_out=None), 'x_out')
    refused(HEAD_FWD, _args(skip_sum=None), 'skip_sum is a NULL')
    refused(HEAD_FWD, _args(post1=None), 'post1')
    refused(HEAD_FWD, _args(y=None), 'y is a NULL')
    refused(HEAD_BWD, _args(skip_sum=None), 'skip_sum is a NULL')
    refused(HEAD_BWD, _args(d_out=None), 'd_out')
    refused(HEAD_BWD, _args(d_skip_sum_out=None), 'd_skip_sum_out is a NULL')
    refused(HEAD_BWD, _args(workspace=None), 'workspace')
    refused(LAYER_BWD, _args(d_skip_sum=None), 'd_skip_sum is a NULL')
    refused(LAYER_BWD, _args(d_skip=None), 'd_skip is a NULL')
    refused(LAYER_BWD, _args(d_proj=None), 'd_proj')
    refused(LAYER_BWD, _args(u=4096), 'alias')
    refused(LAYER_BWD, _args(u_next=None), 'u_next')
    refused(LAYER_BWD, _args(workspace=None), 'workspace')
    want = 3 * max(HEAD_PART, SKIP_PART) * 4
    assert SKIP_PART > HEAD_PART
    for name in (HEAD_BWD, LAYER_BWD):
        refused(name, _args(workspace_bytes=want - 1), 'workspace_bytes')
        refused(name, _args(True, workspace_bytes=want - 1), 'workspace_bytes')
    for packed in (False, True):
        assert lib.pwv_train_skip_workspace_bytes(ctypes.byref(_args(packed))) == want
    assert want >= lib.pwv_train_workspace_bytes(ctypes.byref(_lib.TrainArgs(N=2, T=200, max_workgroups=3)))
    assert lib.pwv_train_skip_workspace_bytes(ctypes.byref(_args(N=0))) == 0 and 'N = 0' in lib.pwv_last_error().decode()
    assert lib.pwv_train_skip_workspace_bytes(None) == 0
    # a PWV_TRAIN_LAST layer needs neither dense nor x_out nor d_o: past every host check such a call reaches the launch, which this
    # process cannot make -- so only the checks in front of it are asked here
    a = _args(form=_lib.TRAIN_LAST, dense=None, x_out=None, skip_sum=None)
    refused(LAYER_FWD, a, 'skip_sum')


def test_skip_kernel_resources():
    """The compiler's resource remarks (gfx950 device code) for every kernel of csrc/pwv_train_skip.hip: no scratch, no spilled register,
    at most 81920 bytes of static LDS (two workgroups share the 160 KiB of a compute unit; the residual backward keeps the dS tile
    resident beside the layer's own arrays: 49792 + 16512 = 66304 bytes, + 528 for the packed geometry's table) and at most 256
    registers per lane (two waves per SIMD)."""
    res = kernel_resources('pwv_train_skip.hip')
    names = ' '.join(res)
    for k in ('train_skip_layer_fwd_kernel<pwv::UniformGeo>', 'train_skip_layer_fwd_kernel<pwv::PackedGeo>', 'train_skip_head_fwd_kernel',
              'train_skip_head_bwd_kernel', 'train_skip_layer_bwd_kernel<pwv::UniformGeo, true>', 'train_skip_layer_bwd_kernel<pwv::UniformGeo, false>',
              'train_skip_layer_bwd_kernel<pwv::PackedGeo, true>', 'train_skip_layer_bwd_kernel<pwv::PackedGeo, false>'):
        assert k in names, (k, names)
    assert len(res) == 8
    for name, r in res.items():
        assert r['scratch'] == 0 and r['vgpr_spills'] == 0 and r['sgpr_spills'] == 0 and not r['dynamic_stack'], (name, r)
        assert r['lds'] <= 81920, (name, r)
        assert r['vgprs'] + r['agprs'] <= 256, (name, r)
    by = lambda k: next(r for n, r in res.items() if k in n)
    assert by('bwd_kernel<pwv::UniformGeo, false>')['lds'] == 49792 + 16512
    assert by('bwd_kernel<pwv::PackedGeo, false>')['lds'] == 49792 + 16512 + 528
    for source in ('pwv_train_skip.hip', 'pwv_train_head.h'):       # (the head's text is the header's)
        src = open(os.path.join(ROOT, 'parallel-wavenet-vocoder_amd', 'csrc', source)).read()
        assert 'atomic' not in src.lower().replace('no floating-point atomics', ''), source


def _model(cfg, N=TO.N, T=TO.T, precision='f32'):
    from pwv_amd.models import IAFVocoder
    from pwv_amd.variables import VariableStore
    set_hparams(cfg)
    return IAFVocoder(N, T, store=VariableStore(device='cpu'), precision=precision)


def test_refusal_table():
    """A bare call refuses the skip hparams with the words "skip accumulation" and says how to ask; the request is accepted, uniform and
    packed, also with a power weight; a request under hparams that say False is a mismatch; the request with transposed-conv
    conditioning is refused by name; every other refusal stands under the request."""
    from pwv_amd import train as TR
    from pwv_amd._lib import PwvError
    from pwv_amd.hparam import hparam as hp
    cfg = SO.small_cfg()
    try:
        model = _model(cfg)
        bare = TR.refusal(model)
        assert 'skip accumulation' in bare and 'use_skip_connection=True' in bare
        assert 'skip accumulation' in TR.refusal(model, packed=True)
        assert TR.refusal(model, use_skip_connection=True) is None and TR.refusal(model, packed=True, use_skip_connection=True) is None
        hp.signal.win_length = 48
        assert TR.refusal(model, power_weight=0.5, use_skip_connection=True) is None
        assert 'use_skip_connection False' in TR.refusal(model, use_skip_connection=False)
        wav, mel = torch.zeros(TO.N, TO.T), torch.zeros(TO.N, 1 + TO.T // TO.HOP, 80)
        with pytest.raises(PwvError, match='training refused.*skip accumulation'):
            TR.loss_and_grad(model, wav, mel)
        with pytest.raises(PwvError, match='training refused.*skip accumulation'):
            TR.loss_and_grad_varlen(model, [wav[0]], [mel[0]])
        with pytest.raises(PwvError, match='training refused.*skip accumulation'):
            TR.Trainer(model)._bind()
        assert TR.Trainer(model, use_skip_connection=True)._bind() and TR.Trainer(model, use_skip_connection=True, fused=True).use_skip_connection
        # every other refusal is what it was
        assert 'f16x3' in TR.refusal(_model(cfg, precision='f16x3'), use_skip_connection=True)
        hp.model.normalize_wavenet = 'bn'
        assert "'bn'" in TR.refusal(model, use_skip_connection=True)
        hp.model.normalize_wavenet = None
        hp.model.shared_nets = True
        assert 'shared' in TR.refusal(model, use_skip_connection=True)
        # a mismatch: the request under hparams without skip connections
        model = _model(TO.small_cfg())
        why = TR.refusal(model, use_skip_connection=True)
        assert 'does not match' in why and TR.refusal(model) is None
        with pytest.raises(PwvError, match='training refused.*does not match'):
            TR.loss_and_grad(model, wav, mel, use_skip_connection=True)
        with pytest.raises(PwvError, match='training refused.*does not match'):
            TR.loss_and_grad_varlen(model, [wav[0]], [mel[0]], use_skip_connection=True)
        # together with the transposed-conv conditioning: still refused, by name
        tran = type(cfg)(dilations=cfg.dilations, n_iaf=2, hop_length=80, cond_upsample_method='transposed_conv', use_skip_connection=True)
        model = _model(tran, 2, 160)
        for why in (TR.refusal(model), TR.refusal(model, use_skip_connection=True)):
            assert 'skip accumulation' in why
        assert 'transposed_conv' in TR.refusal(model, use_skip_connection=True)
    finally:
        hp.set_hparam_yaml('default')


def test_oracle_counts_and_central_differences():
    """The small skip model has 181 variables, 173 with a gradient; the 8 without are the last layer's dense / dense_bias of each net.
    float64 autograd of three variables -- a first layer's skip, a middle layer's skip_bias, a dense below the last layer -- against
    central differences of the restatement's own loss at h = 1e-6, to 1e-6 relative + 1e-9, as
    tests/test_train_host.py::test_float64_gradient_agrees_with_finite_differences does."""
    cfg, w, mel, z, wav = SO.problem()
    g64 = SO.reference()['g64']
    dead = sorted(k for k, v in g64.items() if v is None)
    assert len(g64) == 181 and len(dead) == SO.DEAD == 8 and len(g64) - len(dead) == SO.LIVE == 173
    assert dead == sorted('iaf_vocoder/iaf%d/%s/dilated_stack/layer3/%s' % (i, net, role) for i in (0, 1) for net in ('scalar', 'shifter')
                          for role in ('dense', 'dense_bias'))
    for net in ('iaf_vocoder/iaf0/scalar', 'iaf_vocoder/iaf1/shifter'):
        sb = [g64['%s/dilated_stack/layer%d/skip_bias' % (net, j)] for j in range(4)]
        assert all(np.array_equal(sb[0], s) for s in sb[1:])                 # the same vector for every layer of a net
    names = ['iaf_vocoder/iaf0/scalar/dilated_stack/layer0/skip', 'iaf_vocoder/iaf1/shifter/dilated_stack/layer1/skip_bias',
             'iaf_vocoder/iaf1/scalar/dilated_stack/layer2/dense']
    rng = np.random.RandomState(1)
    W64 = {k: v.astype(np.float64) for k, v in w.items()}

    def loss(name, idx, delta):
        W = dict(W64)
        W[name] = W64[name].copy()
        W[name][idx] += delta
        return TO.loss_only(W, mel, z, wav, cfg)

    h = 1e-6
    for name in names:
        assert g64[name] is not None and np.abs(g64[name]).max() > 0, name
        flat = np.abs(g64[name]).ravel()
        for p in list(np.argsort(flat)[-2:]) + list(rng.randint(0, flat.size, 2)):
            idx = np.unravel_index(int(p), g64[name].shape)
            fd = (loss(name, idx, h) - loss(name, idx, -h)) / (2 * h)
            assert abs(fd - g64[name][idx]) <= 1e-6 * np.abs(g64[name]).max() + 1e-9, (name, idx, fd, g64[name][idx])


def test_layer_restatement_is_the_model():
    """The one-layer restatement against the model-level oracle's pieces: with g = 0 above the last layer and dS from the head, the
    restated layer's d skip_bias is the head's column sums, and U + V shifted is autograd's gradient of a plain causal layer."""
    c = SO.layer_case(3, 2, 40, 8, 4)
    r = SO.skip_layer(c, False, torch.float64)
    head = SO.skip_head(c, torch.float64)
    assert np.allclose(r['skip_bias'], c['dS'].astype(np.float64).sum(axis=0), rtol=1e-12, atol=1e-12)
    assert np.allclose(head['skip_bias'], head['dS'].sum(axis=0))
    # x_out and S_out of the restatement from first principles, row 5 of utterance 1 (t = 5 >= d = 3)
    row = 45
    a = np.concatenate([c['x'][row - 3], c['x'][row]]).astype(np.float64)
    Wf = np.concatenate([c['filter'][0], c['filter'][1]]).astype(np.float64)
    Wg = np.concatenate([c['gate'][0], c['gate'][1]]).astype(np.float64)
    p = c['P'][c['frames'] + (5 + 4) // 8].astype(np.float64)
    o = np.tanh(a @ Wf + p[:64]) / (1 + np.exp(-(a @ Wg + p[64:])))
    assert np.allclose(r['S_out'][row], c['S_in'][row] + o @ c['skip'][0] + c['skip_bias'], rtol=1e-12, atol=1e-12)
    assert np.allclose(r['x_out'][row], c['x'][row] + o @ c['dense'][0] + c['dense_bias'], rtol=1e-12, atol=1e-12)


def test_small_skip_case_loads():
    """hparams/hparams.yaml has train/small_skip = train/small with use_skip_connection True; `refusal` lets the request through."""
    from pwv_amd import train as TR
    from pwv_amd.hparam import hparam as hp
    from pwv_amd.models import IAFVocoder
    from pwv_amd.variables import VariableStore
    keys = ('n_iaf', 'dilations', 'condition_channels', 'cond_upsample_method')
    try:
        hp.set_hparam_yaml('train/small')
        small = {k: hp.model.get(k) for k in keys}, int(hp.signal.length), int(hp.train.batch_size), dict(hp.generate)
        assert not hp.model.use_skip_connection
        hp.set_hparam_yaml('train/small_skip')
        assert hp.model.use_skip_connection is True and hp.data_path == 'synthetic'
        assert ({k: hp.model.get(k) for k in keys}, int(hp.signal.length), int(hp.train.batch_size), dict(hp.generate)) == small
        assert 'skip accumulation' in TR.refusal() and TR.refusal(use_skip_connection=True) is None
        assert TR.refusal(packed=True, use_skip_connection=True) is None
        store = VariableStore(device='cpu')
        tr = TR.Trainer(IAFVocoder(2, 800, store=store, precision='f32'), use_skip_connection=True)
        tr._bind()
        assert sum('/skip' in n for n in tr.names) == 2 * 2 * (4 + 5)           # skip and skip_bias of all 2 x (4 + 5) net-layers
    finally:
        hp.set_hparam_yaml('default')
