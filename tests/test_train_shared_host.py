"""CPU: training the shared-net architecture (include/pwv_hip_train_shared.h, csrc/pwv_train_shared.hip, train.refusal and the
shared branch of train.py) -- the C struct against its ctypes mirror, the header's symbols, every host refusal, the kernels' resources
(the new ones, and the older training kernels against the project's record), the table of what `refusal` lets through, the oracle
against central differences, and the hparams case with its checkpoint names.  Nothing here needs a GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import train_oracle as TO
from tests import train_shared_oracle as SO
from tests.util import kernel_resources, set_hparams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD_PART = 64 * 128 + 128 + 128 * 128 + 128 + 128 + 1         # the existing head's partial
SHARED_PART = HEAD_PART + 128 + 1                              # + the second column of d post2 and the second d b2
OWN = ['head_in', 'skip_sum', 'd_skip_sum_out', 'y_shift']
WS, FWD, BWD = 'pwv_train_shared_workspace_bytes', 'pwv_train_shared_head_fwd_f32', 'pwv_train_shared_head_bwd_f32'


def test_shared_args_layout_matches_ctypes(tmp_path):
    """The C compiler's size and offsets of pwv_train_shared_args (gcc -std=c99 -pedantic -Werror) against the ctypes mirror: the
    embedded pwv_train_args first, then the input mode, the skip sum, dS and the shift plane."""
    from pwv_amd import _lib
    mirror = _lib.TrainSharedArgs
    assert [n for n, _ in mirror._fields_] == ['train'] + OWN and sorted(mirror.OWN) == sorted(OWN)
    old = [n for n, _ in _lib.TrainArgs._fields_]
    probe = (['sizeof(pwv_train_shared_args)', 'offsetof(pwv_train_shared_args, train)'] + ['offsetof(pwv_train_shared_args, %s)' % f for f in OWN]
             + ['offsetof(pwv_train_shared_args, train.%s)' % ('in' if f == 'in_' else f) for f in old]
             + ['sizeof(pwv_train_args)', 'sizeof(pwv_train_skip_args)', '(size_t)PWV_HIP_VERSION', '(size_t)PWV_TRAIN_HEAD_IN_GATED',
                '(size_t)PWV_TRAIN_HEAD_IN_SKIPSUM'])
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "pwv_hip_train_shared.h"\nint main(void){ printf("%s\\n", %s); return 0; }\n'
           % (' '.join(['%zu'] * len(probe)), ', '.join(probe)))
    c, exe = str(tmp_path / 'shared.c'), str(tmp_path / 'shared')
    with open(c, 'w') as f:
        f.write(src)
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Wextra', '-pedantic', '-Werror', '-I' + os.path.join(ROOT, 'include'), c, '-o', exe])
    got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    assert got == ([ctypes.sizeof(mirror), mirror.train.offset] + [getattr(mirror, f).offset for f in OWN]
                   + [getattr(_lib.TrainArgs, f).offset for f in old]
                   + [ctypes.sizeof(_lib.TrainArgs), ctypes.sizeof(_lib.TrainSkipArgs), 301, _lib.TRAIN_HEAD_IN_GATED, _lib.TRAIN_HEAD_IN_SKIPSUM])
    assert mirror.train.offset == 0 and mirror().train.struct_size == ctypes.sizeof(mirror) > ctypes.sizeof(_lib.TrainArgs)
    a = mirror(N=3, y=64, y_shift=128, head_in=1)
    assert (a.train.N, a.train.y, a.y_shift, a.head_in) == (3, 64, 128, 1)


def test_header_declares_exactly_the_new_symbols():
    """include/pwv_hip_train_shared.h declares exactly _lib.TRAIN_SHARED_SYMBOLS, the library exports them, the older lists are what
    they were, and pwv_hip.h keeps its version."""
    from pwv_amd import _lib
    _lib.build_library()
    code = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'pwv_hip_train_shared.h')).read(), flags=re.S)
    assert sorted(set(re.findall(r'\b(pwv_[a-z0-9_]+)\s*\(', code))) == sorted(_lib.TRAIN_SHARED_SYMBOLS) == sorted([WS, FWD, BWD])
    older = [_lib.EXPORTED_SYMBOLS, _lib.EXTENSION_SYMBOLS, _lib.LIVE_TICK_SYMBOLS, _lib.SCORE_SYMBOLS, _lib.TRAIN_SYMBOLS, _lib.TRAIN_LOSS_SYMBOLS,
             _lib.TRAIN_VARLEN_SYMBOLS, _lib.TRAIN_COND_SYMBOLS, _lib.TRAIN_OPT_SYMBOLS, _lib.TRAIN_SKIP_SYMBOLS]
    assert [len(s) for s in older] == [52, 1, 2, 2, 7, 2, 6, 3, 3, 5]
    assert not set(_lib.TRAIN_SHARED_SYMBOLS) & set().union(*older)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(raw, name) for name in _lib.TRAIN_SHARED_SYMBOLS)
    raw.pwv_version.restype = ctypes.c_int
    assert raw.pwv_version() == 301 and '#define PWV_HIP_VERSION 301' in open(os.path.join(ROOT, 'include', 'pwv_hip.h')).read()
    assert os.path.join(os.path.dirname(_lib.__file__), 'csrc', 'pwv_train_shared.hip') in _lib.CSRC


def _args(mode, **kw):
    """A pwv_train_shared_args the library accepts up to its launch: every device pointer a number that is never dereferenced on the
    host."""
    from pwv_amd import _lib
    a = _lib.TrainSharedArgs(N=2, T=200, max_workgroups=3, head_in=mode, workspace_bytes=1 << 40)
    for f in ('x', 'skip', 'post1', 'post2', 'y', 'y_shift', 'd_out', 'd_mul', 'd_o_out', 'skip_sum', 'd_skip_sum_out', 'workspace'):
        a.set(**{f: 4096})
    return a.set(**kw)


def test_shared_calls_refuse_bad_arguments_on_the_host(built_lib):
    """Every refusal of the entry points returns -1 (PWV_EINVAL) with its field named, before anything touches a device (this process
    has none); the workspace is grid x (the existing head's partial + 129) floats, more than pwv_train_workspace_bytes gives."""
    from pwv_amd import _lib
    lib = built_lib

    def refused(name, a, word):
        code = getattr(lib, name)(ctypes.byref(a) if a is not None else None, None)
        msg = lib.pwv_last_error().decode()
        assert code == -1 and word in msg and name in msg, (name, code, word, msg)

    for name in (FWD, BWD):
        refused(name, None, 'NULL')
        for mode in (SO.GATED, SO.SKIPSUM):
            refused(name, _args(mode, N=0), 'N = 0')
            refused(name, _args(mode, T=2 ** 30), 'beyond int32')
            refused(name, _args(mode, max_workgroups=-1), 'max_workgroups')
            a = _args(mode)
            a.train.struct_size = ctypes.sizeof(_lib.TrainArgs)
            refused(name, a, 'train.struct_size')
            a.train.struct_size = ctypes.sizeof(_lib.TrainSkipArgs)
            refused(name, a, 'train.struct_size')
            refused(name, _args(mode, post1=None), 'post1')
            refused(name, _args(mode, post2=None), 'post2')
        refused(name, _args(2), 'head_in 2')
        refused(name, _args(-1), 'head_in -1')
        refused(name, _args(SO.GATED, x=None), 'train.x is a NULL')
        refused(name, _args(SO.GATED, skip=None), 'train.skip is a NULL')
        refused(name, _args(SO.SKIPSUM, skip_sum=None), 'skip_sum is a NULL')
    # a mode does not need the other mode's pointers: such a call passes every host check of the forward but y
    refused(FWD, _args(SO.GATED, skip_sum=None, d_skip_sum_out=None, y=None), 'train.y is a NULL')
    refused(FWD, _args(SO.SKIPSUM, x=None, skip=None, d_o_out=None, y_shift=None), 'y_shift is a NULL')
    for mode in (SO.GATED, SO.SKIPSUM):
        refused(BWD, _args(mode, d_out=None), 'd_out')
        refused(BWD, _args(mode, workspace=None), 'workspace')
    refused(BWD, _args(SO.GATED, d_o_out=None), 'd_o_out is a NULL')
    refused(BWD, _args(SO.SKIPSUM, d_skip_sum_out=None), 'd_skip_sum_out is a NULL')
    want = 3 * SHARED_PART * 4
    for mode in (SO.GATED, SO.SKIPSUM):
        refused(BWD, _args(mode, workspace_bytes=want - 1), 'workspace_bytes')
        assert lib.pwv_train_shared_workspace_bytes(ctypes.byref(_args(mode))) == want
    assert want > lib.pwv_train_workspace_bytes(ctypes.byref(_lib.TrainArgs(N=2, T=200, max_workgroups=3))) == 3 * HEAD_PART * 4
    assert lib.pwv_train_shared_workspace_bytes(ctypes.byref(_args(0, N=0))) == 0 and 'N = 0' in lib.pwv_last_error().decode()
    assert lib.pwv_train_shared_workspace_bytes(ctypes.byref(_args(7))) == 0 and 'head_in 7' in lib.pwv_last_error().decode()
    assert lib.pwv_train_shared_workspace_bytes(None) == 0


def test_shared_kernel_resources():
    """The compiler's resource remarks (gfx950 device code) for the four kernels of csrc/pwv_train_shared.hip: no scratch, no spilled
    register, at most 81920 bytes of static LDS and at most 256 registers per lane, so that two workgroups share a compute unit."""
    res = kernel_resources('pwv_train_shared.hip')
    names = ' '.join(res)
    for k in ('train_shared_head_fwd_kernel<pwv::GatedIn>', 'train_shared_head_fwd_kernel<pwv::SumIn>',
              'train_shared_head_bwd_kernel<pwv::GatedIn>', 'train_shared_head_bwd_kernel<pwv::SumIn>'):
        assert k in names, (k, names)
    assert len(res) == 4
    for name, r in res.items():
        print(name, r)
        assert r['scratch'] == 0 and r['vgpr_spills'] == 0 and r['sgpr_spills'] == 0 and not r['dynamic_stack'], (name, r)
        assert r['lds'] <= 81920, (name, r)
        assert r['vgprs'] + r['agprs'] <= 256, (name, r)
    by = lambda k: next(r for n, r in res.items() if k in n)
    # the arrays of the existing heads + 32 floats for the second dy plane
    assert by('bwd_kernel<pwv::GatedIn>')['lds'] == 41472 + 128 and by('bwd_kernel<pwv::SumIn>')['lds'] == 33152 + 128
    for source in ('pwv_train_shared.hip', 'pwv_train_head.h'):       # (the head's text is the header's)
        src = open(os.path.join(ROOT, 'parallel-wavenet-vocoder_amd', 'csrc', source)).read()
        assert 'atomic' not in src.lower().replace('no floating-point atomics', ''), source


# (VGPRs, AGPRs, static LDS bytes) of every older training kernel: the tables of DESIGN.md section 9 ("Training", "Packed training",
# "Training the skip-connection architecture"), the project's record of the parent commit
RECORD = {
    'pwv_train.hip': {
        'train_front_fwd_kernel': (20, 0, 0), 'train_layer_fwd_kernel': (92, 16, 41472), 'train_head_fwd_kernel': (66, 16, 41344),
        'train_head_bwd_kernel': (140, 112, 41472), 'train_layer_bwd_kernel<true>': (70, 80, 41472),
        'train_layer_bwd_kernel<false>': (102, 96, 49792), 'train_front_bwd_kernel': (64, 0, 9012), 'train_reduce_kernel': (27, 0, 1024)},
    'pwv_train_varlen.hip': {
        'train_front_fwd_varlen_kernel': (20, 0, 528), 'train_layer_fwd_varlen_kernel': (94, 16, 42000),
        'train_front_bwd_varlen_kernel': (66, 0, 9540), 'train_layer_bwd_varlen_kernel<true>': (72, 80, 42000),
        'train_layer_bwd_varlen_kernel<false>': (104, 96, 50320)},
    'pwv_train_cond.hip': {
        'train_cond_layer_fwd_kernel': (82, 16, 53760), 'train_cond_layer_bwd_kernel<true>': (208, 0, 53760),
        'train_cond_layer_bwd_kernel<false>': (254, 0, 62080)},
    'pwv_train_skip.hip': {
        'train_skip_layer_fwd_kernel<pwv::UniformGeo>': (102, 16, 41472), 'train_skip_layer_fwd_kernel<pwv::PackedGeo>': (104, 16, 42000),
        'train_skip_head_fwd_kernel': (53, 16, 33024), 'train_skip_head_bwd_kernel': (117, 80, 33152),
        'train_skip_layer_bwd_kernel<pwv::UniformGeo, true>': (188, 0, 57984), 'train_skip_layer_bwd_kernel<pwv::PackedGeo, true>': (190, 0, 58512),
        'train_skip_layer_bwd_kernel<pwv::UniformGeo, false>': (236, 0, 66304), 'train_skip_layer_bwd_kernel<pwv::PackedGeo, false>': (240, 0, 66832)},
}


@pytest.mark.parametrize('source', sorted(RECORD))
def test_older_training_kernels_compile_to_their_recorded_resources(source):
    """Every kernel of the older training files has the registers and LDS of the project's record: the new file shares their headers
    and changed none of their instantiations."""
    res = kernel_resources(source)
    short = {re.sub(r'^(void )?pwv::', '', n).split('(')[0]: r for n, r in res.items()}
    assert sorted(short) == sorted(RECORD[source]), sorted(short)
    for name, want in RECORD[source].items():
        r = short[name]
        assert (r['vgprs'], r['agprs'], r['lds']) == want and r['scratch'] == 0 and r['vgpr_spills'] == 0 and r['sgpr_spills'] == 0, (name, r)


def _model(cfg, N=TO.N, T=TO.T, precision='f32'):
    from pwv_amd.models import IAFVocoder
    from pwv_amd.variables import VariableStore
    set_hparams(cfg)
    return IAFVocoder(N, T, store=VariableStore(device='cpu'), precision=precision)


def test_refusal_table():
    """A bare call refuses the shared hparams with the word "shared" and says how to ask; the request is accepted -- uniform, packed,
    with a power weight, fused, with skip connections (both requests), with transposed-conv conditioning --; a request under hparams
    that say False is a mismatch; any other value is refused by name; every other refusal stands under the request."""
    from pwv_amd import train as TR
    from pwv_amd._lib import PwvError
    from pwv_amd.hparam import hparam as hp
    cfg = SO.small_cfg()
    try:
        model = _model(cfg)
        bare = TR.refusal(model)
        assert 'shared' in bare and 'shared_nets=True' in bare
        assert 'shared' in TR.refusal(model, packed=True)
        assert TR.refusal(model, shared_nets=True) is None and TR.refusal(model, packed=True, shared_nets=True) is None
        hp.signal.win_length = 48
        assert TR.refusal(model, power_weight=0.5, shared_nets=True) is None
        assert 'shared_nets False' in TR.refusal(model, shared_nets=False) and "shared_nets 'yes'" in TR.refusal(model, shared_nets='yes')
        with pytest.raises(TypeError):
            TR.refusal(model, None, None, None, False, None, True)              # keyword-only
        wav, mel = torch.zeros(TO.N, TO.T), torch.zeros(TO.N, 1 + TO.T // TO.HOP, 80)
        with pytest.raises(PwvError, match='training refused.*shared'):
            TR.loss_and_grad(model, wav, mel)
        with pytest.raises(PwvError, match='training refused.*shared'):
            TR.loss_and_grad_varlen(model, [wav[0]], [mel[0]])
        with pytest.raises(PwvError, match='training refused.*shared'):
            TR.Trainer(model)._bind()
        tr = TR.Trainer(model, shared_nets=True)
        assert tr._bind() and len(tr.names) == SO.TOTAL and TR.Trainer(model, shared_nets=True, fused=True).shared_nets
        assert all('/shared/' in n or '/cond/' in n for n in tr.names)
        # every other refusal is what it was
        assert 'f16x3' in TR.refusal(_model(cfg, precision='f16x3'), shared_nets=True)
        hp.model.normalize_wavenet = 'bn'
        assert "'bn'" in TR.refusal(model, shared_nets=True)
        hp.model.normalize_wavenet = None
        hp.model.residual_channels = 32
        assert 'fused shape' in TR.refusal(model, shared_nets=True)
        hp.model.residual_channels = 64
        # with skip connections: both requests
        model = _model(SO.small_cfg(skip=True))
        assert 'skip accumulation' in TR.refusal(model, shared_nets=True) and 'shared' in TR.refusal(model, use_skip_connection=True)
        assert TR.refusal(model, use_skip_connection=True, shared_nets=True) is None
        assert TR.refusal(model, packed=True, use_skip_connection=True, shared_nets=True) is None
        # a mismatch: the request under hparams with two nets per flow
        model = _model(TO.small_cfg())
        why = TR.refusal(model, shared_nets=True)
        assert 'does not match' in why and TR.refusal(model) is None
        with pytest.raises(PwvError, match='training refused.*does not match'):
            TR.loss_and_grad(model, wav, mel, shared_nets=True)
        with pytest.raises(PwvError, match='training refused.*does not match'):
            TR.loss_and_grad_varlen(model, [wav[0]], [mel[0]], shared_nets=True)
        with pytest.raises(PwvError, match='training refused.*does not match'):
            TR.Trainer(model, shared_nets=True)._bind()
        # transposed-conv conditioning: uniform at hop 80; packed and together with skip still refused
        model = _model(SO.small_cfg(80, tran=True), 2, 160)
        assert 'shared' in TR.refusal(model) and TR.refusal(model, shared_nets=True) is None
        assert 'uniform' in TR.refusal(model, packed=True, shared_nets=True)
        model = _model(SO.small_cfg(80, skip=True, tran=True), 2, 160)
        assert 'transposed_conv' in TR.refusal(model, use_skip_connection=True, shared_nets=True)
    finally:
        hp.set_hparam_yaml('default')


def test_oracle_counts_and_central_differences():
    """The small shared model has 91 variables, 75 with a gradient (with skip connections 87): the ones without are skip / skip_bias of
    every layer but the last and dense / dense_bias of the last (with skip: those alone).  float64 autograd of both columns of one
    postprocess2, both entries of one postprocess2_bias and one gc_gate below against central differences of the restatement's own
    loss at h = 1e-6, to 1e-6 relative + 1e-9, as tests/test_train_host.py does."""
    cfg, w, mel, z, wav = SO.problem()
    g64 = SO.reference()['g64']
    dead = sorted(k for k, v in g64.items() if v is None)
    assert len(g64) == SO.TOTAL == 91 and len(dead) == SO.DEAD == 16
    assert dead == sorted(['iaf_vocoder/iaf%d/shared/dilated_stack/layer%d/%s' % (i, j, role) for i in (0, 1) for j in (0, 1, 2)
                           for role in ('skip', 'skip_bias')]
                          + ['iaf_vocoder/iaf%d/shared/dilated_stack/layer3/%s' % (i, role) for i in (0, 1) for role in ('dense', 'dense_bias')])
    skip = SO.reference(skip=True)['g64']
    assert len(skip) == 91 and sorted(k for k, v in skip.items() if v is None) == sorted(
        'iaf_vocoder/iaf%d/shared/dilated_stack/layer3/%s' % (i, role) for i in (0, 1) for role in ('dense', 'dense_bias'))
    assert len(skip) - SO.DEAD_SKIP == 87
    post2, b2, gc = ('iaf_vocoder/iaf1/shared/postprocessing/postprocess2', 'iaf_vocoder/iaf0/shared/postprocessing/postprocess2_bias',
                     'iaf_vocoder/iaf0/shared/dilated_stack/layer1/gc_gate')
    assert w[post2].shape == (1, 128, 2) and w[b2].shape == (2,)
    W64 = {k: v.astype(np.float64) for k, v in w.items()}

    def loss(name, idx, delta):
        W = dict(W64)
        W[name] = W64[name].copy()
        W[name][idx] += delta
        return SO.loss_only(W, mel, z, wav, cfg)

    rng = np.random.RandomState(1)
    top = lambda a: [int(p) for p in np.argsort(np.abs(a).ravel())[-2:]]
    points = [(post2, (0, c, q)) for q in (0, 1) for c in top(g64[post2][0, :, q]) + [int(rng.randint(128))]]
    points += [(b2, (0,)), (b2, (1,))]
    points += [(gc, np.unravel_index(p, g64[gc].shape)) for p in top(g64[gc]) + [int(rng.randint(g64[gc].size))]]
    h = 1e-6
    for name, idx in points:
        assert np.abs(g64[name]).max() > 0, name
        fd = (loss(name, idx, h) - loss(name, idx, -h)) / (2 * h)
        assert abs(fd - g64[name][idx]) <= 1e-6 * np.abs(g64[name]).max() + 1e-9, (name, idx, fd, g64[name][idx])
    assert np.abs(g64[post2][0, :, 0] - g64[post2][0, :, 1]).max() > 0 and g64[b2][0] != g64[b2][1]


def test_head_restatement_is_the_model_level_head():
    """The kernel-level restatement in both modes from first principles at one row, and its SKIPSUM column sums."""
    c = SO.head_case(3, 80)
    for mode in (SO.GATED, SO.SKIPSUM):
        r = SO.shared_head(c, mode, torch.float64)
        row = 77
        h1 = np.maximum(c['o'][row].astype(np.float64) @ c['skip'][0] + c['skip_bias'], 0) if mode == SO.GATED else np.maximum(c['S'][row], 0).astype(np.float64)
        y = np.maximum(h1 @ c['post1'][0].astype(np.float64) + c['post1_bias'], 0) @ c['post2'][0].astype(np.float64) + c['post2_bias']
        assert np.allclose([r['y0'][row], r['y1'][row]], y, rtol=1e-12, atol=1e-12)
        assert np.allclose(r['post2_bias'], [(c['d_out'].astype(np.float64) * c['d_mul']).sum(), c['d_out'].astype(np.float64).sum()])
        nb = SO.shared_head(c, mode, torch.float64, biased=False)
        assert 'post1_bias' not in nb and not np.allclose(nb['y0'], r['y0'])
    assert np.allclose(SO.shared_head(c, SO.SKIPSUM, torch.float64)['skip_bias'], SO.shared_head(c, SO.SKIPSUM, torch.float64)['dS'].sum(axis=0))


def test_small_shared_case_loads_and_names_its_checkpoint(tmp_path):
    """hparams/hparams.yaml has train/small_shared = train/small with shared_nets True; `refusal` lets the request through; Trainer.save
    writes 'iaf_vocoder/iafK/shared/...' and a FRESH VariableStore under the same hparams loads that .npz, `use_ema` picking the
    shadows."""
    from pwv_amd import train as TR
    from pwv_amd.hparam import hparam as hp
    from pwv_amd.models import IAFVocoder
    from pwv_amd.variables import EMA_SUFFIX, VariableStore
    keys = ('n_iaf', 'dilations', 'condition_channels', 'cond_upsample_method', 'use_skip_connection')
    try:
        hp.set_hparam_yaml('train/small')
        small = {k: hp.model.get(k) for k in keys}, int(hp.signal.length), int(hp.train.batch_size), dict(hp.generate)
        assert not hp.model.get('shared_nets')
        hp.set_hparam_yaml('train/small_shared')
        assert hp.model.shared_nets is True and hp.data_path == 'synthetic'
        assert ({k: hp.model.get(k) for k in keys}, int(hp.signal.length), int(hp.train.batch_size), dict(hp.generate)) == small
        assert 'shared' in TR.refusal() and TR.refusal(shared_nets=True) is None and TR.refusal(packed=True, shared_nets=True) is None
        store = VariableStore(device='cpu')
        tr = TR.Trainer(IAFVocoder(2, 800, store=store, precision='f32'), shared_nets=True)
        tr._bind()
        assert len(tr.names) == (1 + 4 * 10 + 4) + (1 + 5 * 10 + 4) + 1
        assert sum('/shared/' in n for n in tr.names) == len(tr.names) - 1 and not any('/scalar/' in n or '/shifter/' in n for n in tr.names)
        path = str(tmp_path / 'model-0.npz')
        tr.save(path)
        with np.load(path) as zf:
            data = {k: zf[k] for k in zf.files}
        assert 'iaf_vocoder/iaf1/shared/postprocessing/postprocess2' + EMA_SUFFIX in data
        assert data['iaf_vocoder/iaf0/shared/postprocessing/postprocess2'].shape == (1, 128, 2)
        # shadows that differ from the variables, so that the choice shows
        for k in list(data):
            if k.endswith(EMA_SUFFIX):
                data[k] = data[k] + np.float32(0.25)
        moved = str(tmp_path / 'moved.npz')
        np.savez(moved, **data)
        name = 'iaf_vocoder/iaf0/shared/postprocessing/postprocess2_bias'
        for use_ema, want in ((False, data[name]), (True, data[name + EMA_SUFFIX])):
            fresh = VariableStore(device='cpu')
            fresh.load_npz(moved, use_ema=use_ema)
            model = IAFVocoder(1, 1600, store=fresh, precision='f32')
            TR.model_nets(model, fresh)
            assert np.array_equal(fresh.vars[name].numpy(), want) and fresh.vars[name].shape == (2,)
            assert sorted(n for n in TR.trainable_names(fresh)) == tr.names
    finally:
        hp.set_hparam_yaml('default')
