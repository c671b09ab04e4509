"""CPU: training the transposed-conv conditioning (include/pwv_hip_train_cond.h, csrc/pwv_train_cond.hip, train.refusal and the
per-sample branch of train.py) -- the C struct against its ctypes mirror, the header's symbols, every host refusal, the kernels'
resources, the table of what `refusal` lets through, the oracle against central differences, and the hparams case.  Nothing here needs
a GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import train_cond_oracle as CO
from tests.util import kernel_resources, set_hparams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYER_PART = 128 * 128 + 64 * 64 + 64
HEAD_PART = 64 * 128 + 128 + 128 * 128 + 128 + 128 + 1


def test_cond_args_layout_matches_ctypes(tmp_path):
    """The C compiler's size and offsets of pwv_train_cond_args (gcc -std=c99 -pedantic -Werror) against the ctypes mirror: the embedded
    pwv_train_args first, its fields where pwv_train_args has them, then the condition."""
    from pwv_amd import _lib
    mirror = _lib.TrainCondArgs
    fields = [n for n, _ in mirror._fields_]
    old = [n for n, _ in _lib.TrainArgs._fields_]
    assert fields == old + ['cond', 'gc_filter', 'gc_gate', 'filter_bias', 'gate_bias', 'd_cond', 'd_gc_filter', 'd_gc_gate', 'd_filter_bias',
                            'd_gate_bias', 'cond_channels', 'cond_row_stride', 'cond_utt_rows', 'd_cond_accumulate']
    c_name = lambda f: 'train.' + ('in' if f == 'in_' else f) if f in old else f
    probe = (['sizeof(pwv_train_cond_args)'] + ['offsetof(pwv_train_cond_args, %s)' % c_name(f) for f in fields]
             + ['sizeof(pwv_train_args)', '(size_t)PWV_TRAIN_COND_MAX', '(size_t)PWV_HIP_VERSION'])
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "pwv_hip_train_cond.h"\nint main(void){ printf("%s\\n", %s); return 0; }\n'
           % (' '.join(['%zu'] * len(probe)), ', '.join(probe)))
    c, exe = str(tmp_path / 'cond.c'), str(tmp_path / 'cond')
    with open(c, 'w') as f:
        f.write(src)
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Wextra', '-pedantic', '-Werror', '-I' + os.path.join(ROOT, 'include'), c, '-o', exe])
    got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    assert got == ([ctypes.sizeof(mirror)] + [getattr(mirror, f).offset for f in fields]
                   + [ctypes.sizeof(_lib.TrainArgs), _lib.TRAIN_COND_MAX, 301])
    assert all(getattr(mirror, f).offset == getattr(_lib.TrainArgs, f).offset for f in old)
    assert mirror().struct_size == ctypes.sizeof(mirror) and _lib.TRAIN_COND_MAX == 96


def test_header_declares_exactly_the_new_symbols():
    """include/pwv_hip_train_cond.h declares exactly _lib.TRAIN_COND_SYMBOLS, the library exports them, the older lists are what they
    were, and pwv_hip.h keeps its version."""
    from pwv_amd import _lib
    _lib.build_library()
    code = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'pwv_hip_train_cond.h')).read(), flags=re.S)
    assert sorted(set(re.findall(r'\b(pwv_[a-z0-9_]+)\s*\(', code))) == sorted(_lib.TRAIN_COND_SYMBOLS) == [
        'pwv_train_cond_layer_bwd_f32', 'pwv_train_cond_layer_fwd_f32', 'pwv_train_cond_workspace_bytes']
    older = [_lib.EXPORTED_SYMBOLS, _lib.EXTENSION_SYMBOLS, _lib.LIVE_TICK_SYMBOLS, _lib.SCORE_SYMBOLS, _lib.TRAIN_SYMBOLS, _lib.TRAIN_LOSS_SYMBOLS,
             _lib.TRAIN_VARLEN_SYMBOLS]
    assert [len(s) for s in older] == [52, 1, 2, 2, 7, 2, 6]
    assert not set(_lib.TRAIN_COND_SYMBOLS) & set().union(*older)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(raw, name) for name in _lib.TRAIN_COND_SYMBOLS)
    raw.pwv_version.restype = ctypes.c_int
    assert raw.pwv_version() == 301 and '#define PWV_HIP_VERSION 301' in open(os.path.join(ROOT, 'include', 'pwv_hip.h')).read()
    assert os.path.join(os.path.dirname(_lib.__file__), 'csrc', 'pwv_train_cond.hip') in _lib.CSRC


def _args(**kw):
    """A pwv_train_cond_args the library accepts up to its launch: every device pointer a number that is never dereferenced on the host."""
    from pwv_amd import _lib
    a = _lib.TrainCondArgs(N=2, T=200, dilation=1, next_dilation=1, max_workgroups=3, cond_channels=80, cond_row_stride=80, cond_utt_rows=280)
    for f in ('x', 'x_out', 'filter', 'gate', 'dense', 'u_next', 'v_next', 'd_o', 'd_filter', 'd_gate', 'd_dense', 'workspace', 'cond', 'gc_filter',
              'gc_gate', 'd_cond', 'd_gc_filter', 'd_gc_gate'):
        setattr(a, f, 4096)
    a.u, a.v = 8192, 12288
    a.workspace_bytes = 1 << 40
    for k, v in kw.items():
        setattr(a, k, v)
    return a


ENTRIES = ('pwv_train_cond_layer_fwd_f32', 'pwv_train_cond_layer_bwd_f32')


def test_cond_calls_refuse_bad_arguments_on_the_host(built_lib):
    """Every refusal of the two entry points returns -1 (PWV_EINVAL) with its field named, before anything touches a device (this
    process has none); the workspace is grid x max(head partial, layer partial + C 128 + 128) floats."""
    from pwv_amd import _lib
    lib = built_lib

    def refused(name, a, word):
        code = getattr(lib, name)(ctypes.byref(a) if a is not None else None, None)
        msg = lib.pwv_last_error().decode()
        assert code == -1 and word in msg and name in msg, (name, code, word, msg)

    for name in ENTRIES:
        refused(name, None, 'NULL')
        refused(name, _args(cond=None), 'cond is a NULL')
        for C in (81, 0, 1, 98, -2):
            refused(name, _args(cond_channels=C, cond_row_stride=128), 'cond_channels %d' % C)
        refused(name, _args(cond_row_stride=79), 'cond_row_stride 79')
        refused(name, _args(cond_utt_rows=199), 'cond_utt_rows 199')
        refused(name, _args(cond_utt_rows=2 ** 30), 'cond_utt_rows')
        refused(name, _args(proj=4096), 'proj')
        refused(name, _args(d_proj=4096), 'd_proj')
        refused(name, _args(gc_gate=None), 'gc_gate')
        refused(name, _args(x=None), 'NULL')
        refused(name, _args(N=0), 'N = 0')
        refused(name, _args(T=2 ** 30, cond_utt_rows=2 ** 30), 'beyond int32')
        refused(name, _args(dilation=0), 'dilation')
        refused(name, _args(form=2), 'form')
        refused(name, _args(max_workgroups=-1), 'max_workgroups')
        a = _args()
        a.struct_size = ctypes.sizeof(_lib.TrainArgs)           # (the uniform struct is no per-sample one)
        refused(name, a, 'struct_size')
    refused(ENTRIES[0], _args(x_out=None), 'x_out')
    refused(ENTRIES[0], _args(dense=None), 'dense')
    bwd = ENTRIES[1]
    refused(bwd, _args(d_cond=None), 'd_cond')
    refused(bwd, _args(d_gc_filter=None), 'd_gc_filter')
    refused(bwd, _args(u=4096), 'alias')
    refused(bwd, _args(form=_lib.TRAIN_LAST, d_o=None), 'd_o')
    refused(bwd, _args(workspace=None), 'workspace')
    refused(bwd, _args(workspace_bytes=3 * (LAYER_PART + 80 * 128 + 128) * 4 - 1), 'workspace_bytes')
    refused(bwd, _args(cond_channels=34, workspace_bytes=3 * (LAYER_PART + 34 * 128 + 128) * 4 - 1), 'workspace_bytes')
    for C in (80, 34, 2, 96):
        want = 3 * max(HEAD_PART, LAYER_PART + C * 128 + 128) * 4
        assert lib.pwv_train_cond_workspace_bytes(ctypes.byref(_args(cond_channels=C))) == want, C
        assert want >= lib.pwv_train_workspace_bytes(ctypes.byref(_lib.TrainArgs(N=2, T=200, max_workgroups=3)))
    assert LAYER_PART + 80 * 128 + 128 > HEAD_PART > LAYER_PART + 2 * 128 + 128
    assert lib.pwv_train_cond_workspace_bytes(ctypes.byref(_args(cond_channels=81))) == 0 and 'cond_channels' in lib.pwv_last_error().decode()
    assert lib.pwv_train_cond_workspace_bytes(None) == 0


def test_cond_kernel_resources():
    """The compiler's resource remarks (gfx950 device code) for the three kernels of csrc/pwv_train_cond.hip: no scratch, no spilled
    register, static LDS alone (the launches request no dynamic LDS) and within the 64 KiB a kernel may declare: the backward holds
    [x[t-d] | x[t]] and FG at 32 x 129, g and the aliased d o / o at 32 x 65 and the condition tile at 32 x 97.  Two workgroups fit the
    160 KiB and the 512 registers per lane and SIMD of a compute unit, as the default grid of two per compute unit assumes."""
    res = kernel_resources('pwv_train_cond.hip')
    names = ' '.join(res)
    for k in ('train_cond_layer_fwd_kernel', 'train_cond_layer_bwd_kernel<true>', 'train_cond_layer_bwd_kernel<false>'):
        assert k in names, (k, names)
    assert len(res) == 3
    for name, r in res.items():
        assert r['scratch'] == 0 and r['vgpr_spills'] == 0 and r['sgpr_spills'] == 0 and not r['dynamic_stack'], (name, r)
        assert r['lds'] <= 64 * 1024 and 2 * r['lds'] <= 160 * 1024, (name, r)
        assert r['vgprs'] + r['agprs'] <= 256, (name, r)         # two waves per SIMD: two workgroups of four waves per compute unit
    by = lambda k: next(r for n, r in res.items() if k in n)
    tile = 4 * 32 * 97
    assert by('bwd_kernel<false>')['lds'] <= 4 * 32 * (2 * 129 + 2 * 65) + tile + 128
    assert by('fwd_kernel')['lds'] <= 4 * 32 * (2 * 129 + 65) + tile + 128
    src = open(os.path.join(ROOT, 'parallel-wavenet-vocoder_amd', 'csrc', 'pwv_train_cond.hip')).read()
    assert 'atomic' not in src.lower() and src.count('dim3(kTrThreads), 0,') == 3          # no atomics; dynamic LDS 0 at every launch


REFUSAL_TABLE = [
    ('hop80', dict(), {}, None),
    ('hop16', dict(hop_length=16), {}, 'hop_length 16: the strides (4, 4, 5) multiply to 80'),
    ('packed', dict(), dict(packed=True), 'not packed'),
    ('c97', dict(condition_channels=97), {}, 'condition_channels'),
    ('c98', dict(condition_channels=98), {}, 'condition_channels'),
    ('odd_c', dict(condition_channels=35), {}, 'condition_channels'),
    ('normalize_cond', dict(normalize_cond='bn'), {}, 'normalize_cond'),
]


@pytest.mark.parametrize('case', REFUSAL_TABLE, ids=[c[0] for c in REFUSAL_TABLE])
def test_refusal_table(case):
    """transposed_conv is accepted at hop 80 with an even condition_channels <= 96, no normalised conditioning, not packed; every other
    case is refused with "transposed" and its reason, by loss_and_grad / loss_and_grad_varlen too, before a device is touched."""
    from pwv_amd import train as TR
    from pwv_amd._lib import PwvError
    from pwv_amd.hparam import hparam as hp
    from pwv_amd.models import IAFVocoder
    from pwv_amd.variables import VariableStore
    _, cfg_kw, extra, word = case
    kw = dict(dilations=[[1, 2, 32, 64], [4, 48, 256, 3]], n_iaf=2, hop_length=80, cond_upsample_method='transposed_conv')
    kw.update(cfg_kw)
    set_hparams(type(CO.small_cfg())(**kw))
    hop = kw['hop_length']
    try:
        model = IAFVocoder(CO.N, CO.T, store=VariableStore(device='cpu'), precision='f32')
        why = TR.refusal(model, **extra)
        if word is None:
            hp.signal.win_length = CO.WIN
            assert why is None and TR.refusal(model, power_weight=0.5) is None
            assert 'f16x3' in TR.refusal(IAFVocoder(CO.N, CO.T, store=VariableStore(device='cpu'), precision='f16x3'))
            hp.model.use_skip_connection = True
            assert 'skip accumulation' in TR.refusal(model)
            return
        assert 'transposed' in why and word in why, why
        wav, mel = torch.zeros(CO.N, CO.T), torch.zeros(CO.N, 1 + CO.T // hop, 80)
        with pytest.raises(PwvError, match='training refused.*transposed'):
            if extra.get('packed'):
                TR.loss_and_grad_varlen(model, [wav[0], wav[1, :160]], [mel[0], mel[1, :3]])
            else:
                TR.loss_and_grad(model, wav, mel)
        if extra.get('packed'):
            assert 'not packed' in TR.refusal(model, [wav[0]], [mel[0]])
    finally:
        hp.set_hparam_yaml('default')


def test_other_upsample_methods_stay_refused():
    from pwv_amd import train as TR
    from pwv_amd.hparam import hparam as hp
    hp.set_hparam_yaml('default')
    hp.model.cond_upsample_method = 'none'
    try:
        assert "'none'" in TR.refusal()
    finally:
        hp.set_hparam_yaml('default')


def test_oracle_against_central_differences():
    """float64 autograd of the restatement against central differences of its own loss on a handful of entries of the three
    transposed-conv weights and of gc weights and biases: (L(w + h) - L(w - h)) / 2h at h = 1e-6 agrees to 1e-6 relative + 1e-9 (the
    loss is piecewise smooth; the ReLU condition keeps every kink farther than h times any weight's reach)."""
    cfg, w, mel, z, wav = CO.problem()
    assert CO.relu_margin(w, mel, cfg) >= CO.RELU_MARGIN
    g64 = CO.reference()['g64']
    names = ['iaf_vocoder/cond/transposed_conv_%d_weights' % i for i in range(3)]
    names += ['iaf_vocoder/iaf0/scalar/dilated_stack/layer1/gc_filter', 'iaf_vocoder/iaf1/shifter/dilated_stack/layer3/gc_gate',
              'iaf_vocoder/iaf1/scalar/dilated_stack/layer0/filter_bias']
    assert [w['iaf_vocoder/cond/transposed_conv_%d_weights' % i].shape for i in range(3)] == [(1, 4, 80, 80), (1, 4, 80, 80), (1, 5, 80, 80)]
    rng = np.random.RandomState(1)
    W64 = {k: v.astype(np.float64) for k, v in w.items()}

    def loss(name, idx, delta):
        W = dict(W64)
        W[name] = W64[name].copy()
        W[name][idx] += delta
        with torch.no_grad():
            T = {k: torch.from_numpy(v) for k, v in W.items()}
            pred = CO.forward(T, torch.from_numpy(mel).double(), torch.from_numpy(z).double(), cfg)
            return float((pred - torch.from_numpy(wav).double()).abs().mean())

    h = 1e-6
    for name in names:
        assert g64[name] is not None and np.abs(g64[name]).max() > 0, name
        # the entries with the largest gradients and two drawn ones
        flat = np.abs(g64[name]).ravel()
        picks = list(np.argsort(flat)[-2:]) + list(rng.randint(0, flat.size, 2))
        for p in picks:
            idx = np.unravel_index(int(p), g64[name].shape)
            fd = (loss(name, idx, h) - loss(name, idx, -h)) / (2 * h)
            assert abs(fd - g64[name][idx]) <= 1e-6 * np.abs(g64[name]).max() + 1e-9, (name, idx, fd, g64[name][idx])


def test_small_tran_case_loads():
    """hparams/hparams.yaml has train/small_tran = train/small with transposed-conv conditioning; `refusal` lets it through, and its
    variables are the three transposed-conv weights in place of cond/dense."""
    from pwv_amd import train as TR
    from pwv_amd.hparam import hparam as hp
    from pwv_amd.models import IAFVocoder
    from pwv_amd.variables import VariableStore
    try:
        hp.set_hparam_yaml('train/small')
        small = {k: hp.model.get(k) for k in ('n_iaf', 'dilations', 'condition_channels')}, int(hp.signal.length), int(hp.train.batch_size)
        hp.set_hparam_yaml('train/small_tran')
        assert hp.model.cond_upsample_method == 'transposed_conv' and hp.data_path == 'synthetic' and int(hp.signal.hop_length) == 80
        assert ({k: hp.model.get(k) for k in ('n_iaf', 'dilations', 'condition_channels')}, int(hp.signal.length), int(hp.train.batch_size)) == small
        assert TR.refusal() is None and 'not packed' in TR.refusal(packed=True)
        store = VariableStore(device='cpu')
        tr = TR.Trainer(IAFVocoder(2, 800, store=store, precision='f32'))
        tr._bind()
        cond = [n for n in tr.names if '/cond/' in n]
        assert cond == ['iaf_vocoder/cond/transposed_conv_%d_weights' % i for i in range(3)]
        assert [tuple(store.vars[n].shape) for n in cond] == [(1, 4, 80, 80), (1, 4, 80, 80), (1, 5, 80, 80)]
    finally:
        hp.set_hparam_yaml('default')
