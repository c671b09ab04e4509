"""CPU: what streaming a skip-connection model (IAFVocoder.open_stream(slots, use_skip_connection=True), include/pwv_hip_stream_skip.h,
csrc/pwv_layer_stream_skip.hip) settles without a device: the compiler's resource remarks for the new kernels, the extension header and
every refusal of its entry points, the engine's keyword next to its unchanged defaults, the request and what is still refused, and the
history layout -- unchanged for the models that streamed before, with a row history and one scalar for layer 0 of a skip stream.
tests/test_gpu_stream_skip.py runs the routes."""
import ctypes
import os
import re
import subprocess
import tempfile
from types import SimpleNamespace

import pytest

from tests.util import hop_cfg, set_hparams, small_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY, FRONT = 'pwv_wavenet_layer_stream_skip_f32', 'pwv_iaf_front_stream_f32'


def test_five_kernels_without_scratch():
    """Two forms per arithmetic (a residual layer, the gated last layer) and the streaming front: no scratch, no spilled register, no
    dynamic stack, at most 256 VGPRs at 512 threads, LDS (a layer's weights with the skip section and the unit counter) within 160 KB."""
    from tests.util import kernel_resources
    res = kernel_resources('pwv_layer_stream_skip.hip')
    for name, r in sorted(res.items()):
        print(name, r)
        assert r['scratch'] == 0 and r['vgpr_spills'] == 0 and r['sgpr_spills'] == 0 and not r['dynamic_stack'], (name, r)
        assert r['vgprs'] <= 256 and r['lds'] <= 160 * 1024, (name, r)
    assert len(res) == 5, sorted(res)
    for kernel in ('layer_f16x3_stream_skip_kernel', 'layer_f32_stream_skip_kernel'):
        assert sorted(re.search(r'<(\w+)>', n).group(1) for n in res if kernel + '<' in n) == ['false', 'true'], sorted(res)
    assert any('stream_front_kernel' in n for n in res)


def test_header_is_c99_and_declares_the_entries(built_lib):
    """The extension header compiles as C99 with every warning an error and declares exactly _lib.STREAM_SKIP_SYMBOLS, disjoint from every
    older list; the library exports them; pwv_hip.h keeps its version and its 52 symbols."""
    from pwv_amd import _lib
    src = ('#include "pwv_hip_stream_skip.h"\nint main(void){ int (*f)(const pwv_layer_args*, const pwv_stream_args*, pwv_stream_t) = '
           + ENTRY + '; int (*g)(const float*, int, const float* const*, float* const*, int, int, const pwv_stream_args*, pwv_stream_t) = '
           + FRONT + '; return f == 0 || g == 0 || PWV_HIP_VERSION != 301; }\n')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 't.c')
        with open(c, 'w') as f:
            f.write(src)
        subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Wextra', '-pedantic', '-Werror', '-c', '-I' + os.path.join(ROOT, 'include'), c,
                               '-o', os.path.join(d, 't.o')])
    code = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'pwv_hip_stream_skip.h')).read(), flags=re.S)
    assert sorted(set(re.findall(r'\b(pwv_[a-z0-9_]+)\s*\(', code))) == sorted(_lib.STREAM_SKIP_SYMBOLS) == sorted([ENTRY, FRONT])
    older = [_lib.EXPORTED_SYMBOLS, _lib.EXTENSION_SYMBOLS, _lib.LIVE_TICK_SYMBOLS, _lib.SCORE_SYMBOLS, _lib.TRAIN_SYMBOLS, _lib.TRAIN_LOSS_SYMBOLS,
             _lib.TRAIN_VARLEN_SYMBOLS, _lib.TRAIN_COND_SYMBOLS, _lib.TRAIN_OPT_SYMBOLS, _lib.TRAIN_SKIP_SYMBOLS, _lib.TRAIN_SHARED_SYMBOLS,
             _lib.STREAM_COND_SYMBOLS]
    assert not set(_lib.STREAM_SKIP_SYMBOLS) & set().union(*older) and len(_lib.EXPORTED_SYMBOLS) == 52
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(cdll, ENTRY) and hasattr(cdll, FRONT) and built_lib.pwv_version() == 301
    assert os.path.join(_lib._PKG_DIR, 'csrc', 'pwv_layer_stream_skip.hip') in _lib.CSRC


def _args(G=1):
    """A residual layer that passes every check of the entry (made-up pointers: nothing is dereferenced on the host)."""
    from pwv_amd import _lib
    la, sa = _lib.LayerArgs(), _lib.StreamArgs()
    la.G, la.N, la.T, la.dilation, la.precision = G, 1, 80, 4, _lib.PREC_F16X3
    for g in range(G):
        la.x_in[g], la.x_out[g], la.packed[g], la.proj[g], la.skip[g] = 4096, 8192, 4096, 4096, 4096
        sa.row_off[g] = g * 32 * 64
    sa.hist_rd = sa.hist_wr = sa.slot_tab = 4096
    sa.block_stride = G * 32 * 64
    return la, sa


def _no_device():
    try:
        import torch
        return not torch.cuda.is_available()
    except ImportError:
        return True


def test_entry_refusals_no_gpu(built_lib):
    """Every refusal of pwv_wavenet_layer_stream_skip_f32 comes before anything touches a device, with its words; arguments that pass them
    all reach the launcher (which finds no device here).  The two older streaming entries still refuse `skip` in their old words."""
    from pwv_amd import _lib
    lib = built_lib
    call = lambda la, sa: lib.pwv_wavenet_layer_stream_skip_f32(ctypes.byref(la), ctypes.byref(sa), None)

    def refused(la, sa, words):
        rc, err = call(la, sa), lib.pwv_last_error()
        assert rc == -1 and words in err and ENTRY.encode() in err, (rc, err, words)

    la, sa = _args()
    assert lib.pwv_wavenet_layer_stream_skip_f32(None, ctypes.byref(sa), None) == -1 and b'args is NULL' in lib.pwv_last_error()
    assert lib.pwv_wavenet_layer_stream_skip_f32(ctypes.byref(la), None, None) == -1 and b'args is NULL' in lib.pwv_last_error()
    sa.struct_size = 0
    refused(la, sa, b'struct_size does not cover the history fields')
    la, sa = _args()
    sa.struct_size = _lib.StreamArgs.row_off.offset          # ends in front of the offsets
    refused(la, sa, b'struct_size does not cover the history fields')
    la, sa = _args()
    sa.hist_rd = None
    refused(la, sa, b'NULL history')
    la, sa = _args()
    sa.slot_tab = None
    refused(la, sa, b'slot table')
    la, sa = _args()
    sa.cu_rows = 4096
    refused(la, sa, b'hist->cu_rows is set')
    la, sa = _args()
    la.precision = _lib.PREC_F16
    refused(la, sa, b'fp16 storage')
    la, sa = _args()
    la.skip[0] = None
    refused(la, sa, b'skip[0] is NULL')
    la, sa = _args(2)
    la.skip[1] = None
    refused(la, sa, b'skip[1] is NULL')
    la, sa = _args()
    la.cond, la.cond_channels = 4096, 80
    refused(la, sa, b'per-sample condition (cond / cond_channels)')
    la, sa = _args()
    la.cond_channels = 80
    refused(la, sa, b'per-sample condition (cond / cond_channels)')
    la, sa = _args()
    la.head_packed[0], la.head_out[0], la.head_q, la.out_mode = 4096, 4096, 1, _lib.OUT_GATED
    refused(la, sa, b'no fused head with skip accumulation (head_packed)')
    la, sa = _args()
    la.first_fold[0] = 4096
    refused(la, sa, b'first_fold is set')
    la, sa = _args()
    la.x_first, la.causal_filter[0] = 4096, 4096
    refused(la, sa, b'x_first is set')
    la, sa = _args()
    la.dilation = 33                                   # round32(33) = 64 rows do not fit a block of 32
    refused(la, sa, b'leave the history block')
    la, sa = _args()
    sa.row_off[0] = 2                                  # no multiple of 4
    refused(la, sa, b'leave the history block')
    la, sa = _args(2)
    sa.row_off[1] = 16 * 64                            # inside net 0's 32 rows
    refused(la, sa, b"the nets' row histories overlap")
    # the older entries still turn skip accumulation away, in their words
    la, sa = _args()
    assert lib.pwv_wavenet_layer_stream_f32(ctypes.byref(la), ctypes.byref(sa), None) == -1
    assert b'pwv_wavenet_layer_stream_f32: skip accumulation has no streaming form' in lib.pwv_last_error()
    la.cond, la.cond_channels = 4096, 80
    assert lib.pwv_wavenet_layer_stream_cond_f32(ctypes.byref(la), ctypes.byref(sa), None) == -1
    assert b'pwv_wavenet_layer_stream_cond_f32: skip accumulation has no streaming form' in lib.pwv_last_error()
    if not _no_device():
        return          # (with a device the accepted calls below would launch on made-up pointers)
    for mode, G in ((_lib.OUT_RESIDUAL, 1), (_lib.OUT_GATED, 1), (_lib.OUT_RESIDUAL, 2)):
        la, sa = _args(G)
        la.out_mode = mode
        rc, err = call(la, sa), lib.pwv_last_error()
        assert rc != 0 and b'no HIP device' in err, (rc, err)


def test_front_refusals_no_gpu(built_lib):
    from pwv_amd import _lib
    lib = built_lib
    _, sa = _args()
    two = (ctypes.c_void_p * 2)(4096, 4096)

    def front(x, G, filt, h, n, t, sa):
        return lib.pwv_iaf_front_stream_f32(x, G, filt, h, n, t, None if sa is None else ctypes.byref(sa), None), lib.pwv_last_error()

    for bad, words in (((None, 1, two, two, 1, 80, sa), b'NULL pointer'), ((4096, 1, two, two, 1, 80, None), b'args is NULL'),
                       ((4096, 3, two, two, 1, 80, sa), b'bad G'), ((4096, 1, two, two, 1, 0, sa), b'bad G / N / T'),
                       ((4096, 2, (ctypes.c_void_p * 2)(4096, None), two, 1, 80, sa), b'NULL filter / output for net 1')):
        rc, err = front(*bad)
        assert rc == -1 and words in err and FRONT.encode() in err, (rc, err, words)
    _, sa = _args()
    sa.cu_rows = 4096
    rc, err = front(4096, 1, two, two, 1, 80, sa)
    assert rc == -1 and b'cu_rows' in err
    _, sa = _args()
    sa.scalar_off = sa.block_stride
    rc, err = front(4096, 1, two, two, 1, 80, sa)
    assert rc == -1 and b'leaves the history block' in err


def _net(out_channels, skip=False, dilations=(1, 2, 4, 8), cc=80):
    return SimpleNamespace(dilations=list(dilations), use_skip_connection=skip, in_channels=1, out_channels=out_channels, condition_channels=cc,
                           filter_width=2, precision=None, normalize=None, fused_supported=lambda cond: cond is None or cc == 80)


def test_engine_keyword_next_to_unchanged_defaults():
    """stream_refusal / _flow_structure / run_flow_stream on fake nets: the defaults answer as before ('skip' for a skip net); skip=True
    accepts skip nets on both flow shapes, names nets without skip accumulation as the mismatch, keeps f16 / shape / samples, and is
    refused together with per_sample=True."""
    from pwv_amd import _lib, engine
    why = engine._STREAM_STRUCTURE_WHY
    cond = object()          # anything that is no RepeatedCondition: a per-sample condition
    two, one = [_net(1), _net(1)], [_net(2)]
    two_s, one_s = [_net(1, skip=True), _net(1, skip=True)], [_net(2, skip=True)]
    # defaults, word for word
    assert engine.stream_refusal(one, None) is None and engine.stream_refusal(two, None) is None
    assert engine.stream_refusal(one_s, None) == why['skip'] == 'skip accumulation (use_skip_connection)'
    assert engine.stream_refusal(two_s, None) == why['skip'] and engine._flow_structure(two_s, None) == 'skip'
    assert engine.stream_refusal(one_s, cond, per_sample=True) == why['skip']
    assert engine.stream_refusal(two, cond) == why['samples'] and engine.stream_refusal(one, None, 'f16') == why['f16']
    assert engine._VARLEN_STRUCTURE_WHY['skip'] == 'skip accumulation'
    # the keyword
    assert engine.stream_refusal(two_s, None, skip=True) is None and engine.stream_refusal(one_s, None, skip=True) is None
    assert engine.stream_refusal(two_s, None, 'f32', skip=True) is None and engine._flow_structure(one_s, None, skip=True) is None
    assert engine.stream_refusal(two, None, skip=True) == why['noskip'] and 'does not match' in why['noskip']
    assert engine.stream_refusal(one, None, skip=True) == why['noskip'] and engine._flow_structure(two, None, skip=True) == 'noskip'
    assert engine.stream_refusal(two_s, cond, skip=True) == why['samples']
    assert engine.stream_refusal(two_s, None, 'f16', skip=True) == why['f16']
    assert engine.stream_refusal([_net(1, skip=True)], None, skip=True) == why['shape']
    assert engine.stream_refusal([_net(2, skip=True, dilations=(1,))], None, skip=True) == why['shape']
    both = engine.stream_refusal(two_s, cond, skip=True, per_sample=True)
    assert both is not None and 'skip=True together with per_sample=True' in both
    # run_flow_stream raises the same words before it touches its tensors
    for nets, kw, words in ((two, dict(skip=True), 'does not match'), (two_s, dict(skip=True, per_sample=True), 'together with per_sample=True'),
                            (two_s, {}, 'skip accumulation .use_skip_connection.')):
        with pytest.raises(_lib.PwvError, match='no streaming form: .*' + words):
            engine.run_flow_stream(nets, None, None, None, None, 0, None, **kw)


def _model(precision=None):
    from pwv_amd.models import IAFVocoder
    from pwv_amd.variables import VariableStore
    store = VariableStore(device='cpu')
    return IAFVocoder(batch_size=1, length=80, store=store, precision=precision), store


def test_the_request_and_the_bare_call():
    """The bare call under skip hparams is refused in the words tests/test_gpu_stream.py pins; the request is accepted (a CPU store stands in
    for the device's histories) and plans nothing; with shared_nets it is one net per flow; under hparams without the switch the request
    is a mismatch; together with transposed_conv=True it is refused by name."""
    from pwv_amd._lib import PwvError
    from pwv_amd.stream import HistoryLayout
    cfg = hop_cfg(80, use_skip_connection=True)
    set_hparams(cfg)
    model, store = _model()
    with pytest.raises(PwvError, match=r'skip accumulation \(use_skip_connection: True\): the per-layer kernels stream without skip sums only'):
        model.open_stream(slots=2)
    s = model.open_stream(slots=2, use_skip_connection=True)
    assert s.skip and not s.per_sample and s.hop == 80 and s.n_slots == 2 and len(store.vars) == 0
    assert s.layout.block_floats == HistoryLayout(cfg.dilations, skip=True).block_floats
    assert s.state_bytes() == 2 * 4 * s.layout.block_floats + 4 * 80
    set_hparams(hop_cfg(80, use_skip_connection=True, shared_nets=True))
    s1 = model.open_stream(slots=1, use_skip_connection=True)
    assert s1.skip and s1.layout.block_floats == HistoryLayout(cfg.dilations, nets_per_flow=1, skip=True).block_floats
    assert all(len(per_net) == 1 for per_net in s1.layout.row_off)
    set_hparams(hop_cfg(80))
    with pytest.raises(PwvError, match=r'open_stream\(use_skip_connection=True\) does not match these hparams'):
        model.open_stream(slots=2, use_skip_connection=True)
    assert not model.open_stream(slots=2).skip
    set_hparams(hop_cfg(80, use_skip_connection=True, cond_upsample_method='transposed_conv'))
    with pytest.raises(PwvError, match='use_skip_connection=True together with transposed_conv=True'):
        model.open_stream(slots=2, use_skip_connection=True, transposed_conv=True)
    with pytest.raises(PwvError, match='skip accumulation'):          # (the pinned refusal of the transposed-conv request alone)
        model.open_stream(slots=2, transposed_conv=True)
    assert len(store.vars) == 0


@pytest.mark.parametrize('case', ['f16', 'in', 'normalize_wavenet', 'normalize_cond', 'shape'])
def test_still_refused_with_the_request(case):
    from pwv_amd._lib import PwvError
    kw, precision = {}, None
    if case == 'f16':
        precision, reason = 'f16', "precision 'f16'"
    elif case == 'in':
        kw, reason = dict(normalize='in'), 'instance normalisation'
    elif case == 'normalize_wavenet':
        kw, reason = dict(normalize_wavenet='bn'), 'a normaliser'
    elif case == 'normalize_cond':
        kw, reason = dict(normalize_cond='bn'), 'a normaliser'
    else:
        reason = 'outside the fused shape'
    cfg = hop_cfg(80, use_skip_connection=True, **kw) if case != 'shape' else small_cfg(dilations=[[1], [1, 2]], use_skip_connection=True)
    set_hparams(cfg)
    model, store = _model(precision)
    with pytest.raises(PwvError, match=reason):
        model.open_stream(slots=2, use_skip_connection=True)
    assert len(store.vars) == 0


def test_graph_wrappers_refuse_by_name():
    """graphed / graphed_varlen / graphed_live (and the graph classes themselves) name skip accumulation before anything is captured; the
    stream's state is untouched."""
    from pwv_amd import graph
    from pwv_amd._lib import PwvError
    set_hparams(hop_cfg(80, use_skip_connection=True))
    model, _ = _model()
    s = model.open_stream(slots=2, use_skip_connection=True)
    for make in (lambda: s.graphed(2, 1), lambda: s.graphed_varlen(2, 160), lambda: s.graphed_live(None, 2, 160),
                 lambda: graph.GraphedStream(s, 2, 1), lambda: graph.GraphedRaggedStream(s, 2, 160)):
        with pytest.raises(PwvError, match=r'skip accumulation \(use_skip_connection\) streams on per-layer launches only'):
            make()
    assert s._ticker is None and s._pending is None and s._running == [False, False]


def _parent_layout(dilations, nets_per_flow=2):
    """HistoryLayout as it was before skip streams existed, restated: per flow d0 + 1 scalars padded to 64 floats, then per net and layer
    j >= 1 round32(d_j) rows x 64."""
    scalar_off, row_off, carry, off = [], [], [], 0
    for dil in dilations:
        scalar_off.append(off)
        carry.append((off, dil[0] + 1, 1))
        off += (dil[0] + 1 + 63) // 64 * 64
        per_net = []
        for _ in range(nets_per_flow):
            offs = [-1]
            for d in dil[1:]:
                offs.append(off)
                carry.append((off, d, 64))
                off += (d + 31) // 32 * 32 * 64
            per_net.append(offs)
        row_off.append(per_net)
    return scalar_off, row_off, carry, off


def test_history_layout():
    """The default and the shared-net layouts are what they were, offset for offset (the README's state sizes at the default dilations:
    6,949,184 B and 3,475,776 B per session with the 80-float kept frame); the skip layout keeps ONE scalar per flow and a row history
    for layer 0 of every net, both in the carry table, nothing overlapping."""
    from pwv_amd.stream import HistoryLayout, round32
    from oracle import iaf_oracle as O
    default = [list(d) for d in O.ModelConfig().dilations]          # the architecture of bench/c2: the default dilations, largest 512
    odd = [[1, 96, 128, 256], [3, 64, 200, 512, 2, 160], [96, 1, 40]]
    for dil in (default, odd):
        for npf in (2, 1):
            lay, (so, ro, ca, total) = HistoryLayout(dil, nets_per_flow=npf), _parent_layout(dil, npf)
            assert lay.scalar_off == so and lay.row_off == ro and lay.carry == ca and lay.block_floats == total
            assert lay.max_rows == max(r for _, r, _ in ca)
    assert 2 * 4 * HistoryLayout(default).block_floats + 4 * 80 == 6949184
    assert 2 * 4 * HistoryLayout(default, nets_per_flow=1).block_floats + 4 * 80 == 3475776
    for npf in (2, 1):
        lay = HistoryLayout(odd, nets_per_flow=npf, skip=True)
        spans = []
        for i, dil in enumerate(odd):
            assert (lay.scalar_off[i], 1, 1) in lay.carry          # x[-1] of the streaming front
            spans.append((lay.scalar_off[i], 64))
            assert len(lay.row_off[i]) == npf
            for g in range(npf):
                assert len(lay.row_off[i][g]) == len(dil)
                for j, d in enumerate(dil):
                    off = lay.row_off[i][g][j]
                    assert off >= 0 and off % 4 == 0 and (off, d, 64) in lay.carry          # layer 0's entry among them
                    spans.append((off, round32(d) * 64))
        assert len(lay.carry) == len(spans)
        spans.sort()
        assert spans[0][0] == 0 and all(a + n == b for (a, n), (b, _) in zip(spans, spans[1:]))
        assert spans[-1][0] + spans[-1][1] == lay.block_floats
        assert lay.max_rows == 512
    # a skip block is larger than the default block by the layer-0 rows and smaller by the d0 scalars it does not keep
    grow = sum(2 * round32(d[0]) * 64 + 64 - (d[0] + 1 + 63) // 64 * 64 for d in odd)
    assert HistoryLayout(odd, skip=True).block_floats == HistoryLayout(odd).block_floats + grow


def test_state_of_another_layout_is_turned_away():
    """state / load_state between a skip stream and a default stream of the same dilations: block_floats differ, the state is refused."""
    cfg = hop_cfg(80, use_skip_connection=True)
    set_hparams(cfg)
    model, _ = _model()
    s = model.open_stream(slots=1, use_skip_connection=True)
    st = s.state(0)
    s.load_state(0, st)
    set_hparams(hop_cfg(80))
    plain = model.open_stream(slots=1)
    assert plain.layout.block_floats != s.layout.block_floats
    with pytest.raises(ValueError, match='another shape'):
        plain.load_state(0, st)
    with pytest.raises(ValueError, match='another shape'):
        s.load_state(0, plain.state(0))
