"""CPU: what streaming a transposed-conv model (IAFVocoder.open_stream(slots, transposed_conv=True), include/pwv_hip_stream_cond.h,
csrc/pwv_layer_stream_cond.hip) settles without a device: the compiler's resource remarks for the six kernels, the extension header and
every refusal of its entry point, the request and what is still refused, the engine's keyword next to its unchanged defaults, and the
gather arithmetic of a ragged chunk restated in numpy.  tests/test_gpu_stream_cond.py runs the routes."""
import ctypes
import os
import re
import subprocess
import tempfile
from types import SimpleNamespace

import numpy as np
import pytest

from tests.util import hop_cfg, set_hparams, small_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = 'pwv_wavenet_layer_stream_cond_f32'


def test_six_kernels_without_scratch():
    """Three forms per arithmetic (layer 0 folded, a residual layer, the gated last layer): no scratch, no spilled register, no dynamic
    stack, at most 256 VGPRs at 512 threads, LDS (a layer's weights with gc_filter|gc_gate, the unit counter, layer 0's causal filter)
    within the CU's 160 KB."""
    from tests.util import kernel_resources
    res = kernel_resources('pwv_layer_stream_cond.hip')
    for name, r in sorted(res.items()):
        print(name, r)
        assert r['scratch'] == 0 and r['vgpr_spills'] == 0 and r['sgpr_spills'] == 0 and not r['dynamic_stack'], (name, r)
        assert r['vgprs'] <= 256 and r['lds'] <= 160 * 1024, (name, r)
    assert len(res) == 6, sorted(res)
    for kernel in ('layer_f16x3_stream_cond_kernel', 'layer_f32_stream_cond_kernel'):
        assert sorted(re.search(r'<(\w+, \w+)>', n).group(1) for n in res if kernel + '<' in n) == ['false, false', 'false, true', 'true, false'], sorted(res)


def test_header_is_c99_and_declares_the_entry(built_lib):
    """The extension header compiles as C99 with every warning an error, declares exactly _lib.STREAM_COND_SYMBOLS, disjoint from every older
    list; the library exports it; pwv_hip.h keeps its version and its 52 symbols."""
    from pwv_amd import _lib
    src = ('#include "pwv_hip_stream_cond.h"\nint main(void){ int (*f)(const pwv_layer_args*, const pwv_stream_args*, pwv_stream_t) = '
           + ENTRY + '; return f == 0 || PWV_HIP_VERSION != 301; }\n')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 't.c')
        with open(c, 'w') as f:
            f.write(src)
        subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Wextra', '-pedantic', '-Werror', '-c', '-I' + os.path.join(ROOT, 'include'), c,
                               '-o', os.path.join(d, 't.o')])
    code = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'pwv_hip_stream_cond.h')).read(), flags=re.S)
    assert sorted(set(re.findall(r'\b(pwv_[a-z0-9_]+)\s*\(', code))) == sorted(_lib.STREAM_COND_SYMBOLS) == [ENTRY]
    older = [_lib.EXPORTED_SYMBOLS, _lib.EXTENSION_SYMBOLS, _lib.LIVE_TICK_SYMBOLS, _lib.SCORE_SYMBOLS, _lib.TRAIN_SYMBOLS, _lib.TRAIN_LOSS_SYMBOLS,
             _lib.TRAIN_VARLEN_SYMBOLS, _lib.TRAIN_COND_SYMBOLS, _lib.TRAIN_OPT_SYMBOLS, _lib.TRAIN_SKIP_SYMBOLS, _lib.TRAIN_SHARED_SYMBOLS]
    assert not set(_lib.STREAM_COND_SYMBOLS) & set().union(*older) and len(_lib.EXPORTED_SYMBOLS) == 52
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), ENTRY) and built_lib.pwv_version() == 301
    assert os.path.join(_lib._PKG_DIR, 'csrc', 'pwv_layer_stream_cond.hip') in _lib.CSRC


def _args():
    """A residual layer j >= 1 that passes every check of the entry (made-up pointers: nothing is dereferenced on the host)."""
    from pwv_amd import _lib
    la, sa = _lib.LayerArgs(), _lib.StreamArgs()
    la.G, la.N, la.T, la.dilation, la.precision = 1, 1, 80, 4, _lib.PREC_F16X3
    la.cond, la.cond_channels = 4096, 80
    la.x_in[0], la.x_out[0], la.packed[0], la.proj[0] = 4096, 8192, 4096, 4096
    sa.hist_rd = sa.hist_wr = sa.slot_tab = 4096
    sa.block_stride = 32 * 64
    return la, sa


def test_entry_refusals_no_gpu(built_lib):
    """Every refusal of pwv_wavenet_layer_stream_cond_f32 comes before anything touches a device, with its words; arguments that pass them
    all reach the launcher (which finds no device here, or launches nothing it could: this test runs without a GPU)."""
    from pwv_amd import _lib
    lib = built_lib
    call = lambda la, sa: lib.pwv_wavenet_layer_stream_cond_f32(ctypes.byref(la), ctypes.byref(sa), None)

    def refused(la, sa, words):
        rc, err = call(la, sa), lib.pwv_last_error()
        assert rc == -1 and words in err and ENTRY.encode() in err, (rc, err, words)

    la, sa = _args()
    sa.struct_size = 0
    refused(la, sa, b'struct_size')
    la, sa = _args()
    sa.hist_rd = None
    refused(la, sa, b'NULL history')
    la, sa = _args()
    la.precision = _lib.PREC_F16
    refused(la, sa, b'fp16 storage')
    la, sa = _args()
    la.skip[0] = 4096
    refused(la, sa, b'skip accumulation')
    la, sa = _args()
    la.cond = None
    refused(la, sa, b'cond is NULL')
    la, sa = _args()
    la.cond_channels = 96
    refused(la, sa, b'supports 80 channels, got 96')
    la, sa = _args()
    la.x_first = 4096                                  # layer 0 without its fold
    refused(la, sa, b'folded form')
    la, sa = _args()
    la.head_packed[0], la.head_out[0], la.head_q, la.out_mode = 4096, 4096, 1, _lib.OUT_GATED
    refused(la, sa, b'no fused head')
    la, sa = _args()
    la.dilation = 33                                   # round32(33) = 64 rows do not fit a block of 32
    refused(la, sa, b'leave the history block')
    la, sa = _args()
    la.x_first, la.first_fold[0], la.causal_filter[0], la.dilation = 4096, 4096, 4096, 32 * 64      # d + 1 scalars do not fit either
    refused(la, sa, b'scalars leave the history block')
    la, sa = _args()
    la.x_first, la.first_fold[0], la.causal_filter[0], la.out_mode = 4096, 4096, 4096, _lib.OUT_GATED
    refused(la, sa, b'PWV_OUT_GATED for a last layer that is not layer 0')
    # the older entry still turns a per-sample condition and a gated output away, in its words
    la, sa = _args()
    assert lib.pwv_wavenet_layer_stream_f32(ctypes.byref(la), ctypes.byref(sa), None) == -1 and b'per-sample' in lib.pwv_last_error()
    la.cond, la.cond_channels, la.out_mode = None, 0, _lib.OUT_GATED
    assert lib.pwv_wavenet_layer_stream_f32(ctypes.byref(la), ctypes.byref(sa), None) == -1 and b'PWV_OUT_RESIDUAL' in lib.pwv_last_error()
    try:
        import torch
        if torch.cuda.is_available():
            return          # (with a device the accepted call below would launch on made-up pointers)
    except ImportError:
        pass
    for mode in (_lib.OUT_RESIDUAL, _lib.OUT_GATED):
        la, sa = _args()
        la.out_mode = mode
        rc, err = call(la, sa), lib.pwv_last_error()
        assert rc != 0 and b'no HIP device' in err, (rc, err)


def _model():
    from pwv_amd.models import IAFVocoder
    from pwv_amd.variables import VariableStore
    store = VariableStore(device='cpu')
    return IAFVocoder(batch_size=1, length=80, store=store), store


def _tconv(hop=80, **kw):
    return hop_cfg(hop, cond_upsample_method='transposed_conv', **kw)


def test_the_request_and_the_bare_call():
    """The bare call under transposed_conv hparams is refused in the words tests/test_gpu_stream.py pins; the request is accepted -- the
    histories of a CPU store stand in for the device's: the frame geometry, the layout (two nets per flow, one for shared_nets) and the
    session state are those of a 'repeat' stream -- and plans nothing; under 'repeat' hparams the request is a mismatch."""
    from pwv_amd._lib import PwvError
    from pwv_amd.stream import HistoryLayout
    cfg = _tconv()
    set_hparams(cfg)
    model, store = _model()
    with pytest.raises(PwvError, match='transposed-conv'):
        model.open_stream(slots=2)
    s = model.open_stream(slots=2, transposed_conv=True)
    assert s.per_sample and s.hop == 80 and s.n_slots == 2 and len(store.vars) == 0
    assert s.layout.block_floats == HistoryLayout(cfg.dilations).block_floats and s.state_bytes() == 2 * 4 * s.layout.block_floats + 4 * 80
    set_hparams(_tconv(shared_nets=True))
    s1 = model.open_stream(slots=1, transposed_conv=True)
    assert s1.per_sample and s1.layout.block_floats == HistoryLayout(cfg.dilations, nets_per_flow=1).block_floats
    set_hparams(hop_cfg(80))
    with pytest.raises(PwvError, match="does not match these hparams.*'repeat'"):
        model.open_stream(slots=2, transposed_conv=True)
    assert not model.open_stream(slots=2).per_sample


@pytest.mark.parametrize('case', ['normalize_cond', 'skip', 'f16', 'in', 'normalize_wavenet', 'hop', 'shape'])
def test_still_refused_with_the_request(case):
    from pwv_amd._lib import PwvError
    from pwv_amd.models import IAFVocoder
    kw, hop, precision = {}, 80, None
    if case == 'normalize_cond':
        kw, reason = dict(normalize_cond='bn'), 'a normaliser'
    elif case == 'skip':
        kw, reason = dict(use_skip_connection=True), 'skip accumulation'
    elif case == 'f16':
        precision, reason = 'f16', "precision 'f16'"
    elif case == 'in':
        kw, reason = dict(normalize='in'), 'instance normalisation'
    elif case == 'normalize_wavenet':
        kw, reason = dict(normalize_wavenet='bn'), 'a normaliser'
    elif case == 'hop':
        hop, reason = 96, 'hop_length 96'
    else:
        reason = 'outside the fused shape'
    cfg = _tconv(hop, **kw) if case != 'shape' else small_cfg(dilations=[[1], [1, 2]], cond_upsample_method='transposed_conv')
    set_hparams(cfg)
    model, store = _model()
    model = IAFVocoder(batch_size=1, length=80, store=store, precision=precision)
    with pytest.raises(PwvError, match=reason):
        model.open_stream(slots=2, transposed_conv=True)
    assert len(store.vars) == 0


def test_graph_wrappers_refuse_by_name():
    """graphed / graphed_varlen / graphed_live (and the graph classes themselves) name per-sample conditioning before anything is captured;
    the stream's state is untouched."""
    from pwv_amd import graph
    from pwv_amd._lib import PwvError
    set_hparams(_tconv())
    model, _ = _model()
    s = model.open_stream(slots=2, transposed_conv=True)
    for make in (lambda: s.graphed(2, 1), lambda: s.graphed_varlen(2, 160), lambda: s.graphed_live(None, 2, 160),
                 lambda: graph.GraphedStream(s, 2, 1), lambda: graph.GraphedRaggedStream(s, 2, 160)):
        with pytest.raises(PwvError, match='per-sample .transposed-conv. conditioning'):
            make()
    assert s._ticker is None and s._pending is None and s._running == [False, False]


def _net(out_channels, skip=False, dilations=(1, 2, 4, 8), cc=80):
    return SimpleNamespace(dilations=list(dilations), use_skip_connection=skip, in_channels=1, out_channels=out_channels, condition_channels=cc,
                           filter_width=2, precision=None, normalize=None, fused_supported=lambda cond: cond is None or cc == 80)


def test_engine_keyword_next_to_unchanged_defaults():
    """stream_refusal / _flow_structure on fake nets: the defaults answer as before (a per-sample condition is 'samples'); per_sample=True
    accepts that condition on the same flow shapes, keeps skip / f16 / shape, and turns a frame-rate condition (or none) away."""
    from pwv_amd import engine
    why = engine._STREAM_STRUCTURE_WHY
    cond = object()          # anything that is no RepeatedCondition: a per-sample condition
    two, one = [_net(1), _net(1)], [_net(2)]
    # defaults, word for word
    assert engine.stream_refusal(one, None) is None and engine.stream_refusal(two, None) is None
    assert engine.stream_refusal(two, cond) == why['samples'] == 'per-sample (transposed-conv) conditioning'
    assert engine._flow_structure(two, cond) == 'samples' and engine._flow_structure(two, None) is None
    assert engine.stream_refusal([_net(1)], None) == why['shape'] and engine.stream_refusal([_net(2, skip=True)], None) == why['skip']
    assert engine.stream_refusal(one, None, 'f16') == why['f16']
    assert engine._VARLEN_STRUCTURE_WHY['samples'] == 'per-sample conditioning'
    # the keyword
    assert engine.stream_refusal(two, cond, per_sample=True) is None and engine.stream_refusal(one, cond, per_sample=True) is None
    assert engine.stream_refusal(two, cond, 'f32', per_sample=True) is None
    assert engine.stream_refusal(two, None, per_sample=True) == why['frames']
    assert engine.stream_refusal([_net(2, skip=True)], cond, per_sample=True) == why['skip']
    assert engine.stream_refusal(two, cond, 'f16', per_sample=True) == why['f16']
    assert engine.stream_refusal([_net(1)], cond, per_sample=True) == why['shape']
    assert engine.stream_refusal([_net(2, dilations=(1,))], cond, per_sample=True) == why['shape']
    assert engine.stream_refusal([_net(1, cc=64), _net(1, cc=64)], cond, per_sample=True) == why['shape']      # channels the kernels do not take
    assert engine.stream_refusal(two, engine.PackedSampleCondition(np.zeros((160, 80)), 80), per_sample=True) is None


def test_ragged_gather_equals_the_per_session_crop():
    """A ragged tick of frame counts [1, 3, 2, 5], fresh and running sessions mixed.  The stage GEMMs run once over the packed frames, and
    stage output row hop f + r depends on packed frame f alone; a session whose frames start at cu_frames[i] and that yields T_i samples
    reads rows hop cu_frames[i] + hop / 2 + s, s < T_i, of that uncropped output (engine.ragged_cond_rows) -- exactly what the one-shot
    crop [hop/2 : -hop/2] (models.py:124) of the session's OWN T_i / hop + 1 frames gives.  One crop of the packed tensor is wrong from
    the second session on: every session owns one frame more than T_i / hop."""
    from pwv_amd import engine
    from pwv_amd.stream import ragged_plan
    hop, C = 80, 3
    counts, fresh = [1, 3, 2, 5], [True, False, True, False]
    plan = ragged_plan(counts, fresh, hop)
    assert plan.samples == [0, 240, 80, 400] and plan.launch == [1, 2, 3]
    assert plan.cu_frames == [0, 4, 6, 12] and plan.cu_rows == [0, 240, 320, 720]
    rng = np.random.default_rng(0)
    frames = rng.standard_normal((plan.cu_frames[-1], C))
    phase = rng.standard_normal((hop, C))
    full = (frames[:, None, :] * phase[None]).reshape(-1, C)          # "a transposed conv of width == stride": row hop f + r from frame f
    seen = []
    for k, i in enumerate(plan.launch):
        t = plan.samples[i]
        rows = engine.ragged_cond_rows(plan.cu_frames[k], t, hop)
        assert len(rows) == t and rows[0] == hop * plan.cu_frames[k] + hop // 2 and rows[-1] < hop * plan.cu_frames[k + 1] - hop // 2 + 1
        own = (frames[plan.cu_frames[k]:plan.cu_frames[k + 1], None, :] * phase[None]).reshape(-1, C)          # the session alone
        assert own.shape[0] == t + hop
        assert np.array_equal(full[rows], own[hop // 2:hop // 2 + t])
        # sample s is conditioned on the session's frame (s + hop / 2) // hop
        assert np.array_equal(rows // hop - plan.cu_frames[k], (np.arange(t) + hop // 2) // hop)
        seen.append(rows)
    packed_crop = full[hop // 2:hop // 2 + plan.cu_rows[-1]]
    assert np.array_equal(packed_crop[:240], full[seen[0]]) and not np.array_equal(packed_crop[240:320], full[seen[1]])
