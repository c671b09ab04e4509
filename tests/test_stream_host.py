"""CPU: the host side of streaming generation (stream.py, pwv_stream_args) -- the C ABI additions, the push-length and history
index arithmetic restated in numpy, and the compiler's resource remarks for the streaming kernels.  No GPU needed."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_stream_entry_points(built_lib):
    from pwv_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'pwv_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name in ('pwv_wavenet_layer_stream_f32', 'pwv_stream_carry_f32'):
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert '#define PWV_HIP_VERSION 301' in text and _lib.HEADER_VERSION == 301 and built_lib.pwv_version() == 301
    assert 'typedef struct pwv_stream_args' in code


def test_stream_args_size_matches_ctypes():
    from pwv_amd import _lib
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "pwv_hip.h"\nint main(void){ printf("%zu %zu %zu\\n", sizeof(pwv_stream_args), '
           'offsetof(pwv_stream_args, slot_tab), offsetof(pwv_stream_args, carry_tab)); return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, 't.c'), os.path.join(d, 't')
        with open(c, 'w') as f:
            f.write(src)
        subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Wextra', '-pedantic', '-Werror', '-I' + os.path.join(ROOT, 'include'), c, '-o', exe])
        sizes = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    assert sizes == [ctypes.sizeof(_lib.StreamArgs), _lib.StreamArgs.slot_tab.offset, _lib.StreamArgs.carry_tab.offset]
    assert _lib.StreamArgs().struct_size == ctypes.sizeof(_lib.StreamArgs)


def test_stream_argument_validation_no_gpu(built_lib):
    """Every refusal of the streaming entry points comes before anything touches a device."""
    from pwv_amd import _lib
    lib = built_lib
    la, sa = _lib.LayerArgs(), _lib.StreamArgs()
    la.G, la.N, la.T, la.dilation, la.precision = 1, 1, 80, 4, _lib.PREC_F16X3
    sa.struct_size = 0
    assert lib.pwv_wavenet_layer_stream_f32(ctypes.byref(la), ctypes.byref(sa), None) == -1 and b'struct_size' in lib.pwv_last_error()
    sa = _lib.StreamArgs()
    assert lib.pwv_wavenet_layer_stream_f32(ctypes.byref(la), ctypes.byref(sa), None) == -1 and b'NULL history' in lib.pwv_last_error()
    sa.hist_rd = sa.hist_wr = sa.slot_tab = 4096      # (never dereferenced on the host)
    sa.block_stride = 32 * 64
    la.precision = _lib.PREC_F16
    assert lib.pwv_wavenet_layer_stream_f32(ctypes.byref(la), ctypes.byref(sa), None) == -1 and b'fp16 storage' in lib.pwv_last_error()
    la.precision = _lib.PREC_F16X3
    la.skip[0] = 4096
    assert lib.pwv_wavenet_layer_stream_f32(ctypes.byref(la), ctypes.byref(sa), None) == -1 and b'skip accumulation' in lib.pwv_last_error()
    la.skip[0] = None
    la.cond, la.cond_channels = 4096, 80
    assert lib.pwv_wavenet_layer_stream_f32(ctypes.byref(la), ctypes.byref(sa), None) == -1 and b'per-sample' in lib.pwv_last_error()
    la.cond, la.cond_channels = None, 0
    la.dilation = 33                                   # round32(33) = 64 rows do not fit a block of 32
    assert lib.pwv_wavenet_layer_stream_f32(ctypes.byref(la), ctypes.byref(sa), None) == -1 and b'leave the history block' in lib.pwv_last_error()
    la.dilation = 4
    la.x_first = 4096                                  # layer 0 without its fold
    assert lib.pwv_wavenet_layer_stream_f32(ctypes.byref(la), ctypes.byref(sa), None) == -1 and b'folded form' in lib.pwv_last_error()
    la.x_first = None
    la.out_mode = _lib.OUT_GATED                       # gated output without the fused head
    assert lib.pwv_wavenet_layer_stream_f32(ctypes.byref(la), ctypes.byref(sa), None) == -1 and b'PWV_OUT_RESIDUAL' in lib.pwv_last_error()
    assert lib.pwv_stream_carry_f32(ctypes.byref(sa), 1, 80, None) == -1 and b'carry_tab' in lib.pwv_last_error()


def test_push_length_arithmetic():
    from pwv_amd.stream import push_samples
    hop = 80
    assert push_samples(1, True, hop) == 0 and push_samples(5, True, hop) == 320 and push_samples(5, False, hop) == 400
    for schedule in ([1, 1, 1, 7], [21], [5, 5, 5, 5, 1], [2, 19]):
        total = sum(push_samples(f, k == 0, hop) for k, f in enumerate(schedule))
        assert total == (sum(schedule) - 1) * hop      # an utterance of F frames yields (F - 1) * hop samples, however it is cut
        # the frames a push conditions on: the kept frame (the last one of the push before) in front of its own
        first = 0
        for k, f in enumerate(schedule):
            lo, hi = (first if k == 0 else first - 1), first + f
            assert hi - lo == push_samples(f, k == 0, hop) // hop + 1
            first += f


@pytest.mark.parametrize('d', [1, 2, 5, 32, 96])
def test_history_index_arithmetic(d):
    """"The history of a layer after a schedule = the last d rows of the layer's input", with the kernels' index arithmetic restated
    (stream.history_sources): chunks shorter than, equal to and longer than the dilation.  The look-back of chunk row t < d is
    history row t; layer 0's scalar history has d + 1 entries and is read at d (x[t-1], t = 0), t + 1 (x[t-d]) and t (x[t-d-1])."""
    from pwv_amd.stream import advance_history, history_sources
    rng = np.random.default_rng(d)
    x = rng.standard_normal(6 * d + 40)
    for length in (d, d + 1):                          # a row history; the scalar history of a layer 0 with this dilation
        hist, pos = np.zeros(length), 0
        schedule = [max(d - 1, 1), d, d + 3, 1, 2 * d + 1, 1, 1, max(d // 2, 1)]
        for T in schedule:
            chunk = x[pos:pos + T]
            padded = np.concatenate([np.zeros(length), x])           # padded[length + t] = x[t]; zeros left of the utterance
            for t in range(min(T, length)):
                if length == d:
                    assert hist[t] == padded[length + pos + t - d]                   # x[t - d]
                else:
                    if t < d:
                        assert hist[t + 1] == padded[length + pos + t - d]           # x[t - d]
                    assert hist[t] == padded[length + pos + t - d - 1]               # x[t - d - 1]
                    if t == 0:
                        assert hist[d] == padded[length + pos - 1]                   # x[-1]
            new = np.array([hist[i] if kind == 'carry' else chunk[i] for kind, i in history_sources(length, T)])
            assert np.array_equal(new, advance_history(hist, chunk))
            hist, pos = new, pos + T
            assert np.array_equal(hist, padded[pos:pos + length])                    # the last `length` inputs
    kinds = [k for k, _ in history_sources(8, 3)]
    assert kinds == ['carry'] * 5 + ['chunk'] * 3 and history_sources(8, 8) == [('chunk', t) for t in range(8)]


def test_history_layout_is_disjoint_and_bounded():
    from oracle import iaf_oracle as O
    from pwv_amd.stream import HistoryLayout, round32
    dil = O.ModelConfig().dilations
    lay = HistoryLayout(dil)
    spans = sorted((off, off + (rows if width == 1 else round32(rows) * 64)) for off, rows, width in lay.carry)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= lay.block_floats
    assert all(off % 4 == 0 for off, _, _ in lay.carry)
    assert len(lay.carry) == len(dil) + 2 * sum(len(d) - 1 for d in dil) and lay.max_rows == 512
    layers = [d for dl in dil for d in dl] * 2
    assert 2 * lay.block_floats * 4 <= 2 * sum(round32(d) for d in layers) * 256 + (64 << 10)


def test_streaming_kernels_use_no_scratch():
    """The compiler's resource remarks (gfx950 device code, as tests/test_host_logic.py::test_no_vgpr_spills_in_the_layer_kernels reads
    them) for the streaming instantiations: no scratch, no spilled register -- three forms in each arithmetic, and the carry-over."""
    from tests.util import kernel_resources
    seen = []
    for src in ('pwv_layer_f16.hip', 'pwv_layer.hip'):
        for name, r in kernel_resources(src).items():
            if 'stream' not in name:
                continue
            seen.append(name)
            assert r['scratch'] == 0 and r['vgpr_spills'] == 0 and r['sgpr_spills'] == 0, (name, r)
            assert r['vgprs'] <= 256, (name, r)
    assert len(seen) == 7 and sum('layer_f16x3_stream_kernel' in n for n in seen) == 3 and sum('layer_f32_stream_kernel' in n for n in seen) == 3, seen
