"""CPU: per-utterance noise streams of packed batches and the graph replay of packed batches -- the filler layout of
graph.GraphedPackedVocoder, the checks of `seeds` / `offsets`, and the packed sampler's C entry point (declared, exported, built, no
scratch).  No GPU needed."""
import ctypes
import os
import re

import pytest
import torch

from oracle import iaf_oracle as O
from tests.util import set_hparams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _capacity(slots, rows, hop=80):
    """A GraphedPackedVocoder's layout rule without a capture (fits / _layout read only these fields)."""
    from pwv_amd import _lib
    from pwv_amd.graph import GraphedPackedVocoder
    g = GraphedPackedVocoder.__new__(GraphedPackedVocoder)
    g.hop, g.slots, g.rows = hop, slots, rows
    g.filler = hop * -(-max(hop, _lib.VARLEN_MIN_ROWS) // hop)
    return g


def test_filler_layout():
    g = _capacity(4, 32000)
    assert g.filler == 80
    assert g._layout([16000, 8000, 4000, 4000]) == [16000, 8000, 4000, 4000]        # exact fit: no filler
    assert g._layout([16000, 4000]) == [16000, 4000, 80, 11920]                     # one hop, then the remaining rows
    assert g._layout([80]) == [80, 80, 80, 31760]
    assert g._layout([16000, 8000, 7840]) == [16000, 8000, 7840, 160]
    assert g._layout([31760]) == [31760, 80, 80, 80]                                # the last filler is one hop too: the limit
    assert g.fits([31760]) and not g.fits([31840])                                  # 31840 + 3 fillers of 80 > 32000
    assert not g.fits([16000, 8000, 4000, 4080]) and not g.fits([16000, 8000, 4000, 3920])    # 4 slots: exactly 32000 rows
    assert not g.fits([80] * 5)                                                     # more utterances than slots
    assert not g.fits([]) and not g.fits([8000, 4040])                              # none; not a multiple of hop
    with pytest.raises(ValueError, match='5 utterances for 4 slots'):
        g._layout([80] * 5)
    with pytest.raises(ValueError, match='exceed'):
        g._layout([16000, 16000])
    with pytest.raises(ValueError, match='multiples of hop_length'):
        g._layout([8000, 4040])
    with pytest.raises(ValueError, match='exactly'):
        g._layout([8000, 8000, 8000, 7920])


def test_filler_is_at_least_min_rows():
    """hop below the packed persistent form's minimum utterance: the fillers (and real utterances) need VARLEN_MIN_ROWS rows."""
    from pwv_amd import _lib
    g = _capacity(3, 300, hop=10)
    assert g.filler == 40 and _lib.VARLEN_MIN_ROWS == 32
    assert g._layout([100]) == [100, 40, 160]
    assert not g.fits([20, 100])                     # an utterance shorter than 32 rows has no packed persistent form
    assert not g.fits([240]) and g.fits([220])       # 220 + 2 * 40 = 300


def test_graph_needs_a_gpu():
    from pwv_amd import _lib
    from pwv_amd.graph import GraphedPackedVocoder
    from pwv_amd.models import IAFVocoder
    from pwv_amd.variables import VariableStore
    set_hparams(O.ModelConfig())
    model = IAFVocoder(1, 80, store=VariableStore(device=torch.device('cpu')))
    with pytest.raises(_lib.PwvError, match='GPU'):
        GraphedPackedVocoder(model, 2, 16000)


def test_seeds_validation():
    from pwv_amd.models import IAFVocoder, noise_streams
    assert noise_streams(None, None, 3) is None
    assert noise_streams([1, 2], None, 2) == [(1, 0), (2, 0)]
    assert noise_streams([2 ** 64 - 1], [2 ** 40], 1) == [(2 ** 64 - 1, 2 ** 40)]
    with pytest.raises(ValueError, match='offsets need seeds'):
        noise_streams(None, [0], 1)
    set_hparams(O.ModelConfig())
    model = IAFVocoder(1, 80)
    mels = [torch.zeros((3, 80)), torch.zeros((5, 80))]
    for bad, match in (([1], 'seeds holds 1 values for 2'), ([1, 2, 3], 'seeds holds 3'), ([1, -1], r'seeds\[1\]'),
                       ([2 ** 64, 0], r'seeds\[0\]'), ([1.5, 2], r'seeds\[0\]'), ([True, 2], r'seeds\[0\]')):
        with pytest.raises(ValueError, match=match):
            model.generate_varlen(mels, seeds=bad)
    with pytest.raises(ValueError, match=r'offsets\[1\]'):
        model.generate_varlen(mels, seeds=[1, 2], offsets=[0, 2 ** 64])
    with pytest.raises(ValueError, match='offsets holds 1'):
        model.generate_varlen(mels, seeds=[1, 2], offsets=[0])
    with pytest.raises(ValueError, match='exclude each other'):
        model.generate_varlen(mels, z=torch.zeros((480, 1)), seeds=[1, 2])
    with pytest.raises(ValueError, match='exclude each other'):
        model.forward_packed(torch.zeros((8, 80)), [0, 3, 8], z=torch.zeros((480, 1)), seeds=[1, 2])


def test_packed_noise_op_checks(built_lib):
    from pwv_amd import _lib, engine
    cu = torch.tensor([0, 80, 160], dtype=torch.int32)
    st = torch.zeros((2, 2), dtype=torch.int64)
    with pytest.raises(_lib.PwvError, match='GPU'):
        engine.logistic_noise_packed_op(cu, st, 160)
    with pytest.raises(ValueError, match='int32'):
        engine.logistic_noise_packed_op(cu.long(), st, 160)
    with pytest.raises(ValueError, match='int64'):
        engine.logistic_noise_packed_op(cu, st.int(), 160)
    assert engine.as_int64_bits(2 ** 64 - 1) == -1 and engine.as_int64_bits(2 ** 63) == -2 ** 63 and engine.as_int64_bits(5) == 5
    # the C entry point refuses bad arguments before it needs a device
    assert built_lib.pwv_logistic_noise_packed_f32(None, None, None, 1, 10, None) == -1
    assert b'NULL' in built_lib.pwv_last_error()
    assert built_lib.pwv_logistic_noise_packed_f32(0x1000, 0x2000, 0x3000, 0, 10, None) == -1
    assert built_lib.pwv_logistic_noise_packed_f32(0x1000, 0x2000, 0x3000, 1, 1 << 31, None) == -1
    assert b'pwv_logistic_noise_packed_f32' in built_lib.pwv_last_error()


def test_packed_sampler_is_declared_and_exported(built_lib):
    from pwv_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'pwv_hip.h')).read()
    assert re.search(r'int pwv_logistic_noise_packed_f32\(float\* z, const int32_t\* cu_rows, const uint64_t\* streams, int32_t n, '
                     r'int64_t rows,\s+pwv_stream_t stream\);', header)
    assert '#define PWV_HIP_VERSION 301' in header and _lib.HEADER_VERSION == 301
    assert 'pwv_logistic_noise_packed_f32' in _lib.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), 'pwv_logistic_noise_packed_f32')


def test_packed_sampler_uses_no_scratch():
    """The compiler's resource remarks (gfx950 device code, no GPU needed): the packed sampler uses no scratch and spills nothing."""
    from tests.util import kernel_resources
    res = kernel_resources('pwv_misc.hip')
    mine = [r for name, r in res.items() if name.startswith('pwv::logistic_noise_packed_kernel(')]
    assert len(mine) == 1, sorted(res)
    assert mine[0]['scratch'] == 0 and mine[0]['vgpr_spills'] == 0, mine[0]
    assert mine[0]['dynamic_stack'] is False, mine[0]
