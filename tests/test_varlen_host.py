"""CPU: the host side of packed ("varlen") batches -- the layout built from the utterance lengths, the input checks of
IAFVocoder.generate_varlen / forward_packed, the padded-fallback routing of engine.run_flow_varlen, and the C ABI's validation of
the packed-batch fields of pwv_persist_args (no GPU needed for any of it)."""
import ctypes

import pytest
import torch

from oracle import iaf_oracle as O
from tests.util import set_hparams


def _geom(lengths, hop=80):
    from pwv_amd import engine
    return engine.VarlenGeometry(lengths, hop, torch.device('cpu'))


def test_layout_from_lengths():
    g = _geom([16000, 80, 4000])
    assert g.cu_rows_host == [0, 16000, 16080, 20080] and g.cu_frames_host == [0, 201, 203, 254]
    assert g.cu_rows.dtype == torch.int32 and g.cu_rows.tolist() == g.cu_rows_host and g.cu_frames.tolist() == g.cu_frames_host
    assert (g.n, g.rows, g.total_frames, g.max_len, g.max_frames) == (3, 20080, 254, 16000, 201)
    for bad in ([], [0], [81], [-80]):
        with pytest.raises(ValueError):
            _geom(bad)


def test_packed_layout_is_the_host_side_of_the_geometry():
    """engine.PackedLayout: the prefix sums every user of the packed layout takes (VarlenGeometry, the graph's tables, ragged_plan,
    generate_varlen) -- plain integers, the geometry's checks and messages."""
    from pwv_amd import engine
    p = engine.PackedLayout([16000, 80, 4000], 80)
    assert p.cu_rows_host == [0, 16000, 16080, 20080] and p.cu_frames_host == [0, 201, 203, 254]
    assert p.lengths == [16000, 80, 4000] and p.frames == [201, 2, 51] and p.hop == 80
    assert (p.n, p.rows, p.total_frames, p.max_len, p.max_frames) == (3, 20080, 254, 16000, 201)
    assert isinstance(_geom([80]), engine.PackedLayout) and not hasattr(p, 'device')
    with pytest.raises(ValueError, match='a packed batch needs at least one utterance'):
        engine.PackedLayout([], 80)
    for bad in ([81], [0], [-80]):
        with pytest.raises(ValueError, match=r'utterance lengths must be positive multiples of hop_length \(80\), got %d' % bad[0]):
            engine.PackedLayout([160] + bad, 80)


def test_padded_index_maps_round_trip():
    g = _geom([3, 5, 2], hop=1)
    x = torch.arange(10, dtype=torch.float32).reshape(10, 1)
    p = g.pad_rows(x)
    assert p.shape == (3, 5, 1)
    assert p[:, :, 0].tolist() == [[0, 1, 2, 0, 0], [3, 4, 5, 6, 7], [8, 9, 0, 0, 0]]
    assert torch.equal(g.unpad_rows(p), x)
    f = torch.arange(13, dtype=torch.float32).reshape(13, 1)          # len + 1 frames each (hop 1): 4, 6, 3
    assert g.pad_frames(f)[:, :, 0].tolist() == [[0, 1, 2, 3, 0, 0], [4, 5, 6, 7, 8, 9], [10, 11, 12, 0, 0, 0]]


def test_generate_varlen_rejects_bad_inputs():
    from pwv_amd import _lib
    from pwv_amd.models import IAFVocoder
    set_hparams(O.ModelConfig())
    model = IAFVocoder(1, 80)
    with pytest.raises(ValueError):
        model.generate_varlen([])
    with pytest.raises(ValueError, match='t_mel >= 2'):
        model.generate_varlen([torch.zeros((1, 80))])               # one frame: no sample
    with pytest.raises(ValueError, match='t_mel >= 2'):
        model.generate_varlen([torch.zeros((5, 64))])               # wrong n_mels
    with pytest.raises(ValueError, match='t_mel >= 2'):
        model.generate_varlen([torch.zeros((3, 5, 80))])            # a batch, not an utterance
    with pytest.raises(_lib.PwvError, match='GPU'):
        model.generate_varlen([torch.zeros((5, 80))])               # no CPU path
    mels = [torch.zeros((3, 80)), torch.zeros((5, 80))]             # 160 + 320 samples
    with pytest.raises(ValueError, match=r'z\[0\] must be \(160, 1\)'):
        model.generate_varlen(mels, z=[torch.zeros((200, 1)), torch.zeros((280, 1))])      # the right total, the wrong split
    with pytest.raises(ValueError, match='z holds 1 utterances'):
        model.generate_varlen(mels, z=[torch.zeros((480, 1))])


class _Net:
    """What the routing looks at of a WaveNet."""
    def __init__(self, **kw):
        self.use_skip_connection, self.precision, self.in_channels, self.out_channels = False, None, 1, 1
        self.dilations, self.condition_channels, self.filter_width, self.fused = [1, 2, 4, 8], 80, 2, True
        self.__dict__.update(kw)

    def fused_supported(self, cond):
        return self.fused


def test_fallback_routing(monkeypatch):
    from pwv_amd import engine
    monkeypatch.setattr(engine, 'PERSIST', 'auto')
    monkeypatch.setattr(engine, '_persist_cooldown', 0)
    g, nets = _geom([800, 2400, 1600]), [_Net(), _Net()]
    cond = engine.RepeatedCondition(torch.zeros((1, g.total_frames, 80)), 80, 40, g.rows)
    reason = engine.varlen_fallback_reason
    assert reason(nets, cond, g) is None and reason(nets, None, g) is None
    assert reason([_Net(out_channels=2)], cond, g) is None                                      # a shared net
    assert 'shorter than 32' in reason(nets, cond, _geom([16, 48, 32], hop=16))
    assert 'per-sample' in reason(nets, torch.zeros((1, g.rows, 80)), g)                        # transposed_conv
    assert 'skip' in reason([_Net(use_skip_connection=True)] * 2, cond, g)
    assert "'f16'" in reason(nets, cond, g, 'f16')
    assert 'fused' in reason([_Net(fused=False), _Net(fused=False)], cond, g)                  # e.g. normalize 'in' inside the nets
    monkeypatch.setattr(engine, 'PERSIST_AUTO_MAX_ROWS', g.rows - 1)
    assert 'PERSIST_AUTO_MAX_ROWS' in reason(nets, cond, g)
    monkeypatch.setattr(engine, 'PERSIST_AUTO_MAX_ROWS', g.rows)
    monkeypatch.setattr(engine, '_persist_cooldown', 3)
    assert 'suspended' in reason(nets, cond, g)
    monkeypatch.setattr(engine, '_persist_cooldown', 0)
    monkeypatch.setattr(engine, 'PERSIST', False)
    assert 'PWV_PERSIST=0' in reason(nets, cond, g)


def test_instance_norm_nets_are_refused():
    """'in' statistics span the time axis: neither the packed nor the padded batch computes them per utterance."""
    from pwv_amd import _lib, engine

    class Flow:
        def nets(self):
            return [_Net(normalize='in', fused=False), _Net(normalize='in', fused=False)]
    g = _geom([800, 2400])
    with pytest.raises(_lib.PwvError, match='instance normalisation'):
        engine.run_flow_varlen(Flow(), torch.zeros((g.rows, 1)), None, g)


def test_workspace_bytes_refuses_inconsistent_varlen_fields(built_lib):
    """In the style of test_abi.py::test_argument_validation_no_gpu: the packed-batch fields are checked before anything else."""
    from pwv_amd import _lib
    lib = built_lib
    dil = (ctypes.c_int * 4)(1, 2, 4, 8)

    def args(**kw):
        pa = _lib.PersistArgs()
        pa.G, pa.n_layers, pa.dilations, pa.N, pa.T = 2, 4, dil, 3, 0
        for k, v in kw.items():
            setattr(pa, k, v)
        return pa
    for kw in (dict(cu_rows=0x1000), dict(varlen_rows=4800), dict(cu_rows=0x1000, varlen_rows=4800),
               dict(unit_map=0x2000, varlen_rows=4800), dict(cu_rows=0x1000, unit_map=0x2000)):
        pa = args(**kw)
        assert lib.pwv_persist_workspace_bytes(ctypes.byref(pa)) == 0 and b'packed batch' in lib.pwv_last_error()
        assert lib.pwv_persist_short_input(ctypes.byref(pa)) == -1
    pa = args(cu_rows=0x1000, unit_map=0x2000, varlen_rows=4800, cond_hop=80)        # a frame-rate condition needs cu_frames
    assert lib.pwv_persist_workspace_bytes(ctypes.byref(pa)) == 0 and b'cu_frames' in lib.pwv_last_error()
    pa = args(cu_rows=0x1000, unit_map=0x2000, varlen_rows=64)                        # 3 utterances need >= 96 rows
    assert lib.pwv_persist_workspace_bytes(ctypes.byref(pa)) == 0 and b'at least 32 rows' in lib.pwv_last_error()
    pa.workspace = 0x10000          # (past the NULL-workspace check: the launch refuses the packed fields before it needs a device)
    assert lib.pwv_wavenet_stack_persist_f32(ctypes.byref(pa), None) == -1
    assert b'pwv_wavenet_stack_persist_f32' in lib.pwv_last_error() and b'at least 32 rows' in lib.pwv_last_error()


def test_unit_map_is_declared_and_exported(built_lib):
    import os
    import re
    from pwv_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'pwv_hip.h')).read()
    assert re.search(r'int pwv_varlen_unit_map\(const int\* cu_rows, const int\* cu_frames, int n_utt, int units, int\* out', header)
    assert '#define PWV_VARLEN_REC_INTS %d' % _lib.VARLEN_REC_INTS in header
    assert 'pwv_varlen_unit_map' in _lib.EXPORTED_SYMBOLS and hasattr(ctypes.CDLL(_lib.LIB_PATH), 'pwv_varlen_unit_map')
    assert built_lib.pwv_varlen_unit_map(None, None, 1, 1, None, None) == -1 and b'NULL' in built_lib.pwv_last_error()
