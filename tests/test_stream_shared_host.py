"""CPU: what streaming the shared-net architecture (model.shared_nets: True -- one WaveNet of two outputs per flow) settles without a
device: the history layout of one net per flow, the structural refusals of engine.stream_refusal, and the persistent launcher's argument
checks for a streaming launch with G = 1 and a two-output tail.  tests/test_gpu_stream_shared.py runs the routes."""
import ctypes
from types import SimpleNamespace

import pytest

from oracle import iaf_oracle as O

SMALL = [[1, 2, 4, 8], [1, 2, 4, 8, 16, 32]]
WIDE = [[1, 96, 128, 256], [2, 64, 200, 512, 3, 160]]
C2 = [list(d) for d in O.ModelConfig().dilations]          # the architecture of bench/c2: the default dilations, largest 512
SETS = {'small': SMALL, 'wide': WIDE, 'c2': C2}


def _round(v, m):
    return (v + m - 1) // m * m


def _histories(layout):
    """Every history of a layout as (offset, floats it occupies)."""
    return sorted((off, rows * width if width == 1 else _round(rows, 32) * 64) for off, rows, width in layout.carry)


@pytest.mark.parametrize('name', sorted(SETS))
def test_layout_of_one_net_per_flow(name):
    """HistoryLayout(d, nets_per_flow=1): per flow the d0 + 1 scalars padded to 64 floats, then ONE row history of round32(d_j) x 64 floats
    per layer j >= 1."""
    from pwv_amd.stream import HistoryLayout
    dil = SETS[name]
    lay = HistoryLayout(dil, nets_per_flow=1)
    assert lay.block_floats == sum(_round(d[0] + 1, 64) + sum(_round(v, 32) * 64 for v in d[1:]) for d in dil)
    assert len(lay.row_off) == len(dil) and all(len(per_net) == 1 for per_net in lay.row_off)
    offsets = list(lay.scalar_off) + [o for per_net in lay.row_off for offs in per_net for o in offs[1:]]
    assert all(o % 4 == 0 for o in offsets) and lay.block_floats % 4 == 0
    assert all(per_net[0][0] == -1 for per_net in lay.row_off)          # layer 0 has no row history
    # `carry` lists each history exactly once: the flows' scalars and every row history of every layer j >= 1
    assert sorted(o for o, _, _ in lay.carry) == sorted(offsets) and len(set(offsets)) == len(offsets)
    assert len(lay.carry) == sum(len(d) for d in dil)
    for (off, rows, width), want in zip(lay.carry, [(d[0] + 1, 1) if j == 0 else (v, 64) for d in dil for j, v in enumerate(d)]):
        assert (rows, width) == want
    # disjoint and inside the block
    end = 0
    for off, floats in _histories(lay):
        assert off >= end, (off, end)
        end = off + floats
    assert end <= lay.block_floats
    assert lay.max_rows == max(max(v for v in d[1:]) for d in dil)


@pytest.mark.parametrize('name', sorted(SETS))
def test_default_layout_is_unchanged(name):
    """nets_per_flow = 2 (the default, and what HistoryLayout(d) gives): scalars, then net 0's row histories, then net 1's."""
    from pwv_amd.stream import HistoryLayout
    dil = SETS[name]
    lay, same = HistoryLayout(dil), HistoryLayout(dil, nets_per_flow=2)
    assert (lay.scalar_off, lay.row_off, lay.carry, lay.block_floats) == (same.scalar_off, same.row_off, same.carry, same.block_floats)
    off, scalar_off, row_off = 0, [], []
    for d in dil:
        scalar_off.append(off)
        off += _round(d[0] + 1, 64)
        per_net = []
        for _ in range(2):
            offs = [-1]
            for v in d[1:]:
                offs.append(off)
                off += _round(v, 32) * 64
            per_net.append(offs)
        row_off.append(per_net)
    assert lay.scalar_off == scalar_off and lay.row_off == row_off and lay.block_floats == off
    one = HistoryLayout(dil, nets_per_flow=1)
    assert lay.block_floats - one.block_floats == sum(_round(v, 32) * 64 for d in dil for v in d[1:])


def test_session_bytes_of_the_c2_model():
    """Two generations of the block and the kept frame: 3,475,776 bytes for the shared c2 model, 6,949,184 for the default one."""
    from pwv_amd.stream import HistoryLayout
    assert HistoryLayout(C2, nets_per_flow=1).block_floats * 4 == 1737728
    assert 2 * HistoryLayout(C2, nets_per_flow=1).block_floats * 4 + 80 * 4 == 3475776
    assert 2 * HistoryLayout(C2).block_floats * 4 + 80 * 4 == 6949184


def _net(out_channels, skip=False, dilations=(1, 2, 4, 8)):
    return SimpleNamespace(dilations=list(dilations), use_skip_connection=skip, in_channels=1, out_channels=out_channels, condition_channels=80,
                           filter_width=2, precision=None, normalize=None, fused_supported=lambda cond: True)


def test_stream_refusal_structure():
    """No device: one net of two outputs passes next to two nets of one; one net of one output is 'shape'; skip stays skip."""
    from pwv_amd import engine
    assert engine.stream_refusal([_net(2)], None) is None
    assert engine.stream_refusal([_net(1), _net(1)], None) is None
    shape, skip = engine._STREAM_STRUCTURE_WHY['shape'], engine._STREAM_STRUCTURE_WHY['skip']
    assert engine.stream_refusal([_net(1)], None) == shape
    assert engine.stream_refusal([_net(2), _net(2)], None) == shape
    assert engine.stream_refusal([_net(2, dilations=(1,))], None) == shape          # fewer than 2 layers
    assert engine.stream_refusal([_net(2, skip=True)], None) == skip
    assert engine.stream_refusal([_net(2)], None, 'f16') == engine._STREAM_STRUCTURE_WHY['f16']
    normalised = _net(2)
    normalised.normalize = 'bn'
    assert engine.stream_refusal([normalised], None) == shape


def test_launcher_takes_one_net_with_a_two_output_tail(built_lib):
    """pwv_wavenet_stack_persist_f32 with hist, G = 1, tail_q = 2: a valid hist_row_off[0] gets past the checks of the streaming
    arguments; without it the launch is PWV_EINVAL and names the field.  Nothing may be launched here (the pointers are made up): the
    call that passes the streaming checks carries a proj_row_stride that is no multiple of 4, which the launcher refuses later -- or has
    no device to ask for its CU count."""
    from pwv_amd import _lib
    lib = built_lib
    dil = (ctypes.c_int * 3)(1, 2, 4)
    offs = (ctypes.c_size_t * 4)(0, 64, 2112, 4160)          # layers 0 .. 2 of the run and the tail's layer (d = 8)
    sa = _lib.StreamArgs()
    sa.hist_rd = sa.hist_wr = 0x20000
    sa.block_stride, sa.slot_tab = 1 << 16, 0x30000

    def args():
        pa = _lib.PersistArgs()
        pa.G, pa.n_layers, pa.dilations, pa.N, pa.T = 1, 3, dil, 3, 800
        pa.precision, pa.workspace = _lib.PREC_F16X3, 0x10000
        pa.tail_q, pa.tail_dilation = 2, 8
        pa.hist = ctypes.addressof(sa)
        pa.proj_row_stride = 130
        return pa

    pa = args()
    rc = lib.pwv_wavenet_stack_persist_f32(ctypes.byref(pa), None)
    err = lib.pwv_last_error()
    assert rc == -1 and b'hist without hist_row_off[0]' in err, err
    pa = args()
    pa.hist_row_off[0] = offs
    rc = lib.pwv_wavenet_stack_persist_f32(ctypes.byref(pa), None)
    err = lib.pwv_last_error()
    assert rc != 0 and b'hist' not in err and (b'no HIP device' in err or b'bad projection arguments' in err), (rc, err)
    # net 1's offsets are not asked for: G = 1
    assert b'hist_row_off[1]' not in err
