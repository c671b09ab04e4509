"""-m gpu: the top of a unit of the persistent kernel's general loop (csrc/pwv_persist_tasks.inc, MODE 0): the P row is loaded through a
buffer descriptor that starts at the unit's FIRST P row (lane 0's), with the row stride and the hop constants read out of VGPR lanes,
and the layer refill reaches LDS through buffer loads -- what tests/test_persist_top_isa.py looks at in the assembly.  The smallest
shapes at which the P row's address can go wrong: units that cross a frame boundary and units that do not (hop 80), units that span
three frames (hop 16), units that span two utterances (the P base differs between the lanes), a last unit that is not full (its idle
lanes are clamped to the last row), a 7-layer stack (the next task lies in the next layer; the last task has nothing behind it; six
refills), a net without a condition (cond_hop == 0: every lane reads P row 0), a packed batch of unequal lengths (the P base comes from
the unit's record) and a streaming push with a non-zero cond_offset onto a carried history.  Persistent launch against per-layer
launches, torch.equal, both arithmetics.  PERSIST_MIN_UNITS = 16 forces the general instantiation at these sizes; every case asserts
from EVENT_LOG and PERSIST_ARGS_HOOK that this is what ran, with the geometry it claims."""
import pytest
import torch

from tests.test_gpu_persist_prefetch import DIL6, DIL7, _Launches, _nets, knobs  # noqa: F401  (knobs: a fixture)
from tests.util import small_cfg

pytestmark = pytest.mark.gpu
PRECS = ['f16x3', 'f32']


class _Geometry(_Launches):
    """... and the conditioning geometry of every persistent launch"""

    def _hook(self, pa):
        super()._hook(pa)
        self.seen[-1].update(hop=pa.cond_hop, offset=pa.cond_offset, frames=pa.cond_frames, N=pa.N, T=pa.T, layers=pa.n_layers)


# (n, t, dilations, hop, offset): offset None = no condition at all
CASES = {
    'hop80_1x2080': (1, 2080, DIL6, 80, 40),                # 65 units, 26 frame boundaries: most units cross one, some none
    'hop16_1x2080': (1, 2080, DIL6, 16, 8),                 # every unit spans three frames; the look-backs 1 .. 64 near the utterance start
    'hop80_3x1000': (3, 1000, DIL6, 80, 40),                # units 31 and 62 span two utterances: p_base differs between the lanes
    'hop16_1x2070_last_unit_not_full': (1, 2070, DIL6, 16, 8),      # 22 rows in unit 64, the other lanes clamped to row 2069
    'hop80_1x2080_7_layers': (1, 2080, DIL7, 80, 40),       # six layers in the loop: the next task in the next layer, a last task
    'no_condition_1x2080': (1, 2080, DIL6, 0, None),        # cond_hop == 0
}


@pytest.mark.parametrize('precision', PRECS)
@pytest.mark.parametrize('case', list(CASES))
def test_top_of_a_unit_is_bit_identical_to_per_layer_launches(gpu, knobs, case, precision):
    engine = knobs
    n, t, dilations, hop, offset = CASES[case]
    if offset is not None:
        store, nets = _nets(gpu, dilations)
    else:
        from pwv_amd.modules import WaveNet
        from pwv_amd.variables import VariableStore
        store = VariableStore(device=gpu, seed=3)
        kw = dict(batch_size=1, dilations=list(dilations), filter_width=2, residual_channels=64, dilation_channels=64, skip_channels=128,
                  quantization_channels=1, use_biases=True, use_skip_connection=False, is_training=False, store=store)
        nets = [WaveNet(name='n%d' % k, **kw) for k in range(2)]
    g = torch.Generator().manual_seed(len(case) * 5 + t)
    x = torch.randn((n, t, 1), generator=g).to(gpu)
    cond = None
    if offset is not None:
        frames = (t - 1 + offset) // hop + 1
        cond = engine.RepeatedCondition(torch.rand((n, frames, 80), generator=g).to(gpu), hop, offset, t)
    engine.PERSIST = False
    engine.run_nets(nets, x, cond, precision=precision)      # creates the variables
    for name in list(store.vars):
        if store.vars[name].dim() == 1:
            store.vars[name].normal_(0, 0.1)
    store.version += 1
    ref = [o.clone() for o in engine.run_nets(nets, x, cond, precision=precision)]
    engine.PERSIST, engine.PERSIST_MIN_UNITS = True, 16
    with _Geometry(engine) as la:
        for _ in range(2):
            got = engine.run_nets(nets, x, cond, precision=precision)
            torch.cuda.synchronize()
            assert engine.persist_status() == 0
            for a, b in zip(ref, got):
                assert torch.equal(a, b), float((a - b).abs().max())
        la.check_general(n * t, 2)
        assert all(e[4] == len(dilations) - 1 and e[5] == 1 for e in la.log)
        for a in la.seen:
            assert (a['N'], a['T'], a['hop'], a['layers']) == (n, t, hop, len(dilations) - 1) and not a['packed'] and not a['stream'], a
            if offset is not None:
                assert (a['offset'], a['frames']) == (offset, (t - 1 + offset) // hop + 1), a


@pytest.mark.parametrize('precision', PRECS)
def test_packed_batch_of_unequal_lengths_with_a_condition(gpu, knobs, monkeypatch, precision):
    """generate_varlen at hop 80 with 1040 + 400 + 640 rows: 65 units, the utterances end inside units 32 and 45, and a lane's P base is
    its utterance's first frame (cu_frames).  Every piece equals its own one-shot forward on per-layer launches."""
    from tests.test_gpu_hop_geometry import _one_shot, _packed_inputs
    from tests.test_gpu_stream import _model
    engine = knobs
    cfg = small_cfg(dilations=[DIL6, [1, 2, 4, 8]])
    model, _ = _model(gpu, cfg, precision)
    lengths = [1040, 400, 640]
    _, _, mel_t, z_t = _packed_inputs(cfg, lengths, gpu, seed=11)
    engine.PERSIST = False
    want = [_one_shot(model, cfg.hop_length, mt, zt).clone() for mt, zt in zip(mel_t, z_t)]
    engine.PERSIST, engine.PERSIST_MIN_UNITS = True, 16
    monkeypatch.setattr(engine, 'VARLEN_PADDED', 0)
    with _Geometry(engine) as la:
        out = model.generate_varlen(mel_t, z=z_t)
        torch.cuda.synchronize()
        assert engine.persist_status() == 0 and engine.VARLEN_PADDED == 0
        la.check_general(sum(lengths), cfg.n_iaf)
        assert all(a['packed'] and a['hop'] == cfg.hop_length and a['offset'] == cfg.hop_length // 2 and a['N'] == len(lengths) for a in la.seen), la.seen
    for piece, w, L in zip(out, want, lengths):
        assert tuple(piece.shape) == (L, 1) and torch.equal(piece, w), (L, float((piece - w).abs().max()))


@pytest.mark.parametrize('precision', PRECS)
def test_streaming_push_with_a_condition_offset_onto_a_carried_history(gpu, knobs, precision):
    """Two sessions, two pushes of 2 x 1040 rows: the second push continues the first one's history and reads its frames at a non-zero
    cond_offset.  Outputs and every byte of the history arrays equal those of the per-layer streaming launches."""
    from tests.test_gpu_stream import _Feeder, _inputs, _model
    engine = knobs
    cfg = small_cfg(dilations=[DIL6, [1, 2, 4, 8]])
    model, _ = _model(gpu, cfg, precision)
    T, S = 1040, 2
    ins = [_inputs(cfg, 2 * T, gpu, seed=70 + i) for i in range(S)]
    res = {}
    for persist in (False, True):
        engine.PERSIST, engine.PERSIST_MIN_UNITS = persist, 16
        s = model.open_stream(slots=S)
        fd = _Feeder(s)
        for i in range(S):
            fd.start(i, ins[i][2], ins[i][3])
        fd.adv([0, 1], T)
        with _Geometry(engine) as la:
            fd.adv([0, 1], T)
            torch.cuda.synchronize()
            if persist:
                assert engine.persist_status() == 0
                la.check_general(S * T, cfg.n_iaf)
                assert all(a['stream'] and not a['packed'] and a['hop'] == cfg.hop_length and a['offset'] != 0 for a in la.seen), la.seen
            else:
                assert [e[0] for e in la.log] == ['layer_stream'] * cfg.n_iaf and not la.seen
        res[persist] = ([fd.result(i).clone() for i in range(S)], s._hist.clone())
    for a, b in zip(res[True][0], res[False][0]):
        assert torch.equal(a, b), float((a - b).abs().max())
    assert torch.equal(res[True][1], res[False][1]), int((res[True][1] != res[False][1]).sum())
    assert all(bool(torch.isfinite(a).all()) for a in res[True][0])
