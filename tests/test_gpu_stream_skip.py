"""GPU: streaming a skip-connection model (IAFVocoder.open_stream(slots, use_skip_connection=True) -> pwv_iaf_front_stream_f32, L calls of
pwv_wavenet_layer_stream_skip_f32, the head launch on the skip sum, the affine).  The contract is that of tests/test_gpu_stream_cond.py:
the pushes of a session, concatenated, are torch.equal to the one-shot forward IAFVocoder(1, L)(None, mel, z=z) at the same precision
-- which this route does not touch --, a session's audio does not depend on its companions, a push is a transaction.  Smallest shapes:
two sessions of the model hop_cfg(80, use_skip_connection) put a session boundary inside a 32-row unit at every push of one frame (80
rows, a partial last unit of the skip accumulator)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import iaf_oracle as O
from tests.guarded import guarded
from tests.util import TOL_F32, hop_cfg, set_hparams, small_cfg

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOP = 80
PRECISIONS = ['f16x3', 'f32']
OPEN = dict(use_skip_connection=True)


def _skip(**kw):
    return hop_cfg(HOP, use_skip_connection=True, **kw)


def _wide():
    # most dilations above the 80-sample chunk, several that are no multiple of 32; layer 0 at 1, 3 and -- above the chunk -- 96; a look-back
    # of 512 that reads rows carried six times
    return small_cfg(dilations=[[1, 96, 128, 256], [3, 64, 200, 512, 2, 160], [96, 1, 40]], n_iaf=3, use_skip_connection=True)


def _model(gpu, cfg, precision=None, seed=2, weights=None):
    from pwv_amd.models import IAFVocoder
    from pwv_amd.variables import VariableStore
    set_hparams(cfg)
    w = O.init_weights(cfg, seed=seed) if weights is None else weights
    store = VariableStore(device=gpu)
    store.load_dict(w)
    return IAFVocoder(batch_size=1, length=HOP, store=store, precision=precision), w


def _inputs(cfg, frames, gpu, seed=0):
    rng = np.random.default_rng(seed)
    L = (frames - 1) * HOP
    mel = rng.uniform(-1, 1, (frames, cfg.n_mels)).astype(np.float32)
    z = np.clip(rng.logistic(0, 1, (L, 1)), -20, 20).astype(np.float32)
    return mel, z, torch.from_numpy(mel).to(gpu), torch.from_numpy(z).to(gpu)


def _one_shot(model, mel_t, z_t, precision=None):
    from pwv_amd.models import IAFVocoder
    L = (mel_t.shape[0] - 1) * HOP
    one = IAFVocoder(batch_size=1, length=L, store=model.store, precision=precision or model.precision)
    return one(None, mel_t[None], is_training=False, z=z_t[None])[0]


def _push_frames(s, slots, utts, schedule, **kw):
    """Give every slot of `slots` its next f frames for f in `schedule` (all slots in one push); utts[i] = (mel_t, z_t) of slots[i].
    Returns the concatenated pieces per slot."""
    pos, outs = 0, [[] for _ in slots]
    for f in schedule:
        e = s.emitted(slots[0])
        T = (f - (1 if pos == 0 else 0)) * HOP
        got = s.push(torch.stack([m[pos:pos + f] for m, _ in utts]), slots=slots, z=torch.stack([z[e:e + T] for _, z in utts]), **kw)
        assert tuple(got.shape) == (len(slots), T, 1)
        if kw.get('verify') is False:
            s.verify()
        for i in range(len(slots)):
            outs[i].append(got[i])
        pos += f
    return [torch.cat(o) for o in outs]


_REF = {}


def _reference(gpu, precision):
    """Shared, never written to: two utterances of 8 frames (560 samples) and their one-shot forwards at `precision`.  The one-shot forward
    is causal in the frames too -- sample t reads frame (t + 40) // 80 -- so a shorter schedule is compared with its prefix."""
    if precision not in _REF:
        cfg = _skip()
        model, w = _model(gpu, cfg, precision)
        ins = [_inputs(cfg, 8, gpu, seed=60 + i) for i in range(2)]
        _REF[precision] = (cfg, w, ins, [_one_shot(model, u[2], u[3]).clone() for u in ins])
    cfg, w, ins, want = _REF[precision]
    model, _ = _model(gpu, cfg, precision, weights=w)
    return cfg, w, model, ins, want


@pytest.mark.parametrize('schedule', [[1, 1, 2, 3, 1], [4, 1, 1], [7]], ids=['1-1-2-3-1', '4-1-1', '7'])
@pytest.mark.parametrize('precision', PRECISIONS)
def test_chunks_equal_the_one_shot_forward(gpu, precision, schedule):
    """Two sessions advanced together; the first push of one frame yields an empty piece.  torch.equal, both arithmetics; the flows ran
    on the skip route and on no other."""
    from pwv_amd import engine
    cfg, _, model, ins, want = _reference(gpu, precision)
    s = model.open_stream(slots=2, **OPEN)
    saved, engine.EVENT_LOG = engine.EVENT_LOG, []
    try:
        got = _push_frames(s, [0, 1], [(u[2], u[3]) for u in ins], schedule)
        log = [e for e in engine.EVENT_LOG if e[0] in ('layer_stream_skip', 'layer_stream', 'layer_stream_cond', 'persist')]
    finally:
        engine.EVENT_LOG = saved
    launching = sum(1 for k, f in enumerate(schedule) if k or f > 1)
    assert [e[0] for e in log] == ['layer_stream_skip'] * (launching * cfg.n_iaf), log
    assert sorted({(e[3], e[4]) for e in log}) == sorted({(2, len(d)) for d in cfg.dilations[:cfg.n_iaf]}), log
    L = (sum(schedule) - 1) * HOP
    assert s.emitted(0) == s.emitted(1) == L
    for i in range(2):
        assert torch.equal(got[i], want[i][:L]), (i, float((got[i] - want[i][:L]).abs().max()))


@pytest.mark.parametrize('precision', PRECISIONS)
def test_wide_model_one_frame_pushes(gpu, precision):
    """Dilations up to 512 against chunks of 80 rows: almost every history is longer than the chunk, the carry launch runs at every push,
    at 720 samples the look-back of 512 reads rows that were carried over six times; layer-0 dilations 1, 3 and 96 -- the last one above the chunk, where a
    layer-0 history that held anything but the causal layer's rows (or was not carried) would show."""
    cfg = _wide()
    model, _ = _model(gpu, cfg, precision)
    _, _, mel_t, z_t = _inputs(cfg, 10, gpu, seed=1)
    s = model.open_stream(slots=1, **OPEN)
    assert (s.layout.row_off[2][0][0], 96, 64) in s.layout.carry
    got = _push_frames(s, [0], [(mel_t, z_t)], [1] * 10)[0]
    want = _one_shot(model, mel_t, z_t)
    assert got.shape[0] == 720 and torch.equal(got, want), float((got - want).abs().max())


@pytest.mark.parametrize('precision', PRECISIONS)
def test_stream_matches_oracle(gpu, precision):
    """Against the fp64 oracle at the fp32 bar of every parity test (enqueue-only + verify(): no self-repair)."""
    cfg, w, model, ins, _ = _reference(gpu, precision)
    s = model.open_stream(slots=2, **OPEN)
    got = _push_frames(s, [0, 1], [(u[2], u[3]) for u in ins], [2, 1, 3, 2], verify=False)
    for i in range(2):
        want = O.iaf_vocoder_forward(w, ins[i][0][None], ins[i][1][None], cfg)[0]
        err = float(np.abs(got[i].cpu().numpy() - want).max())
        print('skip stream vs oracle, %s, slot %d: %.3g' % (precision, i, err))
        assert err <= TOL_F32, err


def test_sessions_are_independent(gpu):
    """The same utterance pushed alone, beside another session, and on another slot: the same bits."""
    cfg, _, model, ins, want = _reference(gpu, 'f16x3')
    a, b = (ins[0][2], ins[0][3]), (ins[1][2], ins[1][3])
    sched = [2, 1, 3, 2]
    alone = _push_frames(model.open_stream(slots=1, **OPEN), [0], [a], sched)[0]
    beside = _push_frames(model.open_stream(slots=3, **OPEN), [2, 0], [b, a], sched)
    other = _push_frames(model.open_stream(slots=3, **OPEN), [1], [a], sched)[0]
    assert torch.equal(alone, want[0]) and torch.equal(beside[1], alone) and torch.equal(other, alone) and torch.equal(beside[0], want[1])


@pytest.mark.parametrize('precision', PRECISIONS)
def test_ragged_pushes(gpu, precision):
    """push_varlen with frame counts [1, 3, 2] then [2, 1, 4], slot 1 running and slots 0, 2 fresh at the first tick (so a short last chunk
    of one frame beside longer ones): the pieces equal the same sessions advanced by separate push calls, and the one-shot forward; every
    flow of a launching tick took the grouped route on the skip layer launches."""
    from pwv_amd import engine
    cfg, _, model, ins, want = _reference(gpu, precision)
    third = _inputs(cfg, 8, gpu, seed=62)
    utts = [(ins[0][2], ins[0][3]), (ins[1][2], ins[1][3]), (third[2], third[3])]
    ticks = [[1, 3, 2], [2, 1, 4]]
    s, ref = model.open_stream(slots=3, **OPEN), model.open_stream(slots=3, **OPEN)
    pos, outs, routs = [0, 2, 0], [[], [], []], [[], [], []]
    for st in (s, ref):
        head = st.push(utts[1][0][None, :2], slots=[1], z=utts[1][1][None, :HOP])          # slot 1 is running: 2 frames, 80 samples
    outs[1].append(head[0]), routs[1].append(head[0])
    saved, engine.EVENT_LOG = engine.EVENT_LOG, []
    try:
        for counts in ticks:
            fresh = [p == 0 for p in pos]
            T = [(f - (1 if fr else 0)) * HOP for f, fr in zip(counts, fresh)]
            mels = [utts[i][0][pos[i]:pos[i] + counts[i]] for i in range(3)]
            zs = [utts[i][1][s.emitted(i):s.emitted(i) + T[i]] for i in range(3)]
            got = s.push_varlen(mels, slots=[0, 1, 2], z=zs)
            assert [g.shape[0] for g in got] == T
            mark = len(engine.EVENT_LOG)
            for i in range(3):
                outs[i].append(got[i])
                routs[i].append(ref.push(mels[i][None], slots=[i], z=zs[i][None])[0])
                pos[i] += counts[i]
            del engine.EVENT_LOG[mark:]          # (the reference stream's uniform pushes)
        log = [e for e in engine.EVENT_LOG if e[0] in ('stream_ragged', 'persist', 'layer_stream', 'layer_stream_skip')]
    finally:
        engine.EVENT_LOG = saved
    ragged = [e for e in log if e[0] == 'stream_ragged']
    assert len(ragged) == 2 * cfg.n_iaf and all(e[3] == 'grouped' and 'skip accumulation' in e[4] for e in ragged), log
    assert all(e[0] in ('stream_ragged', 'layer_stream_skip') for e in log), log      # neither a persistent launch nor the launches without skip sums
    assert sum(1 for e in log if e[0] == 'layer_stream_skip') == sum(e[5] for e in ragged)      # one uniform skip flow per group
    third_want = _one_shot(model, third[2], third[3])
    for i, w_i in enumerate([want[0], want[1], third_want]):
        got_i = torch.cat(outs[i])
        assert torch.equal(got_i, torch.cat(routs[i])), i
        assert got_i.shape[0] == (pos[i] - 1) * HOP and torch.equal(got_i, w_i[:got_i.shape[0]]), i


@pytest.mark.parametrize('precision', PRECISIONS)
def test_shared_net_variant(gpu, precision):
    """shared_nets with use_skip_connection: one net of two outputs per flow (G = 1, a head of Q = 2 on the skip sum)."""
    from pwv_amd import engine
    cfg = _skip(shared_nets=True)
    model, _ = _model(gpu, cfg, precision)
    ins = [_inputs(cfg, 7, gpu, seed=70 + i) for i in range(2)]
    s = model.open_stream(slots=2, **OPEN)
    saved, engine.EVENT_LOG = engine.EVENT_LOG, []
    try:
        got = _push_frames(s, [0, 1], [(u[2], u[3]) for u in ins], [1, 3, 1, 2])
        log = [e for e in engine.EVENT_LOG if e[0] == 'layer_stream_skip']
    finally:
        engine.EVENT_LOG = saved
    assert log and all(e[3] == 1 for e in log), log
    for i in range(2):
        assert torch.equal(got[i], _one_shot(model, ins[i][2], ins[i][3])), i


# ---- the transaction -----------------------------------------------------------------------------------------------------------------
SKIP_SCALE = 1.0e5      # on flow 0's layer-1 skip weights of both nets (see _scaled_skip)


def _scaled_skip(cfg, w, mel, z):
    """(CPU) Flow 0's layer-1 skip weights times SKIP_SCALE, chosen with the fp64 oracle so that BOTH bounds of the split-fp16 range
    guard are crossed and nothing else saturates: ||skip||_1 of that layer passes fp16's 65000 (the pack-time bound on the skip sum:
    flow 0 itself is planned in exact fp32), flow 0's output -- flow 1's input -- passes 65000 in every 80-sample chunk (the run-time
    bound: x_limit <= 65000 for a scalar-input net, so flow 1's guard trips and the chunk is rerun), and the exact result stays finite and
    far inside fp32 (< 1e12).  Returns {name: scaled weight}."""
    names = ['iaf_vocoder/iaf0/%s/dilated_stack/layer1/skip' % net for net in ('scalar', 'shifter')]
    scaled = {n: (w[n] * np.float32(SKIP_SCALE)).astype(np.float32) for n in names}
    w2 = dict(w)
    w2.update(scaled)
    out, flows = O.iaf_vocoder_forward(w2, mel[None], z[None], cfg, return_flows=True)
    x1 = np.abs(flows[0][0, :, 0])
    per_chunk = [float(x1[i:i + HOP].max()) for i in range(0, x1.shape[0], HOP)]
    l1 = min(float(np.abs(scaled[n][0]).sum(axis=0).max()) for n in names)
    print('scaled skip: ||skip||_1 = %.3g, max |flow-1 input| per chunk = %s, max |out| = %.3g' % (l1, ['%.3g' % v for v in per_chunk],
                                                                                                 float(np.abs(out).max())))
    assert l1 > 65000 * 1.5 and min(per_chunk) > 65000 * 1.2 and bool(np.isfinite(out).all()) and float(np.abs(out).max()) < 1e12
    assert float(max(np.abs(v).max() for v in scaled.values())) < 6.0e4          # every weight itself an ordinary fp16-range value
    return scaled


def _warned(call):
    """call() with every warning recorded (tests/conftest.py turns `pwv:` warnings into errors): (result, messages).  The scaled weights
    also draw the pack-time warning of flow 0's demotion, once per process."""
    import warnings
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        out = call()
    return out, [str(c.message) for c in caught]


def test_range_rerun_is_transactional(gpu):
    """A skip weight scaled past the bounds (_scaled_skip): the chunk warns, is rerun in exact fp32 from the state it started at and equals
    the same chunk pushed by a precision='f32' stream brought to that state -- histories included; the stream goes on from there."""
    from pwv_amd.models import IAFVocoder
    cfg = _skip()
    mel, z, mel_t, z_t = _inputs(cfg, 10, gpu, seed=40)
    w = O.init_weights(cfg, seed=2)
    w = dict(w, **_scaled_skip(cfg, w, mel, z))
    model, _ = _model(gpu, cfg, weights=w)
    m32 = IAFVocoder(batch_size=1, length=HOP, store=model.store, precision='f32')
    s, s32 = model.open_stream(slots=1, **OPEN), m32.open_stream(slots=1, **OPEN)
    first, told = _warned(lambda: s.push(mel_t[None, :4], z=z_t[None, :240]))
    assert sum('rerun in exact fp32' in m for m in told) == 1 and all('rerun in exact fp32' in m or 'exceed the range' in m for m in told), told
    assert s.emitted(0) == 240 and bool(torch.isfinite(first).all())
    assert torch.equal(first, _warned(lambda: s32.push(mel_t[None, :4], z=z_t[None, :240]))[0])
    before = s.state(0)
    assert torch.equal(before['hist'], s32.state(0)['hist']) and bool(before['hist'].abs().sum() > 0)      # the rerun's histories, not the tripped attempt's
    tripped, told = _warned(lambda: s.push(mel_t[None, 4:7], z=z_t[None, 240:480]))
    assert sum('rerun in exact fp32' in m for m in told) == 1, told
    assert s.emitted(0) == 480 and bool(torch.isfinite(tripped).all())
    other = m32.open_stream(slots=1, **OPEN)
    other.load_state(0, before)
    want = other.push(mel_t[None, 4:7], z=z_t[None, 240:480])
    assert torch.equal(tripped, want)
    assert torch.equal(torch.cat([first[0], tripped[0]]), _one_shot(model, mel_t[:7], z_t[:480], 'f32'))
    s2 = m32.open_stream(slots=1, **OPEN)
    s2.load_state(0, s.state(0))
    after, told = _warned(lambda: s.push(mel_t[None, 7:], z=z_t[None, 480:]))
    assert sum('rerun in exact fp32' in m for m in told) == 1, told
    assert torch.equal(after, s2.push(mel_t[None, 7:], z=z_t[None, 480:])) and s.emitted(0) == 720


def test_refused_push_leaves_the_session_where_it_was(gpu):
    """A push that only enqueued and is refused at verify() (the range guard, tripped by the scaled skip weight): generation, counter,
    kept frame and the block the session stands on are what they were; with the weights back, the next chunk has the bits it would
    have had."""
    from pwv_amd import engine
    from pwv_amd._lib import PwvRangeError
    cfg, w, model, ins, want = _reference(gpu, 'f16x3')
    mel, z, mel_t, z_t = ins[0]
    scaled = _scaled_skip(cfg, w, mel, z)
    s = model.open_stream(slots=1, **OPEN)
    first = s.push(mel_t[None, :3], z=z_t[None, :160])
    gen, kept, block, before = list(s._gen), s._kept.clone(), s._hist[s._gen[0]].clone(), s.state(0)
    for name, v in scaled.items():
        model.store.assign(name, v)
    try:
        _warned(lambda: s.push(mel_t[None, 3:6], z=z_t[None, 160:400], verify=False))
        with pytest.raises(PwvRangeError):
            s.verify()
    finally:
        torch.cuda.synchronize()
        engine.clear_range_flag()
    assert s._gen == gen and s.emitted(0) == 160 and s._pending is None and torch.equal(s._kept, kept) and torch.equal(s._hist[gen[0]], block)
    after = s.state(0)
    assert torch.equal(after['hist'], before['hist']) and after['emitted'] == before['emitted'] == 160
    for name in scaled:
        model.store.assign(name, w[name])
    nxt = s.push(mel_t[None, 3:6], z=z_t[None, 160:400])
    assert torch.equal(torch.cat([first[0], nxt[0]]), want[0][:400])


@pytest.mark.parametrize('precision', PRECISIONS)
def test_guard_bands_around_histories_and_accumulators(gpu, precision):
    """The histories inside a 0xFF-filled buffer (tests/guarded.py, via hist_alloc) and every tensor the engine makes -- the per-chunk skip
    accumulators and the residual buffers among them -- between guard bands and filled with NaN (guarded(engine)), on the wide model: after
    uniform pushes of 80 rows (a partial last unit: a full-tile accumulator store would run past the rows) and a ragged push no NaN in a
    live block or in the audio, no mark in a band, the blocks of the slot that was never pushed still zero -- and the pushed slots equal
    their one-shot forwards."""
    from pwv_amd import engine
    cfg = _wide()
    plain, w = _model(gpu, cfg, precision)
    ins = [_inputs(cfg, 8, gpu, seed=50 + i) for i in range(2)]
    wants = [_one_shot(plain, u[2], u[3]).clone() for u in ins]
    with guarded(engine) as bands:
        model, _ = _model(gpu, cfg, precision, weights=w)
        held = []

        def hist_alloc(floats):
            t = bands.allocate((floats,), torch.float32, gpu, 0.0)
            held.append(bands.find(t))
            return t
        s = model.open_stream(slots=3, hist_alloc=hist_alloc, **OPEN)
        hist, = held
        utts = [(u[2], u[3]) for u in ins]
        got = _push_frames(s, [0, 2], utts, [1, 2, 1])
        pieces = s.push_varlen([utts[0][0][4:8], utts[1][0][4:5]], slots=[0, 2], z=[utts[0][1][240:560], utts[1][1][240:320]])
        torch.cuda.synchronize()
        bands.check()
        shapes = [a.shape for a in bands.allocations]
        for rows in (2 * HOP, HOP):          # the uniform pushes' chunk; the ragged push's group of one 80-row session: 2.5 units
            assert (engine._lib.lib().pwv_tile32_floats(rows, 128),) in shapes, ('no guarded skip accumulator of %d rows' % rows, shapes)
        blocks = hist.payload().view(6, -1)
        assert not bool(torch.isnan(blocks).any()) and not bool(blocks[2:4].any()) and bool(blocks[0:2].any()) and bool(blocks[4:6].any())
        for k in range(2):
            whole = torch.cat([got[k], pieces[k]])
            assert not bool(torch.isnan(whole).any()) and torch.equal(whole, wants[k][:whole.shape[0]]), k


def test_state_round_trip_and_foreign_state(gpu):
    """state / load_state across two streams continues bit for bit; a state from a stream without skip sums (another layout) is turned
    away by its block_floats, in both directions."""
    cfg, w, model, ins, want = _reference(gpu, 'f16x3')
    mel_t, z_t = ins[0][2], ins[0][3]
    a, b = model.open_stream(slots=2, **OPEN), model.open_stream(slots=3, **OPEN)
    first = a.push(mel_t[None, :3], slots=[1], z=z_t[None, :160])
    st = a.state(1)
    assert st['block_floats'] == a.layout.block_floats and st['emitted'] == 160
    b.load_state(2, st)
    nxt_b = b.push(mel_t[None, 3:6], slots=[2], z=z_t[None, 160:400])
    nxt_a = a.push(mel_t[None, 3:6], slots=[1], z=z_t[None, 160:400])
    assert torch.equal(nxt_a, nxt_b) and torch.equal(torch.cat([first[0], nxt_b[0]]), want[0][:400]) and b.emitted(2) == 400
    plain_model, _ = _model(gpu, hop_cfg(HOP))
    plain = plain_model.open_stream(slots=1)
    with pytest.raises(ValueError, match='another shape'):
        a.load_state(0, plain.state(0))
    with pytest.raises(ValueError, match='another shape'):
        plain.load_state(0, st)
    set_hparams(cfg)


def test_graph_wrappers_refuse_and_the_stream_goes_on(gpu):
    from pwv_amd._lib import PwvError
    from pwv_amd.audio_frontend import StreamingMel
    cfg, _, model, ins, want = _reference(gpu, 'f16x3')
    s = model.open_stream(slots=2, **OPEN)
    first = _push_frames(s, [0, 1], [(u[2], u[3]) for u in ins], [2])
    for make in (lambda: s.graphed(2, 1), lambda: s.graphed_varlen(2, 160), lambda: s.graphed_live(StreamingMel(2, device=gpu), 2, 160)):
        with pytest.raises(PwvError, match=r'skip accumulation \(use_skip_connection\) streams on per-layer launches only'):
            make()
    assert s._ticker is None and s._pending is None
    nxt = s.push(torch.stack([u[2][2:4] for u in ins]), z=torch.stack([u[3][80:240] for u in ins]))
    for i in range(2):
        assert torch.equal(torch.cat([first[i], nxt[i]]), want[i][:240]), i


def test_generate_cli_stream(gpu, tmp_path, monkeypatch):
    """`generate bench/skip --stream=2` (the case cut down to one flow of four layers, as a user's hparams.yaml would) on three .npy mels
    writes what the non-streamed `--varlen --seed=S` run writes, sample for sample, when the stream's sessions draw the seed S; --graph and
    --live=graph raise the named refusal."""
    from scipy.io import wavfile
    from pwv_amd import engine
    from pwv_amd._lib import PwvError
    from pwv_amd.generate import _fire, generate
    from pwv_amd.hparam import hparam as hp
    rng = np.random.default_rng(4)
    frames = [3, 12, 6]
    for i, f in enumerate(frames):
        np.save(str(tmp_path / ('m%d.npy' % i)), rng.uniform(-1, 1, (f, 80)).astype(np.float32))
    logdir = tmp_path / 'out'
    monkeypatch.setenv('PWV_LOGDIR', str(logdir))
    orig = type(hp).set_hparam_yaml

    def patched(self, case, *a, **k):          # what a user's hparams.yaml case would override
        r = orig(self, case, *a, **k)
        self.data_path = str(tmp_path / '*.npy')
        self.train.dataset_ratio, self.generate.batch_size = 0.0, 3
        self.model.n_iaf, self.model.dilations = 1, [[1, 2, 4, 8]]
        return r

    monkeypatch.setattr(type(hp), 'set_hparam_yaml', patched)
    monkeypatch.setattr(engine, 'os_seed', lambda: 1234)
    pred = _fire(generate, ['bench/skip', '--stream=2'])
    assert hp.model.use_skip_connection is True
    assert [p.shape for p in pred] == [((f - 1) * 80, 1) for f in frames]
    for i, f in enumerate(frames):
        rate, data = wavfile.read(str(logdir / ('pred_%d.wav' % i)))
        assert data.shape == ((f - 1) * 80,)
    monkeypatch.setenv('PWV_LOGDIR', str(tmp_path / 'out_varlen'))          # (a directory that exists is searched for a checkpoint)
    one_shot = _fire(generate, ['bench/skip', '--varlen', '--seed=1234'])
    assert [p.shape for p in one_shot] == [p.shape for p in pred]
    for i, (a, b) in enumerate(zip(pred, one_shot)):
        assert np.array_equal(np.asarray(a), np.asarray(b)), (i, float(np.abs(np.asarray(a) - np.asarray(b)).max()))
    for flags in (['--graph'], ['--live=graph']):
        with pytest.raises(PwvError, match=r'skip accumulation \(use_skip_connection\) streams on per-layer launches only'):
            _fire(generate, ['bench/skip', '--stream=2'] + flags)


def test_trained_checkpoint_streams(gpu, tmp_path):
    """`python -m pwv_amd.train train/small_skip --steps=2` writes a checkpoint that `generate train/small_skip --stream=5` loads and
    streams: finite audio of the case's length, nothing refused."""
    env = dict(os.environ, PWV_LOGDIR=str(tmp_path), PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = subprocess.run([sys.executable, '-m', 'pwv_amd.train', 'train/small_skip', '--steps=2', '--seed=4'], cwd=ROOT, env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert out.returncode == 0 and (tmp_path / 'model-2.npz').exists(), out.stdout[-3000:]
    gen = subprocess.run([sys.executable, '-m', 'pwv_amd.generate', 'train/small_skip', '--stream=5'], cwd=ROOT, env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert gen.returncode == 0 and 'No checkpoint found' not in gen.stdout, gen.stdout[-3000:]
    with np.load(str(tmp_path / 'pred_wav_varlen.npz')) as z:
        pred = z['pred_0']
    assert pred.shape == (1600, 1) and np.isfinite(pred).all() and np.abs(pred).max() > 0
