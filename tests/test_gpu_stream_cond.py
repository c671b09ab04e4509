"""GPU: streaming a transposed-conv model (IAFVocoder.open_stream(slots, transposed_conv=True) -> pwv_wavenet_layer_stream_cond_f32, the head
launch, the affine).  The contract is that of tests/test_gpu_stream.py: the pushes of a session, concatenated, are torch.equal to the
one-shot forward IAFVocoder(1, L)(None, mel, z=z) at the same precision -- which this route does not touch --, a session's audio does not
depend on its companions, a push is a transaction.  Smallest shapes: two sessions of the model hop_cfg(80, transposed_conv) put a session
boundary inside a 32-row unit at every push of one frame (80 rows)."""
import numpy as np
import pytest
import torch

from oracle import iaf_oracle as O
from tests.guarded import Guard
from tests.util import TOL_F32, hop_cfg, saturated_case, set_hparams, small_cfg

pytestmark = pytest.mark.gpu
HOP = 80
PRECISIONS = ['f16x3', 'f32']


def _tconv(**kw):
    return hop_cfg(HOP, cond_upsample_method='transposed_conv', **kw)


def _wide():
    # the tconv analogue of tests/test_gpu_stream.py::_small_wide: most dilations above the 80-sample chunk, two that are no multiple of 32
    return small_cfg(dilations=[[1, 96, 128, 256], [2, 64, 200, 512, 3, 160]], cond_upsample_method='transposed_conv')


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
        cfg = _tconv()
        model, w = _model(gpu, cfg, precision)
        ins = [_inputs(cfg, 8, gpu, seed=60 + i) for i in range(2)]
        _REF[precision] = (cfg, w, ins, [_one_shot(model, u[2], u[3]).clone() for u in ins])
    cfg, w, ins, want = _REF[precision]
    model, _ = _model(gpu, cfg, precision, weights=w)
    return cfg, w, model, ins, want


@pytest.mark.parametrize('schedule', [[1, 1, 2, 3, 1], [4, 1, 1], [7]], ids=['1-1-2-3-1', '4-1-1', '7'])
@pytest.mark.parametrize('precision', PRECISIONS)
def test_chunks_equal_the_one_shot_forward(gpu, precision, schedule):
    """Two sessions advanced together; the first push of one frame yields an empty piece.  torch.equal, both arithmetics."""
    cfg, _, model, ins, want = _reference(gpu, precision)
    s = model.open_stream(slots=2, transposed_conv=True)
    got = _push_frames(s, [0, 1], [(u[2], u[3]) for u in ins], schedule)
    L = (sum(schedule) - 1) * HOP
    assert s.emitted(0) == s.emitted(1) == L
    for i in range(2):
        assert torch.equal(got[i], want[i][:L]), (i, float((got[i] - want[i][:L]).abs().max()))


@pytest.mark.parametrize('precision', PRECISIONS)
def test_wide_model_one_frame_pushes(gpu, precision):
    """Dilations up to 512 against chunks of 80 rows: every history is longer than the chunk, the carry launch runs at every push, and at
    720 samples the look-back of 512 reads rows that were carried over six times."""
    cfg = _wide()
    model, _ = _model(gpu, cfg, precision)
    _, _, mel_t, z_t = _inputs(cfg, 10, gpu, seed=1)
    s = model.open_stream(slots=1, transposed_conv=True)
    got = _push_frames(s, [0], [(mel_t, z_t)], [1] * 10)[0]
    want = _one_shot(model, mel_t, z_t)
    assert torch.equal(got, want), float((got - want).abs().max())


@pytest.mark.parametrize('precision', PRECISIONS)
def test_stage_gemm_rows_do_not_depend_on_the_row_count(gpu, precision):
    """What both the chunked and the ragged route rest on: the three stage GEMMs on 3 frames give, bit for bit, the rows they give for those
    frames inside a 9-frame run (uncropped stage-3 output: 80 rows per frame)."""
    from pwv_amd.variables import variable_scope
    cfg = _tconv()
    model, _ = _model(gpu, cfg, precision)
    _, _, mel_t, _ = _inputs(cfg, 9, gpu, seed=3)

    def stages(frames):
        with variable_scope('iaf_vocoder'), variable_scope('cond'):
            return model._condition(frames[None], False, strides=[4, 4, 5], store=model.store, precision=precision,
                                    length=(frames.shape[0] - 1) * HOP, crop=False)[0]
    whole, part = stages(mel_t), stages(mel_t[4:7])
    assert tuple(whole.shape) == (9 * HOP, cfg.condition_channels) and tuple(part.shape) == (3 * HOP, cfg.condition_channels)
    assert torch.equal(part, whole[4 * HOP:7 * HOP]) and bool(part.abs().sum() > 0)


@pytest.mark.parametrize('precision', PRECISIONS)
def test_stream_matches_oracle(gpu, precision):
    """Against the fp64 oracle at the fp32 bar of every parity test (enqueue-only + verify(): no self-repair)."""
    cfg, w, model, ins, _ = _reference(gpu, precision)
    s = model.open_stream(slots=2, transposed_conv=True)
    got = _push_frames(s, [0, 1], [(u[2], u[3]) for u in ins], [2, 1, 3, 2], verify=False)
    for i in range(2):
        want = O.iaf_vocoder_forward(w, ins[i][0][None], ins[i][1][None], cfg)[0]
        err = float(np.abs(got[i].cpu().numpy() - want).max())
        print('tconv stream vs oracle, %s, slot %d: %.3g' % (precision, i, err))
        assert err <= TOL_F32, err


def test_sessions_are_independent(gpu):
    """The same utterance pushed alone, beside another session, and on another slot: the same bits."""
    cfg, _, model, ins, want = _reference(gpu, 'f16x3')
    a, b = (ins[0][2], ins[0][3]), (ins[1][2], ins[1][3])
    sched = [2, 1, 3, 2]
    alone = _push_frames(model.open_stream(slots=1, transposed_conv=True), [0], [a], sched)[0]
    beside = _push_frames(model.open_stream(slots=3, transposed_conv=True), [2, 0], [b, a], sched)
    other = _push_frames(model.open_stream(slots=3, transposed_conv=True), [1], [a], sched)[0]
    assert torch.equal(alone, want[0]) and torch.equal(beside[1], alone) and torch.equal(other, alone) and torch.equal(beside[0], want[1])


@pytest.mark.parametrize('precision', PRECISIONS)
def test_ragged_pushes(gpu, precision):
    """push_varlen with frame counts [1, 3, 2] then [2, 1, 4], slot 1 running and slots 0, 2 fresh at the first tick: the pieces equal the same
    sessions advanced by separate push calls, and the one-shot forward; every flow of a launching tick took the grouped route on the
    per-sample layer launches."""
    from pwv_amd import engine
    cfg, _, model, ins, want = _reference(gpu, precision)
    third = _inputs(cfg, 8, gpu, seed=62)
    utts = [(ins[0][2], ins[0][3]), (ins[1][2], ins[1][3]), (third[2], third[3])]
    ticks = [[1, 3, 2], [2, 1, 4]]
    s, ref = model.open_stream(slots=3, transposed_conv=True), model.open_stream(slots=3, transposed_conv=True)
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
            for i in range(3):
                outs[i].append(got[i])
                routs[i].append(ref.push(mels[i][None], slots=[i], z=zs[i][None])[0])
                pos[i] += counts[i]
        log = [e for e in engine.EVENT_LOG if e[0] in ('stream_ragged', 'persist', 'layer_stream')]
    finally:
        engine.EVENT_LOG = saved
    ragged = [e for e in log if e[0] == 'stream_ragged']
    assert len(ragged) == 2 * cfg.n_iaf and all(e[3] == 'grouped' and 'per-sample' in e[4] for e in ragged), log
    assert len(log) == len(ragged)          # neither a persistent launch nor the launches without a condition
    third_want = _one_shot(model, third[2], third[3])
    for i, w_i in enumerate([want[0], want[1], third_want]):
        got_i = torch.cat(outs[i])
        assert torch.equal(got_i, torch.cat(routs[i])), i
        assert got_i.shape[0] == (pos[i] - 1) * HOP and torch.equal(got_i, w_i[:got_i.shape[0]]), i


@pytest.mark.parametrize('precision', PRECISIONS)
def test_shared_net_variant(gpu, precision):
    """shared_nets with transposed_conv: one net of two outputs per flow (G = 1, a head of Q = 2)."""
    cfg = _tconv(shared_nets=True)
    model, _ = _model(gpu, cfg, precision)
    ins = [_inputs(cfg, 7, gpu, seed=70 + i) for i in range(2)]
    s = model.open_stream(slots=2, transposed_conv=True)
    got = _push_frames(s, [0, 1], [(u[2], u[3]) for u in ins], [1, 3, 1, 2])
    for i in range(2):
        assert torch.equal(got[i], _one_shot(model, ins[i][2], ins[i][3])), i


def test_range_rerun_is_transactional(gpu):
    """As tests/test_gpu_stream.py::test_range_rerun_is_transactional: the chunk whose mel trips the range guard of the split-fp16 stage GEMMs
    warns and equals the same chunk pushed by a precision='f32' stream brought to the same state; the stream goes on from the state the
    rerun left."""
    from pwv_amd.models import IAFVocoder
    cfg = _tconv()
    model, _ = _model(gpu, cfg)
    m32 = IAFVocoder(batch_size=1, length=HOP, store=model.store, precision='f32')
    _, _, mel_t, z_t = _inputs(cfg, 10, gpu, seed=40)
    mel_t = mel_t.clone()
    mel_t[4:6] *= 1e5                      # frames 4, 5 of the chunk that brings frames 4, 5, 6
    s = model.open_stream(slots=1, transposed_conv=True)
    first = s.push(mel_t[None, :4], z=z_t[None, :240])
    assert torch.equal(first[0], _one_shot(model, mel_t[:4], z_t[:240]))
    before = s.state(0)
    with pytest.warns(UserWarning, match='rerun in exact fp32'):
        tripped = s.push(mel_t[None, 4:7], z=z_t[None, 240:480])
    assert s.emitted(0) == 480 and bool(torch.isfinite(tripped).all())
    s32 = m32.open_stream(slots=1, transposed_conv=True)
    s32.load_state(0, before)
    want = s32.push(mel_t[None, 4:7], z=z_t[None, 240:480])
    assert torch.equal(tripped, want)
    s2 = model.open_stream(slots=1, transposed_conv=True)
    s2.load_state(0, s32.state(0))
    after = s.push(mel_t[None, 7:], z=z_t[None, 480:])
    assert torch.equal(after, s2.push(mel_t[None, 7:], z=z_t[None, 480:])) and s.emitted(0) == 720


def test_refused_push_leaves_the_session_where_it_was(gpu):
    """A push that only enqueued and is refused at verify() (the range guard): generation, counter, kept frame and the block the session
    stands on are what they were; the same chunk then goes through on an f32 stream of that state."""
    from pwv_amd import engine
    from pwv_amd._lib import PwvRangeError
    from pwv_amd.models import IAFVocoder
    cfg = _tconv()
    model, _ = _model(gpu, cfg)
    _, _, mel_t, z_t = _inputs(cfg, 6, gpu, seed=41)
    s = model.open_stream(slots=1, transposed_conv=True)
    s.push(mel_t[None, :3], z=z_t[None, :160])
    gen, kept, block, before = list(s._gen), s._kept.clone(), s._hist[s._gen[0]].clone(), s.state(0)
    bad = mel_t[3:6].clone()
    bad[:2] *= 1e5
    try:
        s.push(bad[None], z=z_t[None, 160:400], verify=False)
        with pytest.raises(PwvRangeError):
            s.verify()
    finally:
        torch.cuda.synchronize()
        engine.clear_range_flag()
    assert s._gen == gen and s.emitted(0) == 160 and s._pending is None and torch.equal(s._kept, kept) and torch.equal(s._hist[gen[0]], block)
    s32 = IAFVocoder(batch_size=1, length=HOP, store=model.store, precision='f32').open_stream(slots=1, transposed_conv=True)
    s32.load_state(0, before)
    assert bool(torch.isfinite(s32.push(bad[None], z=z_t[None, 160:400])).all()) and s32.emitted(0) == 400


@pytest.mark.parametrize('precision', PRECISIONS)
def test_guard_bands_around_the_histories(gpu, precision):
    """The histories inside a 0xFF-filled buffer (tests/guarded.py) on the wide model: after uniform and ragged pushes no NaN in a live block, no
    mark in a band, the blocks of the slot that was never pushed still zero -- and the pushed slots equal their one-shot forwards."""
    cfg = _wide()
    model, _ = _model(gpu, cfg, precision)
    bands = Guard(band_bytes=1 << 18)
    s = model.open_stream(slots=3, hist_alloc=lambda floats: bands.allocate((floats,), torch.float32, gpu, 0.0), transposed_conv=True)
    ins = [_inputs(cfg, 8, gpu, seed=50 + i) for i in range(2)]
    utts = [(u[2], u[3]) for u in ins]
    got = _push_frames(s, [0, 2], utts, [1, 2, 1])
    pieces = s.push_varlen([utts[0][0][4:8], utts[1][0][4:5]], slots=[0, 2], z=[utts[0][1][240:560], utts[1][1][240:320]])
    torch.cuda.synchronize()
    bands.check()
    blocks = bands.allocations[0].payload().view(6, -1)
    assert not bool(torch.isnan(blocks).any()) and not bool(blocks[2:4].any()) and bool(blocks[0:2].any()) and bool(blocks[4:6].any())
    for k, u in enumerate(ins):
        whole = torch.cat([got[k], pieces[k]])
        assert torch.equal(whole, _one_shot(model, u[2], u[3])[:whole.shape[0]]), k


def test_saturated_gates(gpu):
    """The weights of the saturated-gate route tests (a third of the gates beyond |F| = 20): the stream equals the one-shot forward there too."""
    cfg, w, mel, z = saturated_case('transposed')
    model, _ = _model(gpu, cfg, weights=w)
    mel_t, z_t = torch.from_numpy(mel).to(gpu), torch.from_numpy(z).to(gpu)
    s = model.open_stream(slots=2, transposed_conv=True)
    got = _push_frames(s, [0, 1], [(mel_t[i], z_t[i]) for i in range(2)], [2, 1, 1])
    for i in range(2):
        assert torch.equal(got[i], _one_shot(model, mel_t[i], z_t[i])), i


def test_graph_wrappers_refuse_and_the_stream_goes_on(gpu):
    from pwv_amd._lib import PwvError
    from pwv_amd.audio_frontend import StreamingMel
    cfg, _, model, ins, want = _reference(gpu, 'f16x3')
    s = model.open_stream(slots=2, transposed_conv=True)
    first = _push_frames(s, [0, 1], [(u[2], u[3]) for u in ins], [2])
    for make in (lambda: s.graphed(2, 1), lambda: s.graphed_varlen(2, 160), lambda: s.graphed_live(StreamingMel(2, device=gpu), 2, 160)):
        with pytest.raises(PwvError, match='per-sample .transposed-conv. conditioning'):
            make()
    assert s._ticker is None and s._pending is None
    nxt = s.push(torch.stack([u[2][2:4] for u in ins]), z=torch.stack([u[3][80:240] for u in ins]))
    for i in range(2):
        assert torch.equal(torch.cat([first[i], nxt[i]]), want[i][:240]), i


def test_generate_cli_stream(gpu, tmp_path, monkeypatch):
    """`generate test/tran --stream=5` on three .npy mels writes the sample counts `--varlen` (the one-shot forward of such a case) writes;
    --graph raises the named refusal."""
    from scipy.io import wavfile
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
    pred = _fire(generate, ['test/tran', '--stream=5'])
    assert hp.model.cond_upsample_method == 'transposed_conv'
    assert [p.shape for p in pred] == [((f - 1) * 80, 1) for f in frames]
    for i, f in enumerate(frames):
        rate, data = wavfile.read(str(logdir / ('pred_%d.wav' % i)))
        assert data.shape == ((f - 1) * 80,)
    monkeypatch.setenv('PWV_LOGDIR', str(tmp_path / 'out_varlen'))          # (a directory that exists is searched for a checkpoint)
    one_shot = _fire(generate, ['test/tran', '--varlen'])
    assert [p.shape for p in one_shot] == [p.shape for p in pred]
    with pytest.raises(PwvError, match='per-sample .transposed-conv. conditioning'):
        _fire(generate, ['test/tran', '--stream=5', '--graph'])
