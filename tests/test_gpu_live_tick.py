"""GPU: the LIVE tick -- wav chunks in, wav chunks out, one graph launch (graph.GraphedLiveStream, StreamingVocoder.graphed_live;
live_tick_mel_kernel / live_tick_commit_kernel in csrc/pwv_audio.hip, include/pwv_hip_live_tick.h).  The contract: whatever the chunking,
the pieces of a session concatenate `torch.equal` to generate_varlen([wav_to_mel_device(wav)], seeds=[seed]) and to the eager
fe.push / fe.finish / push_varlen sequence; both halves of a session are committed or refused together; a tick that does not fit runs
eagerly with the same bits."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.test_gpu_mel_stream import _one_shot as _mel_one_shot, _signals
from tests.test_gpu_stream import _model
from tests.test_gpu_stream_persist import knobs      # noqa: F401  (the fixture)
from tests.test_gpu_stream_ragged_graph import hop_80_afterwards      # noqa: F401  (the fixture)
from tests.util import hop_cfg

pytestmark = pytest.mark.gpu

DEFAULT = SimpleNamespace(name='default', sr=16000, n_fft=512, win_length=400, hop_length=80, n_mels=80, max_db=35.0, min_db=-55.0)
HOP16 = SimpleNamespace(name='hop16', sr=16000, n_fft=64, win_length=40, hop_length=16, n_mels=80, max_db=35.0, min_db=-55.0)
LENGTHS = (1040, 1700, 2400)
SEEDS = (11, (1 << 63) + 7, 5)


def _wavs(gpu, lengths=LENGTHS, first=0):
    """Signals first, first + 1, ... of test_gpu_mel_stream (decaying tone, silence then noise, near the floor, square wave), cut."""
    begin = (0, 6000, 7900, 0)          # (into the loud part of the second signal, 100 samples ahead of the quiet part of the third)
    return [torch.from_numpy(_signals()[(first + i) % 4, begin[(first + i) % 4]:begin[(first + i) % 4] + L].copy()).to(gpu)
            for i, L in enumerate(lengths)]


def _noise(gpu, lengths, hop, seed=3):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy(np.clip(rng.logistic(0, 1, (L // hop * hop, 1)), -20, 20).astype(np.float32)).to(gpu) for L in lengths]


def _want(model, geom, wav, seed=None, z=None):
    """The one-shot pair on the whole utterance: the one-shot front-end, then generate_varlen on its noise stream (or on z)."""
    if geom is DEFAULT:          # (the hparams' own geometry: the public one-shot call)
        from pwv_amd.audio_frontend import wav_to_mel_device
        mel = wav_to_mel_device(wav[None])[0]
    else:
        mel = _mel_one_shot(geom, wav[None])[0]
    if z is not None:
        return model.generate_varlen([mel], z=z)[0]
    return model.generate_varlen([mel], seeds=[seed])[0]


class _Feed(object):
    """Sessions, their wavs and how far each has got: tick(which) = the arguments of one live tick that gives every session of `which`
    its next chunk (sizes[i] samples), starting it with its first chunk and ending it with its last."""

    def __init__(self, geom, wavs, sizes, seeds, zs=None, slots=None):
        self.geom, self.wavs, self.sizes, self.seeds, self.zs = geom, wavs, list(sizes), seeds, zs
        self.slots = list(range(len(wavs))) if slots is None else slots
        self.pos, self.K, self.out = [0] * len(wavs), [0] * len(wavs), [0] * len(wavs)
        self.got = [[] for _ in wavs]

    def left(self):
        return [i for i, w in enumerate(self.wavs) if self.pos[i] < w.shape[0]]

    def args(self, which=None):
        from pwv_amd.audio_frontend import frames_ready
        which = self.left() if which is None else which
        g, chunks, starts, ends, z = self.geom, [], {}, [], []
        for i in which:
            L, n = self.wavs[i].shape[0], self.sizes[i]
            chunks.append(self.wavs[i][self.pos[i]:self.pos[i] + n])
            if self.pos[i] == 0:
                starts[self.slots[i]] = self.seeds[i]
            R = min(self.pos[i] + n, L)
            if R == L:
                ends.append(self.slots[i])
            K1 = 1 + L // g.hop_length if R == L else frames_ready(R, g.n_fft, g.hop_length)
            samples = (K1 - self.K[i] - (1 if self.K[i] == 0 and K1 > 0 else 0)) * g.hop_length
            if self.zs is not None:
                z.append(self.zs[i][self.out[i]:self.out[i] + samples])
            self.pos[i], self.K[i], self.out[i] = R, K1, self.out[i] + samples
        return which, chunks, [self.slots[i] for i in which], starts, ends, (z if self.zs is not None else None)

    def tick(self, live, which=None):
        which, chunks, slots, starts, ends, z = self.args(which)
        got = live.tick(chunks, slots, starts=starts, ends=ends, z=z)
        assert len(got) == len(which)
        for i, piece in zip(which, got):
            self.got[i].append(piece.clone())
        return got

    def state(self):
        return (list(self.pos), list(self.K), list(self.out), [len(g) for g in self.got])

    def rewind(self, state):
        self.pos, self.K, self.out = list(state[0]), list(state[1]), list(state[2])
        self.got = [g[:n] for g, n in zip(self.got, state[3])]

    def result(self, i):
        return torch.cat(self.got[i])


def _eager_sequence(model, geom, feed_args, n_slots, sample):
    """The ticks `feed_args` (a list of _Feed.args() results) as the eager sequence on a fresh front-end and stream: per session the
    concatenated samples."""
    from pwv_amd.audio_frontend import StreamingMel
    fe, s = StreamingMel(n_slots, signal=geom), model.open_stream(slots=n_slots)
    out, begun, wait = {}, set(), {}
    for which, chunks, slots, starts, ends, z in feed_args:
        for sl in starts:
            fe.reset(sl)
            begun.discard(sl)
            wait[sl] = starts[sl]          # (the seed waits for the utterance's first frame)
        fed = [k for k, c in enumerate(chunks) if c.shape[0]]
        frames = {k: [] for k in range(len(slots))}
        for k, p in zip(fed, fe.push([chunks[k] for k in fed], slots=[slots[k] for k in fed])):
            frames[k].append(p)
        for sl in ends:
            frames[slots.index(sl)].append(fe.finish(sl))
        part = [k for k in range(len(slots)) if sum(p.shape[0] for p in frames[k])]
        if not part:
            continue
        for k in part:
            if slots[k] not in begun:
                s.reset(slots[k], wait.pop(slots[k], None))
        got = s.push_varlen([torch.cat(frames[k]) for k in part], slots=[slots[k] for k in part], z=None if sample else [z[k] for k in part])
        for k, piece in zip(part, got):
            begun.add(slots[k])
            out.setdefault(which[k], []).append(piece)
    return {i: torch.cat(p) for i, p in out.items()}


def _bits_case(gpu, engine, precision, sample, guard=None):
    """Case 1 / 2 / 7: three sessions of 1040, 1700 and 2400 samples at a capacity of 3 slots / 2400 rows, chunks of 400 samples, the
    first session fed 200 (its first tick brings no frame: its vocoder side starts in the second tick)."""
    from pwv_amd.audio_frontend import StreamingMel
    cfg = hop_cfg(80)
    model, _ = _model(gpu, cfg, precision)
    wavs = _wavs(gpu)
    zs = None if sample else _noise(gpu, LENGTHS, 80)
    fe, s = StreamingMel(4, signal=DEFAULT), model.open_stream(slots=4)          # (a slot to spare: the filler of a tick of all three)
    live = s.graphed_live(fe, 3, 2400, sample=sample)
    assert live.sessions == 3 and live.slots == 4 and live.wav_cap == 2400 + 3 * (256 + 80)
    feed = _Feed(DEFAULT, wavs, [200, 400, 400], SEEDS, zs)
    log, n_ticks = [], 0
    while feed.left():
        before = feed.state()
        log.append(feed.args())
        feed.rewind(before)
        got = feed.tick(live)
        if n_ticks == 0:
            assert got[0].shape == (0, 1) and got[1].shape == (80, 1) and got[2].shape == (80, 1)
            assert fe._live is live and s._ticker is live
        n_ticks += 1
    assert live.verify() == n_ticks == 6 and live.eager_calls == 0 and live.captures == 1
    assert [fe.received(i) for i in range(3)] == [0, 0, 0] and [fe.emitted(i) for i in range(3)] == [0, 0, 0]
    assert [s.emitted(i) for i in range(3)] == [L // 80 * 80 for L in LENGTHS]
    eager = _eager_sequence(model, DEFAULT, log, 4, sample)
    for i, L in enumerate(LENGTHS):
        got = feed.result(i)
        want = _want(model, DEFAULT, wavs[i], SEEDS[i], None if sample else zs[i])
        assert got.shape == want.shape == (L // 80 * 80, 1) and bool(torch.isfinite(got).all())
        assert torch.equal(got, want), (i, float((got - want).abs().max()))
        assert torch.equal(got, eager[i]), i
        if guard is not None:
            assert not bool(torch.isnan(got).any())
    return live, fe, s


@pytest.mark.parametrize('precision', ['f16x3', 'f32'])
def test_bits_of_the_one_shot_and_of_the_eager_sequence(gpu, knobs, precision):
    _bits_case(gpu, knobs, precision, True)


@pytest.mark.parametrize('precision', ['f16x3', 'f32'])
def test_bits_without_a_sampler(gpu, knobs, precision):
    _bits_case(gpu, knobs, precision, False)


def test_hop_16_geometry(gpu, knobs, hop_80_afterwards):      # noqa: F811
    """n_fft 64, win_length 40, hop 16, min_frames 2: chunks of 96 samples (6 frames a tick), a start of three frames, ends with the last
    chunk -- all graphed; the same bits."""
    from pwv_amd.audio_frontend import StreamingMel
    cfg = hop_cfg(16)
    model, _ = _model(gpu, cfg)
    lengths = (400, 290)
    wavs = _wavs(gpu, lengths, first=1)
    fe, s = StreamingMel(3, signal=HOP16), model.open_stream(slots=3)
    live = s.graphed_live(fe, 2, 320)
    assert live.min_frames == 2 and live.wav_cap == 320 + 2 * (32 + 16)
    feed = _Feed(HOP16, wavs, [96, 96], (21, 22))
    n = 0
    while feed.left():
        feed.tick(live)
        n += 1
    assert live.verify() == n and live.eager_calls == 0 and live.captures == 1
    for i, L in enumerate(lengths):
        want = _want(model, HOP16, wavs[i], (21, 22)[i])
        assert feed.result(i).shape == (L // 16 * 16, 1) and torch.equal(feed.result(i), want), i


def test_slot_reuse_and_a_loud_utterance(gpu, knobs):
    """Slot 1 ends an utterance in tick k and starts the next one in tick k + 1 with no verify() in between; both are their one-shots.  A
    third utterance on the same slot, scaled by 100, goes over min_db + top_db: the next verify() raises naming top_db and slot 1
    alone -- although the utterance has ended and the slot has been started again inside the window."""
    from pwv_amd._lib import PwvError
    from pwv_amd.audio_frontend import StreamingMel
    cfg = hop_cfg(80)
    model, _ = _model(gpu, cfg)
    sig = _signals()
    a, b, other = (torch.from_numpy(sig[k, :L].copy()).to(gpu) for k, L in ((0, 1040), (3, 1200), (3, 2400)))
    loud = torch.from_numpy(sig[0, :800].copy()).to(gpu) * 100.0
    fe, s = StreamingMel(3, signal=DEFAULT), model.open_stream(slots=3)
    live = s.graphed_live(fe, 2, 1600)
    one = _Feed(DEFAULT, [a, other], [400, 400], (31, 41), slots=[1, 2])
    n = 0
    while 0 in one.left():
        one.tick(live)
        n += 1
    two = _Feed(DEFAULT, [b, other], [400, 400], (32, 41), slots=[1, 2])
    two.pos[1], two.K[1], two.got[1] = one.pos[1], one.K[1], one.got[1]
    while 0 in two.left():
        two.tick(live)
        n += 1
    assert live.verify() == n and live.eager_calls == 0
    assert torch.equal(one.result(0), _want(model, DEFAULT, a, 31)) and torch.equal(two.result(0), _want(model, DEFAULT, b, 32))
    assert not two.left() and torch.equal(two.result(1), _want(model, DEFAULT, other, 41))          # (the companion ended with it)
    three = _Feed(DEFAULT, [loud], [400], (33,), slots=[1])
    while three.left():
        three.tick(live)
    four = _Feed(DEFAULT, [a], [400], (34,), slots=[1])          # the slot starts again inside the window
    four.tick(live)
    with pytest.raises(PwvError, match=r'top_db.*slot\(s\) \[1\]|slot\(s\) \[1\].*top_db'):
        live.verify()
    assert fe.received(1) == 400 and fe.emitted(1) == 2          # (everything committed: the report is about the bits, not the state)
    while four.left():
        four.tick(live)
    live.verify()                                                 # (the flag was the host's to clear)
    assert torch.equal(four.result(0), _want(model, DEFAULT, a, 34))


def test_refused_ticks_leave_both_halves_behind_the_committed_prefix(gpu, knobs):
    """Nothing on the GPU is made to fail: the give-up word is set by a host write between ticks.  Two ticks commit, two are refused on
    the device: verify() raises with .committed == 2, and fe.received / fe.emitted, the carry block each session will read and s.emitted
    are what the first two ticks left.  The same chunks fed again -- eagerly while the suspension lasts, graphed after it -- finish to the
    one-shot's bits."""
    from pwv_amd._lib import PwvPersistError
    from pwv_amd.audio_frontend import StreamingMel
    engine = knobs
    cfg = hop_cfg(80)
    model, _ = _model(gpu, cfg)
    lengths = (2000, 2400)
    wavs = _wavs(gpu, lengths)
    fe, s = StreamingMel(3, signal=DEFAULT), model.open_stream(slots=3)
    live = s.graphed_live(fe, 2, 1600)
    feed = _Feed(DEFAULT, wavs, [400, 400], (51, 52))
    feed.tick(live)
    feed.tick(live)
    torch.cuda.synchronize()
    kept = feed.state()
    table = fe._sess.cpu()
    blocks = [fe._state[2 * i + (int(table[i, 0]) & 1)].clone() for i in range(2)]
    assert table[:2, 1].tolist() == [800, 800] and table[:2, 2].tolist() == [7, 7] and not bool(table[2].any())
    engine.poke_persist_status(4)
    feed.tick(live)
    feed.tick(live)                                # refused too: the word is sticky
    with pytest.raises(PwvPersistError) as ei:
        live.verify()
    assert ei.value.committed == 2 and s._pending is None and fe._live is None
    assert [fe.received(i) for i in range(2)] == [800, 800] and [fe.emitted(i) for i in range(2)] == [7, 7]
    assert [s.emitted(i) for i in range(2)] == [480, 480]
    for i in range(2):
        assert fe._gen[i] == int(table[i, 0]) & 1 and torch.equal(fe._state[2 * i + fe._gen[i]], blocks[i])
    assert torch.equal(fe._sess.cpu(), table)
    assert engine.persist_suspended() and live.graph is None
    feed.rewind(kept)
    feed.tick(live)                                # eager: the suspension
    assert live.eager_calls == 1
    assert live.verify() == 1
    engine.resume_persist()
    n = 0
    while feed.left():
        feed.tick(live)
        n += 1
    assert live.verify() == n and live.captures == 2 and live.eager_calls == 1
    for i in range(2):
        assert torch.equal(feed.result(i), _want(model, DEFAULT, wavs[i], (51, 52)[i])), i


def test_ticks_that_go_eager(gpu, knobs):
    """A tick that brings more samples than the capacity holds, and a start with one ready frame (fewer than min_frames + 1), run the eager
    sequence inside tick(): counted in eager_calls, the same bits; the ticks around them replay the graph."""
    from pwv_amd.audio_frontend import StreamingMel
    cfg = hop_cfg(80)
    model, _ = _model(gpu, cfg)
    lengths = (2400, 1300)
    wavs = _wavs(gpu, lengths, first=3)
    fe, s = StreamingMel(3, signal=DEFAULT), model.open_stream(slots=3)
    live = s.graphed_live(fe, 2, 1600)
    feed = _Feed(DEFAULT, wavs, [300, 400], (61, 62))
    feed.tick(live, [0])                           # 300 samples: frame 0 alone is ready -- a start of one frame
    assert live.eager_calls == 1 and s._running[0] and s.emitted(0) == 0
    feed.tick(live)                                # graphed: slot 0 goes on, slot 1 starts with two frames
    assert live.eager_calls == 1 and s._ticker is live
    feed.sizes = [1200, 400]
    feed.tick(live)                                # 15 + 5 frames and a filler against 20: settles the tick in flight, runs eagerly
    assert live.eager_calls == 2 and s._ticker is None
    feed.sizes = [300, 300]
    n = 0
    while feed.left():
        feed.tick(live)
        n += 1
    assert n == 2 and live.verify() == n + 3 and live.eager_calls == 2 and live.captures == 1
    for i in range(2):
        assert torch.equal(feed.result(i), _want(model, DEFAULT, wavs[i], (61, 62)[i])), i


def test_interleaving_with_the_eager_calls(gpu, knobs):
    """One session advanced alternately by live ticks and by the eager fe.push / push_varlen: with ticks in flight the eager calls raise
    and name verify(); after it the host's views are the device tables', and the next live tick rewrites the rows the eager calls moved.
    The concatenation is the one-shot."""
    from pwv_amd._lib import PwvError
    from pwv_amd.audio_frontend import StreamingMel
    cfg = hop_cfg(80)
    model, _ = _model(gpu, cfg)
    L, seed = 2400, 71
    wav = _wavs(gpu, (L,), first=1)[0]
    fe, s = StreamingMel(2, signal=DEFAULT), model.open_stream(slots=2)
    live = s.graphed_live(fe, 2, 800)
    out, pos = [], 0
    for how, n in (('live', 400), ('eager', 300), ('live', 500), ('live', 320), ('eager', 480), ('live', 400)):
        chunk, end = wav[pos:pos + n], pos + n >= L
        if how == 'live':
            out.append(live.tick([chunk], [1], starts={1: seed} if pos == 0 else None, ends=[1] if end else None)[0].clone())
            with pytest.raises(PwvError, match='verify'):
                fe.push([chunk], slots=[1])
            with pytest.raises(PwvError, match='verify'):
                fe.finish(1)
            with pytest.raises(PwvError, match='verify'):
                s.push_varlen([torch.zeros((1, 80), device=gpu)], slots=[1])
        else:
            live.verify()
            assert fe.received(1) == pos and s.emitted(1) == sum(o.shape[0] for o in out)
            out.append(s.push_varlen([fe.push([chunk], slots=[1])[0]], slots=[1])[0])
        pos += n
    assert pos == L and live.verify() == 1 and live.eager_calls == 0
    got, want = torch.cat(out), _want(model, DEFAULT, wav, seed)
    assert got.shape == want.shape and torch.equal(got, want)


def test_bits_inside_guarded_buffers(gpu, knobs):
    """Case 1 with every buffer of the package inside poisoned, guard-banded allocations (tests/guarded.py): no NaN in an output or a carry
    block, no mark in a band."""
    from pwv_amd import audio_frontend, engine, graph, stream
    from tests.guarded import guarded
    with guarded(audio_frontend, engine, graph, stream) as g:
        live, fe, s = _bits_case(gpu, knobs, 'f16x3', True, guard=g)
        assert g.holds(fe._state) and g.holds(fe._sess) and g.holds(live._wav) and g.holds(live._rec) and g.holds(live._scratch)
        assert g.holds(live.mel) and g.holds(live._first)
        torch.cuda.synchronize()
        assert not bool(torch.isnan(fe._state).any())
        g.check()


def test_generate_cli_stream_live_graph_writes_what_varlen_writes(gpu, tmp_path, monkeypatch):
    """generate CASE --stream=5 --live=graph on three short wavs: the files and sample counts of --varlen, through graphed live ticks."""
    from scipy.io import wavfile
    from pwv_amd import graph
    from pwv_amd.generate import _fire, generate
    from pwv_amd.hparam import hparam as hp
    sr = 16000
    for i, n in enumerate((2400, 1700, 3300)):
        t = np.arange(n + 1500) / sr
        wav = 0.3 * np.sin(2 * np.pi * (200 + 40 * i) * t) * (t > 0.05)
        wavfile.write(str(tmp_path / ('a%02d.wav' % i)), sr, (wav * 32767).astype(np.int16))
    orig = type(hp).set_hparam_yaml

    def patched(self, case, *a, **k):
        r = orig(self, case, *a, **k)
        self.data_path = str(tmp_path / '*.wav')
        self.train.dataset_ratio = 0.0
        self.generate.batch_size = 3
        self.model.n_iaf, self.model.dilations = 1, [[1, 2, 4, 8]]
        return r

    monkeypatch.setattr(type(hp), 'set_hparam_yaml', patched)
    ticks, real = [], graph.GraphedLiveStream.tick

    def counting(self, *a, **k):
        out = real(self, *a, **k)
        ticks.append(self.eager_calls)
        return out

    monkeypatch.setattr(graph.GraphedLiveStream, 'tick', counting)
    counts = {}
    for key, argv in (('varlen', ['default', '--varlen']), ('live', ['default', '--stream=5', '--live=graph'])):
        logdir = tmp_path / key
        monkeypatch.setenv('PWV_LOGDIR', str(logdir))
        pred = _fire(generate, argv)
        assert len(pred) == 3 and all(np.isfinite(p).all() for p in pred)
        counts[key] = [wavfile.read(str(logdir / ('pred_%d.wav' % i)))[1].shape[0] for i in range(3)]
        assert counts[key] == [len(p) for p in pred] and (logdir / 'pred_wav_varlen.npz').exists()
    assert counts['live'] == counts['varlen'] and len(set(counts['varlen'])) == 3 and all(c % 80 == 0 and c > 400 for c in counts['varlen'])
    assert len(ticks) >= 5 and ticks.count(0) >= 3          # graphed ticks carried the run (the short tails may run eagerly)
