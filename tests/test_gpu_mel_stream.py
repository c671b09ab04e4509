"""GPU: the streaming mel front-end (audio_frontend.StreamingMel, pwv_wav_to_mel_db_stream_f32, stft_mel_stream_kernel).  The contract:
whatever the chunking, the frames a session returns concatenate `torch.equal` to the rows of the one-shot front-end on the whole
utterance; a session does not depend on its companions; a session whose raw dB would have set the one-shot's top_db floor above min_db
is reported, not silently different."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SMALL = SimpleNamespace(name='small', sr=16000, n_fft=32, win_length=20, hop_length=8, n_mels=5, max_db=35.0, min_db=-55.0)
DEFAULT = SimpleNamespace(name='default', sr=16000, n_fft=512, win_length=400, hop_length=80, n_mels=80, max_db=35.0, min_db=-55.0)
# h + 1 (the shortest legal utterance), a length that is no multiple of hop, a multiple of hop
CASES = [(DEFAULT, 257), (DEFAULT, 1000), (DEFAULT, 1040), (SMALL, 17), (SMALL, 100)]
CASE_IDS = ['%s-%d' % (g.name, L) for g, L in CASES]


@functools.lru_cache(maxsize=None)
def _signals():
    """The four signals of test_device_mel_frontend_matches_numpy_restatement, [4, 16000] float32 (cut to L by the caller)."""
    rng = np.random.RandomState(5)
    L = 16000
    t = np.arange(L) / 16000
    wavs = np.stack([
        (0.3 * np.sin(2 * np.pi * 220 * t) * np.exp(-3 * t) + 0.05 * rng.randn(L)),         # decaying tone + noise
        0.8 * rng.randn(L) * (t > 0.3),                                                    # silence then loud noise
        np.concatenate([np.zeros(L // 2), 1e-4 * rng.randn(L // 2)]),                       # near the amin floor
        np.sign(np.sin(2 * np.pi * 50 * t)) * 0.5,                                         # square wave: many harmonics
    ]).astype(np.float32)
    wavs.setflags(write=False)
    return wavs


_REF = {}


def _one_shot(geom, wav):
    """pwv_wav_to_mel_db_f32 (normalised) on wav [N, L] at the geometry `geom`, called directly: [N, 1 + L // hop, n_mels]."""
    from pwv_amd import _lib, audio_frontend as A, engine
    window, basis = A._consts(wav.device, geom)
    n, length = wav.shape
    mel = torch.empty((n, 1 + length // geom.hop_length, geom.n_mels), dtype=torch.float32, device=wav.device)
    _lib.check(_lib.lib().pwv_wav_to_mel_db_f32(wav.data_ptr(), window.data_ptr(), basis.data_ptr(), mel.data_ptr(), n, length, geom.n_fft,
                                                geom.hop_length, geom.n_mels, 1e-5, 80.0, geom.max_db, geom.min_db, 1, engine._stream()),
               'pwv_wav_to_mel_db_f32')
    return mel


def _case(geom, L, gpu):
    """(wav [4, L] on the GPU, the one-shot's frames [4, 1 + L // hop, n_mels]) -- computed once per case, shared, never written to."""
    key = (geom.name, L)
    if key not in _REF:
        wav = torch.from_numpy(_signals()[:, :L].copy()).to(gpu)
        _REF[key] = (wav, _one_shot(geom, wav))
    return _REF[key]


def _chunkings(geom, L):
    h, hop = geom.n_fft // 2, geom.hop_length

    def cut(sizes):
        out, left = [], L
        for n in sizes:
            if left <= 0:
                break
            out.append(min(n, left))
            left -= out[-1]
        assert sum(out) == L
        return out
    return {
        'at_once': [L],
        'edges': cut([h, 1, 1, h - 2, hop, hop, 7] + [hop, hop, 7] * (L // 7 + 1)),          # [256, 1, 1, 254, 80, 80, 7, ...] at the default geometry
        'hops': cut([hop] * (L // hop + 1)),
        'samples': cut([1] * 300 + [L]),                                                 # one sample at a time through the first 300
    }


def _stream_all(fe, wav, sizes, slots=None):
    """Every row of wav [S, L] is a session of `fe` (slots: default 0 .. S - 1); all get the chunk sizes `sizes`, then finish.  Returns
    the concatenated frames per session and the frame counts per push."""
    slots = list(range(wav.shape[0])) if slots is None else slots
    got, counts, pos = [[] for _ in slots], [], 0
    for n in sizes:
        pieces = fe.push([wav[i, pos:pos + n] for i in range(len(slots))], slots=slots)
        counts.append([int(p.shape[0]) for p in pieces])
        for i, p in enumerate(pieces):
            assert p.dim() == 2 and p.shape[1] == fe.n_mels
            got[i].append(p)
        pos += n
    for i, s in enumerate(slots):
        assert fe.received(s) == wav.shape[1]
        got[i].append(fe.finish(s))
    return [torch.cat(g) for g in got], counts


@pytest.mark.parametrize('chunking', ['at_once', 'edges', 'hops', 'samples'])
@pytest.mark.parametrize('geom,L', CASES, ids=CASE_IDS)
def test_streamed_frames_are_the_one_shot_frames(gpu, geom, L, chunking):
    from pwv_amd.audio_frontend import StreamingMel, frames_ready
    wav, want = _case(geom, L, gpu)
    sizes = _chunkings(geom, L)[chunking]
    fe = StreamingMel(4, signal=geom)
    got, counts = _stream_all(fe, wav, sizes)
    # a push emits exactly the frames that became ready
    R, K = 0, 0
    for n, c in zip(sizes, counts):
        R += n
        k1 = frames_ready(R, geom.n_fft, geom.hop_length)
        assert c == [k1 - K] * 4
        K = k1
    for i in range(4):
        assert got[i].shape == want[i].shape == (1 + L // geom.hop_length, geom.n_mels)
        assert torch.equal(got[i], want[i]), (i, int((got[i] != want[i]).sum()), float((got[i] - want[i]).abs().max()))
        assert fe.received(i) == 0 and fe.emitted(i) == 0          # finish leaves the slot fresh


def test_default_geometry_one_shot_is_wav_to_mel_device(gpu):
    """The reference of the cases above at the default geometry is the public one-shot call."""
    from pwv_amd import audio_frontend as A
    from pwv_amd.hparam import hparam as hp
    hp.set_hparam_yaml('default')
    s = hp.signal
    assert (s.sr, s.n_fft, s.win_length, s.hop_length, s.n_mels, s.max_db, s.min_db) == (
        DEFAULT.sr, DEFAULT.n_fft, DEFAULT.win_length, DEFAULT.hop_length, DEFAULT.n_mels, DEFAULT.max_db, DEFAULT.min_db)
    for L in (257, 1000, 1040):
        wav, want = _case(DEFAULT, L, gpu)
        assert torch.equal(A.wav_to_mel_device(wav), want)
    fe = A.StreamingMel(2)                                          # hp.signal
    got, _ = _stream_all(fe, wav[:2], [500, 540])
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert fe.state_bytes() == 2 * 512 * 4 + 4


@pytest.mark.parametrize('geom,L', CASES, ids=CASE_IDS)
def test_streamed_frames_match_the_numpy_restatement(gpu, geom, L):
    """The existing bar of the one-shot kernel, 1e-5 on the normalised mel, for the streamed frames."""
    from pwv_amd import audio_frontend as A
    wav, _ = _case(geom, L, gpu)
    got, _ = _stream_all(A.StreamingMel(4, signal=geom), wav, _chunkings(geom, L)['hops'])
    for i in range(4):
        want = A.wav2melspec_db(_signals()[i, :L], geom.sr, geom.n_fft, geom.win_length, geom.hop_length, geom.n_mels, max_db=geom.max_db,
                                min_db=geom.min_db)
        err = float(np.abs(got[i].cpu().numpy() - want).max())
        print('%s L=%d signal %d: max |streamed - numpy| = %.3g' % (geom.name, L, i, err))
        assert err <= 1e-5


def test_three_sessions_at_different_phases_in_one_push(gpu):
    """One ragged push: slot 2 well into its utterance, slot 0 fresh and given too little for a frame, slot 1 about to end."""
    from pwv_amd.audio_frontend import StreamingMel
    L = 1000
    wav, want = _case(DEFAULT, L, gpu)
    fe = StreamingMel(3, signal=DEFAULT)
    out = {0: [], 1: [], 2: []}
    out[2] += fe.push([wav[2, :300]], slots=[2])
    out[1] += fe.push([wav[1, :700]], slots=[1])
    a, b, c = fe.push([wav[0, :100], wav[1, 700:1000], wav[2, 300:500]], slots=[0, 1, 2])          # THE push
    assert a.shape[0] == 0 and b.shape[0] == 4 and c.shape[0] == 3
    assert c.data_ptr() == b.data_ptr() + 4 * 80 * 4                                             # views of one packed result
    out[0].append(a), out[1].append(b), out[2].append(c)
    assert [fe.received(s) for s in range(3)] == [100, 1000, 500] and [fe.emitted(s) for s in range(3)] == [0, 10, 4]
    out[1].append(fe.finish(1))
    x, y = fe.push([wav[2, 500:], wav[0, 100:]], slots=[2, 0])                                   # (slots in another order than the blocks)
    out[2].append(x), out[0].append(y)
    for s in (0, 2):
        out[s].append(fe.finish(s))
    for s in range(3):
        assert torch.equal(torch.cat(out[s]), want[s]), s


def test_reset_in_mid_utterance_and_reuse(gpu):
    from pwv_amd.audio_frontend import StreamingMel
    L = 100
    wav, want = _case(SMALL, L, gpu)
    fe = StreamingMel(2, signal=SMALL)
    fe.push([wav[0, :57], wav[1, :30]])
    assert fe.received(0) == 57 and fe.emitted(0) == 6
    fe.reset(0)
    assert fe.received(0) == 0 and fe.emitted(0) == 0 and fe.received(1) == 30
    first = fe.push([wav[3, :41], wav[1, 30:]])
    rest = fe.push([wav[3, 41:]], slots=[0])
    assert torch.equal(torch.cat([first[0], rest[0], fe.finish(0)]), want[3])
    assert fe.max_db_seen(1) is not None and fe.max_db_seen(0) is None            # slot 0: fresh after finish
    with pytest.raises(Exception, match='final_len'):                            # nothing received: no utterance to finish
        fe.finish(0)


def test_a_loud_session_is_reported_and_its_companions_are_exact(gpu):
    """A wav scaled by 100 reaches raw dB above min_db + top_db = 25: the one-shot's floor would have been active, and finish says so.
    The sessions that shared its pushes are untouched."""
    from pwv_amd._lib import PwvError
    from pwv_amd.audio_frontend import StreamingMel, TOP_DB
    L = 1040
    wav, want = _case(DEFAULT, L, gpu)
    loud = wav[0] * 100.0
    fe = StreamingMel(3, signal=DEFAULT)
    out = {0: [], 2: []}
    for lo in range(0, L, 400):
        a, _, c = fe.push([wav[3, lo:lo + 400], loud[lo:lo + 400], wav[0, lo:lo + 400]])
        out[0].append(a), out[2].append(c)
    assert fe.max_db_seen(1) > DEFAULT.min_db + TOP_DB > max(fe.max_db_seen(0), fe.max_db_seen(2))
    fe.verify([0, 2])
    with pytest.raises(PwvError, match='top_db'):
        fe.verify()
    with pytest.raises(PwvError, match='top_db'):
        fe.finish(1)
    out[0].append(fe.finish(0)), out[2].append(fe.finish(2))
    assert torch.equal(torch.cat(out[0]), want[3]) and torch.equal(torch.cat(out[2]), want[0])
    fe.verify()                                                                  # (the loud slot is fresh again)


def test_inside_guarded_buffers(gpu):
    """One pass with the results and the state blocks inside poisoned, guard-banded buffers (tests/guarded.py): every row of a result
    was written (no NaN left), nothing was written beside a result, the carries or the maximum words."""
    from pwv_amd import audio_frontend as A
    from tests.guarded import guarded
    L = 100
    wav, want = _case(SMALL, L, gpu)
    with guarded(A) as g:
        fe = A.StreamingMel(4, signal=SMALL)
        assert g.holds(fe._state) and g.holds(fe._max)
        got, pos = [[] for _ in range(4)], 0
        for n in _chunkings(SMALL, L)['edges']:
            pieces = fe.push([wav[i, pos:pos + n] for i in range(4)])
            assert all(g.holds(p) for p in pieces if p.shape[0])
            for i, p in enumerate(pieces):
                got[i].append(p)
            pos += n
        for i in range(4):
            got[i].append(fe.finish(i))
            assert g.holds(got[i][-1])
        torch.cuda.synchronize()
        for i in range(4):
            full = torch.cat(got[i])
            assert not bool(torch.isnan(full).any()) and torch.equal(full, want[i])
        assert not bool(torch.isnan(fe._state).any())
        g.check()
    wav, want = _case(DEFAULT, 1000, gpu)
    with guarded(A) as g:
        fe = A.StreamingMel(4, signal=DEFAULT)
        got, _ = _stream_all(fe, wav, _chunkings(DEFAULT, 1000)['edges'])
        torch.cuda.synchronize()
        assert all(not bool(torch.isnan(got[i]).any()) and torch.equal(got[i], want[i]) for i in range(4))
        g.check()


def test_wav_chunks_in_wav_chunks_out(gpu):
    """End to end: wav -> StreamingMel -> StreamingVocoder.push_varlen, concatenated, is the one-shot pair wav_to_mel_device ->
    generate_varlen on the same seed, bit for bit."""
    from pwv_amd import audio_frontend as A
    from tests.test_gpu_stream import _model
    from tests.util import small_cfg
    model, _ = _model(gpu, small_cfg())
    seed, L = 1234, 1040
    wav = torch.from_numpy(_signals()[0, :L].copy()).to(gpu)
    want = model.generate_varlen([A.wav_to_mel_device(wav[None])[0]], seeds=[seed])[0]
    fe, s = A.StreamingMel(1), model.open_stream(slots=1)
    out, fresh = [], True
    for lo in range(0, L, 200):
        frames = fe.push([wav[lo:lo + 200]])[0]
        if lo + 200 >= L:
            frames = torch.cat([frames, fe.finish(0)])
        if frames.shape[0]:                      # (the first 200 samples bring no frame: the session sits that tick out)
            out.append(s.push_varlen([frames], seeds=[seed] if fresh else None)[0])
            fresh = False
    got = torch.cat(out)
    assert got.shape == want.shape == (L, 1) and torch.equal(got, want)


def test_generate_stream_live_writes_what_varlen_writes(gpu, tmp_path, monkeypatch):
    """generate CASE --stream=5 --live on three short wavs: the files and sample counts of --varlen."""
    from scipy.io import wavfile
    from pwv_amd.generate import generate
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
    counts = {}
    for key, kw in (('varlen', dict(varlen=True)), ('live', dict(stream=5, live=True))):
        logdir = tmp_path / key
        monkeypatch.setenv('PWV_LOGDIR', str(logdir))
        pred = generate('default', **kw)
        assert len(pred) == 3 and all(np.isfinite(p).all() for p in pred)
        counts[key] = [wavfile.read(str(logdir / ('pred_%d.wav' % i)))[1].shape[0] for i in range(3)]
        assert counts[key] == [len(p) for p in pred] and (logdir / 'pred_wav_varlen.npz').exists()
    assert counts['live'] == counts['varlen'] and len(set(counts['varlen'])) == 3 and all(c % 80 == 0 and c > 400 for c in counts['varlen'])
