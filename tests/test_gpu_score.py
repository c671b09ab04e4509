"""GPU: scoring on the device (pwv_amd/score.py -> pwv_score_f32, csrc/pwv_score.hip) against its numpy float64 restatement
(score.score_reference): parity, a closed form, identity, batch independence, lengths read on the device under graph replay, the L1-only
mode, guarded buffers and `generate --score`.

The parity bar, 1e-10 relative on abs_sum and power_sum, is derived and not tuned: a float64 direct DFT with table twiddles differs from
rfft by 1.4 - 2.7e-16 on these inputs, an fp32 evaluation by 1.5 - 2.2e-7; 1e-10 leaves six orders of magnitude for the summation
order and the device's sincospi and still fails if any fp32 step crept in.  Inputs: seeded 0.5 N(0, 1) float32, prediction and ground
truth drawn independently."""
import functools
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REL = 1e-10
# what one pass of the second kernel takes: a workgroup of 256 threads adds an utterance's partials t, t + 256, ... per thread, so an
# utterance of more than 256 frames (or 256 tiles of 1024 samples) is the first whose threads add more than one partial
REDUCE_STRIDE = 256
TILE = 1024


@functools.lru_cache(maxsize=None)
def _pair(n, length, seed):
    """(pred, gt) float32 [n, length], shared between the tests, never written to."""
    rng = np.random.default_rng(seed)
    a, b = (0.5 * rng.standard_normal((n, length))).astype(np.float32), (0.5 * rng.standard_normal((n, length))).astype(np.float32)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def _frames_len(frames, win, hop, extra=0):
    return win + hop * (frames - 1) + extra


# (id, utterances, samples, win, hop)
UNIFORM_CASES = ([('batch3x800', 3, 800, 400, 80)]
                 + [('single%d' % L, 1, L, 400, 80) for L in (80, 399, 400, 479, 480, 1200)]
                 + [('win64', 2, 304, 64, 16), ('win100_fft128', 2, 304, 100, 20)]
                 + [('frames%d' % f, 1, _frames_len(f, 64, 16, 5), 64, 16) for f in (REDUCE_STRIDE - 1, REDUCE_STRIDE, REDUCE_STRIDE + 1)]
                 + [('tile%d' % L, 2, L, 400, 80) for L in (TILE - 1, TILE, TILE + 1)]
                 + [('tiles%d' % REDUCE_STRIDE, 1, REDUCE_STRIDE * TILE + 1, 0, 80)])
PACKED_LENGTHS = (80, 400, 560, 1040, 2000)


def _assert_table(got, want, what=''):
    got = got.cpu().numpy() if hasattr(got, 'cpu') else np.asarray(got)
    assert got.shape == want.shape and got.dtype == np.float64, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), (what, got)
    assert np.array_equal(got[:, 1], want[:, 1]) and np.array_equal(got[:, 3], want[:, 3]), (what, got, want)          # the counts: exact
    for col in (0, 2):
        err = np.abs(got[:, col] - want[:, col])
        print(what, 'column', col, 'max relative error', float((err / np.maximum(np.abs(want[:, col]), 1e-300)).max()))
        assert (err <= REL * np.abs(want[:, col])).all(), (what, col, got[:, col], want[:, col])


def _uniform_case(gpu, case):
    import torch
    from pwv_amd import score as S
    name, n, length, win, hop = case
    a, b = _pair(n, length, 11)
    s = S.score(torch.tensor(a).to(gpu)[:, :, None], torch.tensor(b).to(gpu), win, hop)
    return s, S.score_reference(a, b, win, hop)


@pytest.mark.parametrize('case', UNIFORM_CASES, ids=[c[0] for c in UNIFORM_CASES])
def test_score_matches_the_restatement(gpu, case):
    """Uniform batches: the batch of three, single utterances around the one- and two-frame lengths (80 and 399 have no frame), the two
    smaller windows (100 has fft_length 128), frame counts and tile counts one below, at and one above REDUCE_STRIDE partials of one
    utterance, lengths around one tile."""
    from pwv_amd.score import frame_count
    s, want = _uniform_case(gpu, case)
    _assert_table(s.table, want, case[0])
    assert list(s.frames) == [frame_count(case[2], case[3], case[4])] * case[1] and list(s.samples) == [case[2]] * case[1]
    if case[0].startswith('frames'):
        assert s.frames[0] == int(case[0][6:])
    if case[3] == 0:
        assert np.isnan(s.power_loss) and want[0, 3] == 0


def _packed_case(gpu):
    import torch
    from pwv_amd import score as S
    a, b = _pair(1, sum(PACKED_LENGTHS), 12)
    cu = np.concatenate([[0], np.cumsum(PACKED_LENGTHS)])
    pa, pb = ([torch.from_numpy(v[0, lo:hi].copy()).to(gpu)[:, None] for lo, hi in zip(cu, cu[1:])] for v in (a, b))
    want = S.score_reference([a[0, lo:hi] for lo, hi in zip(cu, cu[1:])], [b[0, lo:hi] for lo, hi in zip(cu, cu[1:])], 400, 80)
    return pa, pb, want


def test_score_varlen_matches_the_restatement(gpu):
    """The packed batch (80: no frame; 400: one; 560: three; ...), as a list and as an output object whose .packed is scored in place."""
    import torch
    from pwv_amd import score as S
    from pwv_amd.stream import RaggedOutput
    pa, pb, want = _packed_case(gpu)
    s = S.score_varlen(pa, pb, 400, 80)
    _assert_table(s.table, want, 'packed')
    assert list(s.frames) == [0, 1, 3, 9, 21] and np.isnan(s.power[0]) and np.isfinite(s.l1).all()
    whole_a, whole_b = RaggedOutput(torch.cat(pa), PACKED_LENGTHS), RaggedOutput(torch.cat(pb), PACKED_LENGTHS)
    assert torch.equal(S.score_varlen(whole_a, whole_b, 400, 80).table, s.table)
    assert abs(s.likelihood - want[:, 0].sum() / want[:, 1].sum()) <= REL * s.likelihood
    assert abs(s.power_loss - want[:, 2].sum() / want[:, 3].sum()) <= REL * s.power_loss
    assert abs(s.total(0.5) - (s.likelihood + 0.5 * s.power_loss)) <= 1e-15 * s.total(0.5)
    with pytest.raises(ValueError, match='utterance 2'):
        S.score_varlen(pa, pb[:2] + [pb[2][:-1]] + pb[3:], 400, 80)


def _closed_form(gpu):
    import torch
    from pwv_amd import score as S
    x = (0.25 * np.cos(2 * np.pi * 5 * np.arange(160) / 64 + 0.3)).astype(np.float32)
    return S.score(torch.from_numpy(x[None]).to(gpu), torch.zeros((1, 160), device=gpu), 64, 16)


def test_closed_form_on_the_device(gpu):
    """out = 0.25 cos(2 pi 5 t / 64 + phi), y = 0, win = fft_length = 64, hop 16, L = 160: power = ((16 A)^4 + 2 (8 A)^4) / 33 = 8.7272...
    to 1e-6, the float32 input's rounding."""
    s = _closed_form(gpu)
    want = ((16 * 0.25) ** 4 + 2 * (8 * 0.25) ** 4) / 33
    print('closed form', s.power[0], want)
    assert s.frames[0] == 7 and abs(s.power[0] - want) <= 1e-6 * want and abs(s.power_loss - want) <= 1e-6 * want


def test_identity_scores_exact_zeros(gpu):
    """score(x, x): abs_sum == 0.0 and power_sum == 0.0 exactly (both spectra are the same arithmetic on the same values)."""
    import torch
    from pwv_amd import score as S
    x = torch.tensor(_pair(3, 800, 11)[0]).to(gpu)
    t = S.score(x, x.clone(), 400, 80).table.cpu().numpy()
    assert np.array_equal(t[:, 0], np.zeros(3)) and np.array_equal(t[:, 2], np.zeros(3))
    assert np.array_equal(t[:, 1], [800] * 3) and np.array_equal(t[:, 3], [6 * 257] * 3)


def test_a_row_does_not_depend_on_the_batch(gpu):
    """Every row of the packed batch is the same bits as its utterance scored alone and as the utterance inside a uniform batch (between
    two others), and two runs agree bit for bit."""
    import torch
    from pwv_amd import score as S
    pa, pb, want = _packed_case(gpu)
    first = S.score_varlen(pa, pb, 400, 80).table
    again = S.score_varlen(pa, pb, 400, 80).table
    assert torch.equal(first, again)
    g = torch.Generator(device='cpu').manual_seed(5)
    for i, (a, b) in enumerate(zip(pa, pb)):
        alone = S.score(a[None], b[None], 400, 80).table
        assert torch.equal(alone[0], first[i]), (i, alone, first[i])
        others = (0.5 * torch.randn((2, 2, a.shape[0]), generator=g)).to(gpu)
        batch_a = torch.stack([others[0, 0], a[:, 0], others[0, 1]])
        batch_b = torch.stack([others[1, 0], b[:, 0], others[1, 1]])
        inside = S.score(batch_a, batch_b, 400, 80).table
        assert torch.equal(inside[1], first[i]), (i, inside, first[i])
    assert torch.equal(S.score_varlen(pa[::-1], pb[::-1], 400, 80).table, first.flip(0))


def _graph_case(gpu):
    """score_varlen captured at 4 utterances / 4000 rows (one stream, no parallel branches) and replayed for two length sets written into
    the same cu_rows tensor: [(replayed table, eager table of the same utterances, reference)], and the graph (kept alive)."""
    import torch
    from pwv_amd import score as S
    a, b = _pair(1, 4000, 13)
    pred, gt = torch.from_numpy(a[0].copy()).to(gpu)[:, None], torch.from_numpy(b[0].copy()).to(gpu)[:, None]
    cu = torch.zeros((5,), dtype=torch.int32, device=gpu)
    sets = ([1200, 80, 1520, 1200], [400, 2000, 399, 0])
    cu.copy_(torch.tensor(np.concatenate([[0], np.cumsum(sets[0])]), dtype=torch.int32))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        S.score_varlen(pred, gt, 400, 80, cu_rows=cu)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured = S.score_varlen(pred, gt, 400, 80, cu_rows=cu)
    out = []
    for lengths in sets:
        bounds = np.concatenate([[0], np.cumsum(lengths)])
        cu.copy_(torch.tensor(bounds, dtype=torch.int32))
        graph.replay()
        replayed = captured.table.clone()
        pieces = [(pred[lo:hi], gt[lo:hi]) for lo, hi in zip(bounds, bounds[1:])]
        eager = S.score_varlen([p for p, _ in pieces], [q for _, q in pieces], 400, 80).table
        want = S.score_reference([a[0, lo:hi] for lo, hi in zip(bounds, bounds[1:])], [b[0, lo:hi] for lo, hi in zip(bounds, bounds[1:])], 400, 80)
        out.append((replayed, eager, want))
    return out, graph


def test_lengths_are_read_on_the_device_under_graph_replay(gpu):
    """One capture, two length sets (the second does not fill the capacity and holds an empty utterance): each replay equals the eager
    call on the same utterances, bit for bit, and the restatement."""
    import torch
    runs, graph = _graph_case(gpu)
    for replayed, eager, want in runs:
        assert torch.equal(replayed, eager)
        _assert_table(replayed, want, 'replay')
    assert not torch.equal(runs[0][0], runs[1][0])


def _mel_case(gpu):
    import torch
    from pwv_amd import score as S
    rng = np.random.default_rng(14)
    a, b = rng.uniform(-1, 1, (2, 11, 80)).astype(np.float32), rng.uniform(-1, 1, (2, 11, 80)).astype(np.float32)
    ta, tb = torch.from_numpy(a).to(gpu), torch.from_numpy(b).to(gpu)
    return S.mel_l1(ta, tb), S.mel_l1([ta[0], ta[1, :7]], [tb[0], tb[1, :7]]), a, b


def test_l1_only_mode(gpu):
    """mel_l1 on [2, 11, 80] equals the numpy mean of the downloaded mels to 1e-10 (uniform and as a list of different frame counts);
    win_length = 0 leaves columns 2 and 3 zero."""
    import torch
    from pwv_amd import score as S
    s, ragged, a, b = _mel_case(gpu)
    want = np.abs(a.astype(np.float64) - b.astype(np.float64)).mean(axis=(1, 2))
    assert np.abs(s.l1 - want).max() <= 1e-10 * want.max()
    t = s.table.cpu().numpy()
    assert np.array_equal(t[:, 2:], np.zeros((2, 2))) and np.array_equal(t[:, 1], [880, 880])
    assert abs(s.likelihood - np.abs(a.astype(np.float64) - b).mean()) <= 1e-10
    want7 = np.abs(a[1, :7].astype(np.float64) - b[1, :7]).mean()
    assert abs(ragged.l1[1] - want7) <= 1e-10 * want7 and ragged.l1[0] == s.l1[0] and list(ragged.samples) == [880, 560]
    x, y = _pair(3, 800, 11)
    t0 = S.score(torch.tensor(x).to(gpu), torch.tensor(y).to(gpu), 0, 80).table.cpu().numpy()
    assert np.array_equal(t0[:, 2:], np.zeros((3, 2)))
    _assert_table(t0, S.score_reference(x, y, 0, 80), 'win0')


def test_every_call_inside_guarded_buffers(gpu):
    """Every call of the tests above once more with the module's allocations -- tables, workspaces, packed copies -- inside poisoned,
    guard-banded buffers: the same parity, no NaN in any table (a slot that was never written but read would bring one), clean bands."""
    import torch
    from pwv_amd import score as S
    from tests.guarded import guarded
    with guarded(S) as g:
        tables = []
        for case in UNIFORM_CASES:
            s, want = _uniform_case(gpu, case)
            assert g.holds(s.table)
            _assert_table(s.table, want, 'guarded ' + case[0])
            tables.append(s.table)
        pa, pb, want = _packed_case(gpu)
        s = S.score_varlen(pa, pb, 400, 80)
        assert g.holds(s.table)
        _assert_table(s.table, want, 'guarded packed')
        tables += [s.table, _closed_form(gpu).table]
        x = torch.tensor(_pair(3, 800, 11)[0]).to(gpu)
        ident = S.score(x, x.clone(), 400, 80).table
        assert float(ident[:, 0].abs().sum()) == 0.0 and float(ident[:, 2].abs().sum()) == 0.0
        runs, graph = _graph_case(gpu)
        for replayed, eager, want in runs:
            assert torch.equal(replayed, eager)
            _assert_table(replayed, want, 'guarded replay')
        m, ragged, a, b = _mel_case(gpu)
        tables += [ident, m.table, ragged.table]
        torch.cuda.synchronize()
        for t in tables:
            assert not bool(torch.isnan(t).any())
        assert len(g.allocations) >= 2 * len(UNIFORM_CASES)
        g.check()
        del graph


def _patched_hparams(monkeypatch, pattern, length=None):
    from pwv_amd.hparam import hparam as hp
    orig = type(hp).set_hparam_yaml

    def patched(self, case, *a, **k):          # what a user's hparams.yaml case would override
        r = orig(self, case, *a, **k)
        self.data_path = pattern
        self.train.dataset_ratio, self.generate.batch_size = 0.0, 3
        self.model.n_iaf, self.model.dilations = 1, [[1, 2, 4, 8]]
        if length is not None:
            self.generate.length = length
        return r

    monkeypatch.setattr(type(hp), 'set_hparam_yaml', patched)
    return hp


SCORE_KEYS = {'loss/likelihood', 'loss/power', 'loss/total', 'weight_power_loss', 'inputs'}
INPUT_KEYS = {'file', 'samples', 'l1', 'frames', 'power', 'mel_l1'}


def _close(got, want):
    return got is not None and abs(got - want) <= REL * abs(want)


def test_generate_cli_score_on_wavs(gpu, tmp_path, monkeypatch):
    """`generate default --score`, `--varlen --score`, `--stream=5 --score` and `--stream=5 --live --score` on three short wavs of
    different lengths, a one-flow model: scores.json holds the batch numbers under the reference's names and per input file, samples, l1,
    frames, power and mel_l1; its numbers equal score_reference on the returned predictions and the ground truth as the mode loads it
    (the three packed modes keep the trimmed wav, cut to whole hops), to 1e-10."""
    from scipy.io import wavfile
    from pwv_amd import audio_frontend as A
    from pwv_amd import score as S
    from pwv_amd.generate import _fire, generate
    sr = 16000
    files = []
    for i, n in enumerate((2400, 1700, 3300)):
        t = np.arange(n + 1500) / sr
        wav = 0.3 * np.sin(2 * np.pi * (200 + 40 * i) * t) * (t > 0.05)
        files.append(str(tmp_path / ('a%02d.wav' % i)))
        wavfile.write(files[-1], sr, (wav * 32767).astype(np.int16))
    hp = _patched_hparams(monkeypatch, str(tmp_path / '*.wav'), length=2400)
    for mode, argv in (('plain', ['default', '--score']), ('varlen', ['default', '--varlen', '--score']),
                       ('stream', ['default', '--stream=5', '--score']), ('live', ['default', '--stream=5', '--live', '--score'])):
        logdir = tmp_path / mode
        monkeypatch.setenv('PWV_LOGDIR', str(logdir))
        pred = _fire(generate, argv)
        got = json.loads((logdir / 'scores.json').read_text())
        assert SCORE_KEYS <= set(got) and len(got['inputs']) == 3 and all(set(e) == INPUT_KEYS for e in got['inputs'])
        if mode == 'plain':
            gts = [A.load_wav_fixed(f, 2400) for f in files]
        else:
            gts = [A.trim_wav(A.read_wav(f, sr)) for f in files]
            gts = [w[:len(w) // 80 * 80].astype(np.float32) for w in gts]
            assert len(set(len(w) for w in gts)) == 3
        preds = [np.asarray(p, dtype=np.float32).reshape(-1) for p in pred]
        want = S.score_reference(preds, gts, int(hp.signal.win_length), int(hp.signal.hop_length))
        ref = S.Scores(want, int(hp.signal.win_length))
        for i, e in enumerate(got['inputs']):
            assert e['file'] == files[i] and e['samples'] == len(gts[i]) and e['frames'] == ref.frames[i] > 0
            assert _close(e['l1'], ref.l1[i]) and _close(e['power'], ref.power[i]), (mode, i, e, ref.l1[i], ref.power[i])
            assert e['mel_l1'] is not None and np.isfinite(e['mel_l1']) and 0 <= e['mel_l1'] <= 2
        assert got['weight_power_loss'] == float(hp.train.weight_power_loss)
        assert _close(got['loss/likelihood'], ref.likelihood) and _close(got['loss/power'], ref.power_loss)
        assert _close(got['loss/total'], ref.total(got['weight_power_loss']))


def test_generate_cli_score_on_npy_mels(gpu, tmp_path, monkeypatch):
    """With .npy mels there is no ground-truth wav: l1 and power (and the batch numbers) are null, mel_l1 is finite; without --score no
    scores.json is written."""
    from pwv_amd.generate import _fire, generate
    rng = np.random.default_rng(4)
    frames = [6, 21, 9]
    for i, f in enumerate(frames):
        np.save(str(tmp_path / ('m%d.npy' % i)), rng.uniform(-1, 1, (f, 80)).astype(np.float32))
    _patched_hparams(monkeypatch, str(tmp_path / '*.npy'))
    monkeypatch.setenv('PWV_LOGDIR', str(tmp_path / 'plain'))
    pred = _fire(generate, ['default', '--varlen'])
    assert len(pred) == 3 and (tmp_path / 'plain' / 'pred_0.wav').exists() and not (tmp_path / 'plain' / 'scores.json').exists()
    monkeypatch.setenv('PWV_LOGDIR', str(tmp_path / 'scored'))
    pred = _fire(generate, ['default', '--varlen', '--score'])
    got = json.loads((tmp_path / 'scored' / 'scores.json').read_text())
    assert SCORE_KEYS <= set(got) and [e['samples'] for e in got['inputs']] == [(f - 1) * 80 for f in frames]
    assert got['loss/likelihood'] is None and got['loss/power'] is None and got['loss/total'] is None
    for e in got['inputs']:
        assert set(e) == INPUT_KEYS and e['l1'] is None and e['power'] is None and e['frames'] == 0
        assert e['mel_l1'] is not None and np.isfinite(e['mel_l1']) and e['mel_l1'] > 0
