"""CPU: scoring (pwv_amd/score.py, include/pwv_hip_score.h, csrc/pwv_score.hip) -- the numpy restatement against a closed form and
against torch.stft, the frame arithmetic, the aggregation of a Scores, the C ABI addition with its refusals, and the kernels' resources.
No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cosine(dtype, A=0.25, k=5, L=160, phase=0.3):
    return (A * np.cos(2 * np.pi * k * np.arange(L) / 64 + phase)).astype(dtype)


CLOSED_FORM = ((16 * 0.25) ** 4 + 2 * (8 * 0.25) ** 4) / 33          # = 8.7272...


@pytest.mark.parametrize('dtype,tol', [(np.float64, 1e-12), (np.float32, 1e-6)])
def test_restatement_against_the_closed_form(dtype, tol):
    """win = fft_length = 64, hop 16, out = A cos(2 pi k t / 64 + phi), y = 0: under the periodic Hann window every frame has
    P[k] = (A 64 / 4)^2 and P[k +- 1] = (A 64 / 8)^2 and nothing else, so power = ((16 A)^4 + 2 (8 A)^4) / 33 -- whatever the phase."""
    from pwv_amd.score import Scores, score_reference
    x = _cosine(dtype)
    t = score_reference([x], [np.zeros_like(x)], 64, 16)
    assert t.shape == (1, 4) and t[0, 1] == 160 and t[0, 3] == 7 * 33
    assert abs(CLOSED_FORM - 8.727272727272727) < 1e-14
    assert abs(t[0, 2] / t[0, 3] - CLOSED_FORM) <= tol * CLOSED_FORM, (t[0, 2] / t[0, 3], CLOSED_FORM)
    assert abs(Scores(t, 64).power[0] - CLOSED_FORM) <= tol * CLOSED_FORM
    assert abs(t[0, 0] - np.abs(x.astype(np.float64)).sum()) <= 1e-12 * t[0, 0]


@pytest.mark.parametrize('win,hop,L', [(400, 80, 1200), (64, 16, 160), (100, 20, 300)])
def test_restatement_against_torch_stft(win, hop, L):
    """torch.stft(center=False, periodic Hann of win_length) on the signal zero-padded by (fft_length - win) // 2 in front and the rest
    behind places its window in the middle of fft_length: the same samples under the same weights as TF's frame padded behind, hence the
    same power frames.  (100, 20, 300) has fft_length 128."""
    import torch
    from pwv_amd.score import fft_length, frame_count, power_frames
    rng = np.random.default_rng(win)
    x = 0.5 * rng.standard_normal(L)
    nfft = fft_length(win)
    assert nfft == {400: 512, 64: 64, 100: 128}[win]
    front = (nfft - win) // 2
    padded = torch.from_numpy(np.concatenate([np.zeros(front), x, np.zeros(nfft - win - front)]))
    spec = torch.stft(padded, n_fft=nfft, hop_length=hop, win_length=win, window=torch.hann_window(win, periodic=True, dtype=torch.float64),
                      center=False, return_complex=True)
    want = (spec.real ** 2 + spec.imag ** 2).numpy().T
    got = power_frames(x, win, hop)
    assert got.shape == want.shape == (frame_count(L, win, hop), nfft // 2 + 1)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_frame_arithmetic():
    """L = 399 -> no frame (power NaN, l1 defined); 400 -> 1; 479 -> 1; 480 -> 2."""
    from pwv_amd.score import Scores, frame_count, score_reference
    rng = np.random.default_rng(0)
    for L, frames in ((399, 0), (400, 1), (479, 1), (480, 2)):
        a, b = rng.standard_normal(L).astype(np.float32), rng.standard_normal(L).astype(np.float32)
        t = score_reference([a], [b], 400, 80)
        s = Scores(t, 400)
        assert frame_count(L, 400, 80) == frames and t[0, 3] == frames * 257 and s.frames[0] == frames and s.samples[0] == L
        assert np.isfinite(s.l1[0]) and abs(s.l1[0] - np.abs(a.astype(np.float64) - b).mean()) < 1e-12
        assert np.isnan(s.power[0]) == (frames == 0)
        assert np.isnan(s.power_loss) == (frames == 0) and np.isfinite(s.likelihood)
    assert frame_count(1000, 0, 80) == 0


def test_scores_aggregation_weights_by_counts():
    """A hand-written table: the batch means are ratios of column sums (an utterance counts by its samples and its terms, not once),
    and an utterance with terms = 0 is left out of power_loss and not out of likelihood."""
    from pwv_amd.score import Scores
    table = np.array([[10.0, 100, 66.0, 2 * 33],
                      [90.0, 300, 0.0, 0],
                      [5.0, 50, 33.0 * 7, 5 * 33]])
    s = Scores(table, 64)
    assert np.allclose(s.l1, [0.1, 0.3, 0.1], rtol=0, atol=1e-15)
    assert s.power[0] == 1.0 and np.isnan(s.power[1]) and s.power[2] == 7 / 5
    assert list(s.frames) == [2, 0, 5] and list(s.samples) == [100, 300, 50]
    assert s.likelihood == 105.0 / 450 and s.likelihood != np.mean(s.l1)
    assert s.power_loss == (66.0 + 231.0) / (7 * 33) and s.power_loss != np.nanmean(s.power)
    assert s.total(2.0) == s.likelihood + 2.0 * s.power_loss and s.total(0.0) == s.likelihood
    from pwv_amd.hparam import hparam as hp
    hp.set_hparam_yaml('default')
    assert s.total() == s.likelihood + float(hp.train.weight_power_loss) * s.power_loss
    l1_only = Scores(table[:, [0, 1, 1, 1]] * [1, 1, 0, 0], 0)
    assert np.isnan(l1_only.power_loss) and list(l1_only.frames) == [0, 0, 0] and l1_only.likelihood == s.likelihood


def test_score_varlen_names_the_utterance_whose_lengths_differ():
    """A prediction and a ground truth of different lengths: the ValueError names the utterance -- checked before anything is asked of a
    device, so plain CPU tensors show it; so are the settings."""
    import torch
    from pwv_amd import score as S
    with pytest.raises(ValueError, match='utterance 1'):
        S.score_varlen([torch.zeros(5, 1), torch.zeros(6, 1)], [torch.zeros(5, 1), torch.zeros(7, 1)], 400, 80)
    with pytest.raises(ValueError, match='2 predictions for 1'):
        S.score_varlen([torch.zeros(5, 1), torch.zeros(6, 1)], [torch.zeros(5, 1)], 400, 80)
    with pytest.raises(ValueError, match='utterance 1'):
        S.score_reference([np.zeros(5), np.zeros(6)], [np.zeros(5), np.zeros(7)], 0, 1)
    with pytest.raises(ValueError, match='win_length'):
        S.score(torch.zeros(1, 8), torch.zeros(1, 8), win_length=2048, hop_length=80)
    with pytest.raises(ValueError, match='hop_length'):
        S.score(torch.zeros(1, 8), torch.zeros(1, 8), win_length=64, hop_length=0)


def test_score_args_layout_matches_ctypes(tmp_path):
    """The C compiler's size and offsets of pwv_score_args (gcc -std=c99 -pedantic -Werror on include/pwv_hip_score.h) against the ctypes
    mirror; the header declares exactly _lib.SCORE_SYMBOLS, which are disjoint from the three older lists -- unchanged -- and exported by the
    built library; pwv_hip.h keeps its version."""
    import subprocess
    from pwv_amd import _lib
    _lib.build_library()
    fields = [n for n, _ in _lib.ScoreArgs._fields_]
    assert fields == ['struct_size', 'out', 'y', 'cu_rows', 'n', 'T', 'rows', 'win_length', 'hop_length', 'result', 'workspace', 'workspace_bytes']
    probe = (['sizeof(pwv_score_args)'] + ['offsetof(pwv_score_args, %s)' % f for f in fields]
             + ['(size_t)PWV_SCORE_MAX_WIN', '(size_t)PWV_SCORE_TILE', '(size_t)PWV_HIP_VERSION'])
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "pwv_hip_score.h"\nint main(void){ printf("%s\\n", %s); return 0; }\n'
           % (' '.join(['%zu'] * len(probe)), ', '.join(probe)))
    c, exe = str(tmp_path / 't.c'), str(tmp_path / 't')
    with open(c, 'w') as f:
        f.write(src)
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Wextra', '-pedantic', '-Werror', '-I' + os.path.join(ROOT, 'include'), c, '-o', exe])
    got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    want = ([ctypes.sizeof(_lib.ScoreArgs)] + [getattr(_lib.ScoreArgs, f).offset for f in fields]
            + [_lib.SCORE_MAX_WIN, _lib.SCORE_TILE, _lib.HEADER_VERSION])
    assert got == want and _lib.HEADER_VERSION == 301 and _lib.SCORE_MAX_WIN >= 1024
    assert _lib.ScoreArgs().struct_size == ctypes.sizeof(_lib.ScoreArgs)
    text = open(os.path.join(ROOT, 'include', 'pwv_hip_score.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    assert '#include "pwv_hip.h"' in code
    assert sorted(set(re.findall(r'\b(pwv_[a-z0-9_]+)\s*\(', code))) == sorted(_lib.SCORE_SYMBOLS) == ['pwv_score_f32', 'pwv_score_workspace_bytes']
    assert not set(_lib.SCORE_SYMBOLS) & (set(_lib.EXPORTED_SYMBOLS) | set(_lib.EXTENSION_SYMBOLS) | set(_lib.LIVE_TICK_SYMBOLS))
    assert len(_lib.EXPORTED_SYMBOLS) == 52 and _lib.EXTENSION_SYMBOLS == ('pwv_wav_to_mel_db_stream_f32',)
    assert _lib.LIVE_TICK_SYMBOLS == ('pwv_live_tick_mel', 'pwv_live_tick_commit')
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(raw, name) for name in _lib.SCORE_SYMBOLS)
    assert os.path.join(os.path.dirname(_lib.__file__), 'csrc', 'pwv_score.hip') in _lib.CSRC


def _args(n=3, rows=2400, T=800, win=400, hop=80, packed=False):
    """A pwv_score_args the library accepts up to its launch: every device pointer a number that is never dereferenced on the host."""
    from pwv_amd import _lib
    a = _lib.ScoreArgs()
    a.out = a.y = a.result = a.workspace = 4096
    a.cu_rows = 4096 if packed else None
    a.n, a.T, a.rows, a.win_length, a.hop_length = n, T, rows, win, hop
    a.workspace_bytes = 1 << 30
    return a


def test_score_workspace_bytes_follow_the_slot_layout(built_lib):
    """rows / hop + n frame slots (none in the L1-only mode) and rows / TILE + n tile slots of one double each; 0 for a refused call."""
    from pwv_amd import _lib
    for n, rows, win, hop in ((3, 2400, 400, 80), (1, 80, 400, 80), (5, 4080, 64, 16), (2, 1760, 0, 1), (8, 64000, 400, 80)):
        a = _args(n=n, rows=rows, T=rows // n, win=win, hop=hop)
        want = 8 * ((rows // hop + n if win else 0) + rows // _lib.SCORE_TILE + n)
        assert built_lib.pwv_score_workspace_bytes(ctypes.byref(a)) == want
        a.cu_rows = 4096
        assert built_lib.pwv_score_workspace_bytes(ctypes.byref(a)) == want
    assert built_lib.pwv_score_workspace_bytes(None) == 0
    assert built_lib.pwv_score_workspace_bytes(ctypes.byref(_args(hop=0))) == 0 and b'hop_length' in built_lib.pwv_last_error()


@pytest.mark.parametrize('packed', [False, True], ids=['uniform', 'packed'])
def test_score_refusals_no_gpu(built_lib, packed):
    """Every refusal of pwv_score_f32 returns -1 (PWV_EINVAL) with its field named, before anything touches a device (this process has
    none)."""
    def refused(a, word):
        code = built_lib.pwv_score_f32(ctypes.byref(a), None)
        msg = built_lib.pwv_last_error()
        assert code == -1 and word in msg and b'pwv_score_f32' in msg, (code, word, msg)

    assert built_lib.pwv_score_f32(None, None) == -1 and b'NULL' in built_lib.pwv_last_error()
    a = _args(packed=packed)
    a.struct_size = 0
    refused(a, b'struct_size')
    a.struct_size = ctypes.sizeof(a) - 4
    refused(a, b'struct_size')
    for n in (0, -1):
        refused(_args(n=n, packed=packed), b': n ')
    for hop in (0, -80):
        refused(_args(hop=hop, packed=packed), b'hop_length')
    from pwv_amd import _lib
    for win in (_lib.SCORE_MAX_WIN + 1, 4096, -1):
        refused(_args(win=win, packed=packed), b'win_length')
    for field in ('out', 'y', 'result', 'workspace'):
        a = _args(packed=packed)
        setattr(a, field, None)
        refused(a, b'NULL pointer')
        refused(a, field.encode())
    a = _args(packed=packed)
    a.workspace_bytes = built_lib.pwv_score_workspace_bytes(ctypes.byref(a)) - 1
    refused(a, b'workspace_bytes')
    a.workspace_bytes = 0
    refused(a, b'workspace_bytes')
    for rows in (-1, 1 << 31):
        refused(_args(rows=rows, packed=packed), b'rows')
    if not packed:
        refused(_args(n=3, T=801, rows=2400), b': T ')          # n T leaves rows
        refused(_args(T=-1), b': T ')
    # the largest window the header admits is accepted up to the launch: only the sizes are checked here
    assert built_lib.pwv_score_workspace_bytes(ctypes.byref(_args(win=_lib.SCORE_MAX_WIN, packed=packed))) > 0


def test_score_kernels_use_no_scratch():
    """The compiler's resource remarks (gfx950 device code) for every kernel of csrc/pwv_score.hip: no scratch, no spilled register."""
    from tests.util import kernel_resources
    res = kernel_resources('pwv_score.hip')
    assert len(res) == 2 and all('score_' in n for n in res), sorted(res)
    for name, r in res.items():
        assert r['scratch'] == 0 and r['vgpr_spills'] == 0 and r['sgpr_spills'] == 0 and not r['dynamic_stack'], (name, r)
