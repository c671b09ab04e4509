"""CPU: the host side of the streaming mel front-end (audio_frontend.StreamingMel, pwv_mel_stream_args) -- the ready / finish / carry
arithmetic against a direct evaluation of what the frames read, the C ABI addition and its refusals, the top_db headroom of the default
hparams, and the compiler's resource remarks for the new kernel.  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N_FFTS = (8, 32, 512)
HOPS = (1, 3, 8, 80)


def _reads(k, n_fft, hop, L=None):
    """The sample indices frame k reads, as stft_mel_kernel computes them (csrc/pwv_audio.hip): t = k hop - h .. k hop + h - 1, t < 0 at
    -t, and with a final length L: t >= L at 2 (L - 1) - t, clamped."""
    t = k * hop - n_fft // 2 + np.arange(n_fft)
    t = np.where(t < 0, -t, t)
    if L is not None:
        t = np.where(t >= L, 2 * (L - 1) - t, t)
        t = np.clip(t, 0, L - 1)
    return t


@pytest.mark.parametrize('n_fft', N_FFTS)
@pytest.mark.parametrize('hop', HOPS)
def test_frames_ready_emits_every_frame_once_and_never_early(n_fft, hop):
    """K(R) against the direct statement "the frames whose reads are all < R", every R <= 3 n_fft; a push from R_a to R_b emits frames
    K(R_a) .. K(R_b) - 1, so an arrival cut into pushes at R_1 <= R_2 <= ... emits every frame exactly once iff K never decreases --
    walked literally over every split into two and three pushes at the small sizes (a session's state is a function of R alone)."""
    from pwv_amd.audio_frontend import frames_ready
    top = 3 * n_fft
    last = np.array([_reads(k, n_fft, hop).max() for k in range(top // hop + 2)])      # the newest sample frame k needs
    assert np.all(np.diff(last) >= 0)
    K = np.array([frames_ready(R, n_fft, hop) for R in range(top + 1)])
    direct = np.array([int(np.sum(last < R)) for R in range(top + 1)])
    assert np.array_equal(K, direct)                     # not early, not late
    assert np.all(np.diff(K) >= 0) and K[0] == 0 and K[n_fft // 2] == 0 and K[n_fft // 2 + 1] >= 1
    if n_fft <= 32:
        for R in range(top + 1):
            for a in range(R + 1):
                assert list(range(0, K[a])) + list(range(K[a], K[R])) == list(range(K[R]))
                for b in range(a, R + 1):
                    assert list(range(0, K[a])) + list(range(K[a], K[b])) + list(range(K[b], K[R])) == list(range(K[R]))


@pytest.mark.parametrize('n_fft', N_FFTS)
@pytest.mark.parametrize('hop', HOPS)
def test_carry_covers_every_later_read(n_fft, hop):
    """For every R <= 3 n_fft: every index a frame k >= K(R) reads -- pushed later (no right reflection) or at a finish at any L in
    R .. 3 n_fft -- is >= carry_start(R), and the carry R - carry_start(R) is at most n_fft - 1 samples.  The reads are evaluated per
    sample position t with the kernel's reflection rule; the positions of frames k >= K are those >= K hop - h that any frame covers
    (frames tile or overlap for hop <= n_fft and are disjoint beyond)."""
    from pwv_amd.audio_frontend import carry_start, frames_ready
    h, top = n_fft // 2, 3 * n_fft
    K = [frames_ready(R, n_fft, hop) for R in range(top + 1)]
    c = [carry_start(R, n_fft, hop) for R in range(top + 1)]
    assert all(0 <= c[R] <= R and R - c[R] <= n_fft - 1 for R in range(top + 1))
    assert all(c[R] <= c[R + 1] for R in range(top))                              # a carry never needs a sample it has dropped
    Ka, ca = np.array(K), np.array(c)
    t = np.arange(-h, top + h + hop)
    for L in [None] + list(range(h + 1, top + 1)):
        frames = (top // hop + 2) if L is None else (1 + L // hop)                 # the frames that exist
        edge = np.zeros(t.size + 1, dtype=np.int64)                                # (t[0] = -h: frame k covers array positions k hop .. + n_fft - 1)
        begin = np.arange(frames) * hop
        np.add.at(edge, begin, 1)
        np.add.at(edge, np.minimum(begin + n_fft, t.size), -1)
        covered = np.cumsum(edge[:-1]) > 0
        g = np.where(t < 0, -t, t)
        if L is not None:
            g = np.clip(np.where(g >= L, 2 * (L - 1) - g, g), 0, L - 1)
        g = np.where(covered, g, np.iinfo(np.int64).max)
        low = np.minimum.accumulate(g[::-1])[::-1]                                 # low[j]: the lowest index read at array positions >= j
        Rs = np.arange((top if L is None else L) + 1)                              # the states the utterance passed through
        Rs = Rs[Ka[Rs] < frames]                                                   # (those that still have a frame to come)
        bad = low[Ka[Rs] * hop] < ca[Rs]
        assert not bad.any(), (L, Rs[bad][:4], Ka[Rs][bad][:4], ca[Rs][bad][:4])
    # the direct form on a few states, frame by frame
    for R in (0, h, h + 1, min(h + hop, top), n_fft, 2 * n_fft + 1, top):
        for L in (None, max(R, h + 1), top):
            ks = range(K[R], (top // hop + 2) if L is None else (1 + L // hop))
            assert all(_reads(k, n_fft, hop, L).min() >= c[R] for k in ks)


def test_mel_stream_args_layout_matches_ctypes(tmp_path):
    """The C compiler's size and offsets of pwv_mel_stream_args (gcc -std=c99 -pedantic -Werror on include/pwv_hip_mel_stream.h) against the
    ctypes mirror; the entry point is declared in that header -- an extension of pwv_hip.h, which keeps its 52 -- listed in
    _lib.EXTENSION_SYMBOLS and exported by the built library."""
    import subprocess
    from pwv_amd import _lib
    _lib.build_library()
    fields = [n for n, _ in _lib.MelStreamArgs._fields_]
    probe = ['sizeof(pwv_mel_stream_args)'] + ['offsetof(pwv_mel_stream_args, %s)' % f for f in fields] + ['(size_t)PWV_MEL_STREAM_REC', '(size_t)PWV_HIP_VERSION']
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "pwv_hip_mel_stream.h"\nint main(void){ printf("%s\\n", %s); return 0; }\n'
           % (' '.join(['%zu'] * len(probe)), ', '.join(probe)))
    c, exe = str(tmp_path / 't.c'), str(tmp_path / 't')
    with open(c, 'w') as f:
        f.write(src)
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Wextra', '-pedantic', '-Werror', '-I' + os.path.join(ROOT, 'include'), c, '-o', exe])
    got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    want = [ctypes.sizeof(_lib.MelStreamArgs)] + [getattr(_lib.MelStreamArgs, f).offset for f in fields] + [_lib.MEL_STREAM_REC, _lib.HEADER_VERSION]
    assert got == want and _lib.HEADER_VERSION == 301
    assert _lib.MelStreamArgs().struct_size == ctypes.sizeof(_lib.MelStreamArgs)
    assert len(_lib.MEL_REC_FIELDS) == _lib.MEL_STREAM_REC
    text = open(os.path.join(ROOT, 'include', 'pwv_hip_mel_stream.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    assert sorted(set(re.findall(r'\b(pwv_[a-z0-9_]+)\s*\(', code))) == sorted(_lib.EXTENSION_SYMBOLS) == ['pwv_wav_to_mel_db_stream_f32']
    assert not set(_lib.EXTENSION_SYMBOLS) & set(_lib.EXPORTED_SYMBOLS)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(raw, name) for name in _lib.EXTENSION_SYMBOLS)
    for rule in ('READY rule', 'FINISH rule', 'CARRY rule'):
        assert rule in text


def _args(recs, n_fft=32, hop=8, wav_len=64, mel_rows=16):
    """A pwv_mel_stream_args the library accepts up to its launch -- every device pointer a number that is never dereferenced on the
    host -- and the host record array it points to."""
    from pwv_amd import _lib
    host = (ctypes.c_int64 * (len(recs) * _lib.MEL_STREAM_REC))(*[v for r in recs for v in r])
    a = _lib.MelStreamArgs()
    a.wav = a.window = a.mel_basis = a.mel = a.state = a.max_key = a.rec = 4096
    a.rec_host = ctypes.addressof(host)
    a.wav_len, a.mel_rows, a.N, a.n_fft, a.hop, a.n_mels, a.n_blocks, a.n_words = wav_len, mel_rows, len(recs), n_fft, hop, 5, 4, 2
    a.amin, a.max_db, a.min_db = 1e-5, 35.0, -55.0
    return a, host


def _rec(**kw):
    from pwv_amd import _lib
    base = dict(carry_first=0, carry_len=0, chunk_off=0, chunk_len=17, first_frame=0, frames=1, final_len=-1, read_block=0, write_block=1,
                out_row=0, new_carry_first=0, max_word=0)
    base.update(kw)
    return [base[f] for f in _lib.MEL_REC_FIELDS]


def test_mel_stream_refusals_no_gpu(built_lib):
    """Every refusal of pwv_wav_to_mel_db_stream_f32 returns -1 with its field named, before anything touches a device (this process
    has none)."""
    lib = built_lib

    def refused(a, word):
        code = lib.pwv_wav_to_mel_db_stream_f32(ctypes.byref(a), None)
        msg = lib.pwv_last_error()
        assert code == -1 and word in msg, (code, word, msg)

    assert lib.pwv_wav_to_mel_db_stream_f32(None, None) == -1 and b'NULL' in lib.pwv_last_error()
    a, keep = _args([_rec()])
    a.struct_size = 0
    refused(a, b'struct_size')
    a.struct_size = ctypes.sizeof(a) - 4
    refused(a, b'struct_size')
    for field in ('wav', 'window', 'mel_basis', 'mel', 'state', 'max_key', 'rec', 'rec_host'):
        a, keep = _args([_rec()])
        setattr(a, field, None)
        refused(a, b'NULL pointer')
        refused(a, field.encode())
    for n_fft in (31, 2050, 0):
        a, keep = _args([_rec()], n_fft=n_fft)
        refused(a, b'n_fft')
    a, keep = _args([_rec()], hop=0)
    refused(a, b'hop')
    a, keep = _args([_rec()])
    a.max_db = a.min_db
    refused(a, b'max_db == min_db')
    # a finishing session: L = h = 16 is too short, L = 17 is the shortest legal (it gets as far as the launch on a GPU; not called here)
    a, keep = _args([_rec(carry_len=16, chunk_len=0, frames=0, final_len=16)])
    refused(a, b'final_len')
    a, keep = _args([_rec(carry_len=16, chunk_len=0, frames=2, final_len=20)])      # not what was received
    refused(a, b'final_len')
    # records that would make the kernel read or write outside what the caller holds
    for bad, word in ((dict(chunk_len=65), b'chunk'), (dict(chunk_off=60), b'chunk'), (dict(frames=17), b'rows'), (dict(out_row=16), b'rows'),
                      (dict(write_block=0), b'block'), (dict(read_block=4), b'block'), (dict(max_word=2), b'max word'),
                      (dict(chunk_len=16), b'read samples'), (dict(frames=2), b'read samples'), (dict(carry_first=3), b'read samples'),
                      (dict(carry_len=33), b'carry'), (dict(new_carry_first=18), b'new carry')):
        a, keep = _args([_rec(), _rec(**bad)])
        refused(a, word)
        refused(a, b'record 1')


def test_streaming_mel_refuses_raw_db():
    """Normalised mode only: construction without both max_db and min_db is a ValueError (before any device is asked for)."""
    from types import SimpleNamespace
    from pwv_amd.audio_frontend import StreamingMel
    base = dict(sr=16000, n_fft=32, win_length=20, hop_length=8, n_mels=5)
    for extra in (dict(), dict(max_db=35.0), dict(min_db=-55.0), dict(max_db=None, min_db=-55.0)):
        with pytest.raises(ValueError, match='max_db'):
            StreamingMel(1, signal=SimpleNamespace(**dict(base, **extra)))
    with pytest.raises(ValueError, match='slots'):
        StreamingMel(0, signal=SimpleNamespace(max_db=35.0, min_db=-55.0, **base))


def test_live_flag_refusals(tmp_path, monkeypatch):
    """generate --live: without --stream, with --graph, on synthetic or .npy inputs -> ValueError, before a GPU is asked for."""
    from pwv_amd.generate import generate
    from pwv_amd.hparam import hparam as hp
    with pytest.raises(ValueError, match='--live'):
        generate('bench/c1', live=True)
    with pytest.raises(ValueError, match='--live'):
        generate('bench/c1', stream=5, graph=True, live=True)
    with pytest.raises(ValueError, match='--live'):
        generate('bench/c1', stream=5, live=True)                   # data_path: synthetic
    np.save(str(tmp_path / 'a.npy'), np.zeros((4, 80), dtype=np.float32))
    orig = type(hp).set_hparam_yaml

    def patched(self, case, *a, **k):
        r = orig(self, case, *a, **k)
        self.data_path = str(tmp_path / '*.npy')
        return r

    monkeypatch.setattr(type(hp), 'set_hparam_yaml', patched)
    with pytest.raises(ValueError, match='--live'):
        generate('bench/c1', stream=5, live=True)


def test_top_db_headroom_of_the_default_hparams():
    """|wav| <= 1 bounds every |STFT| bin by sum |window| and every band by its filter's row sum times that: 17.02 dB with the default
    hparams, below min_db + top_db = 25 -- the one-shot's floor max - top_db then never rises above min_db, whatever the utterance.
    With min_db = -70 the bound does not hold the floor down."""
    from pwv_amd import audio_frontend as A
    from pwv_amd.hparam import hparam as hp
    hp.set_hparam_yaml('default')
    s = hp.signal
    fb = A.mel_filterbank(s.sr, s.n_fft, s.n_mels)
    window = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(s.win_length) / s.win_length)       # the 400-sample periodic hann
    bound = 20.0 * np.log10((fb.sum(axis=1) * np.abs(window).sum()).max())
    assert abs(bound - 17.02) < 0.01 and abs(A.mel_db_bound(s.sr, s.n_fft, s.win_length, s.n_mels) - bound) < 1e-9
    assert (float(s.min_db), A.TOP_DB) == (-55.0, 80.0)
    assert bound < float(s.min_db) + A.TOP_DB
    assert not bound < -70.0 + A.TOP_DB


def test_mel_stream_kernel_uses_no_scratch():
    """The compiler's resource remarks (gfx950 device code) for the kernels of csrc/pwv_audio.hip: no scratch, no spilled register."""
    from tests.util import kernel_resources
    res = kernel_resources('pwv_audio.hip')
    new = [n for n in res if 'stft_mel_stream_kernel' in n]
    assert len(new) == 1, sorted(res)
    for name, r in res.items():
        assert r['scratch'] == 0 and r['vgpr_spills'] == 0 and r['sgpr_spills'] == 0 and not r['dynamic_stack'], (name, r)
