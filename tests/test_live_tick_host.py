"""CPU: the host side of the live tick (graph.GraphedLiveStream, include/pwv_hip_live_tick.h) -- the C ABI addition and its refusals, and
the bookkeeping of its two kernels (records -> rows written, commit -> session table) in their numpy restatement against the ready /
carry arithmetic of the streaming front-end.  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_live_tick_args_layout_matches_ctypes(tmp_path):
    """The C compiler's size and offsets of pwv_live_tick_args (gcc -std=c99 -pedantic -Werror on include/pwv_hip_live_tick.h) against
    the ctypes mirror; the header declares exactly _lib.LIVE_TICK_SYMBOLS, which are disjoint from the two older lists and exported by
    the built library; pwv_hip.h and pwv_hip_mel_stream.h keep their version and their record."""
    import subprocess
    from pwv_amd import _lib
    _lib.build_library()
    fields = [n for n, _ in _lib.LiveTickArgs._fields_]
    probe = (['sizeof(pwv_live_tick_args)'] + ['offsetof(pwv_live_tick_args, %s)' % f for f in fields]
             + ['(size_t)PWV_LIVE_TICK_REC', '(size_t)PWV_MEL_STREAM_REC', '(size_t)PWV_HIP_VERSION'])
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "pwv_hip_live_tick.h"\nint main(void){ printf("%s\\n", %s); return 0; }\n'
           % (' '.join(['%zu'] * len(probe)), ', '.join(probe)))
    c, exe = str(tmp_path / 't.c'), str(tmp_path / 't')
    with open(c, 'w') as f:
        f.write(src)
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Wextra', '-pedantic', '-Werror', '-I' + os.path.join(ROOT, 'include'), c, '-o', exe])
    got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    want = ([ctypes.sizeof(_lib.LiveTickArgs)] + [getattr(_lib.LiveTickArgs, f).offset for f in fields]
            + [_lib.LIVE_TICK_REC, _lib.MEL_STREAM_REC, _lib.HEADER_VERSION])
    assert got == want and _lib.HEADER_VERSION == 301
    assert _lib.LiveTickArgs().struct_size == ctypes.sizeof(_lib.LiveTickArgs)
    assert len(_lib.LIVE_REC_FIELDS) == _lib.LIVE_TICK_REC
    text = open(os.path.join(ROOT, 'include', 'pwv_hip_live_tick.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    assert '#include "pwv_hip_mel_stream.h"' in code
    assert sorted(set(re.findall(r'\b(pwv_[a-z0-9_]+)\s*\(', code))) == sorted(_lib.LIVE_TICK_SYMBOLS) == ['pwv_live_tick_commit', 'pwv_live_tick_mel']
    assert not set(_lib.LIVE_TICK_SYMBOLS) & (set(_lib.EXPORTED_SYMBOLS) | set(_lib.EXTENSION_SYMBOLS))
    assert len(_lib.EXPORTED_SYMBOLS) == 52 and _lib.EXTENSION_SYMBOLS == ('pwv_wav_to_mel_db_stream_f32',)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(raw, name) for name in _lib.LIVE_TICK_SYMBOLS)


def _rec(**kw):
    from pwv_amd import _lib
    base = dict(carry_first=0, carry_len=0, chunk_off=0, chunk_len=17, first_frame=0, frames=1, final_len=-1, slot=0, flags=_lib.LIVE_ACTIVE,
                out_row=0, new_carry_first=0, first_row=0)
    base.update(kw)
    return [base[f] for f in _lib.LIVE_REC_FIELDS]


def _args(recs, n_fft=32, hop=8):
    """A pwv_live_tick_args the library accepts up to its launch -- every device pointer a number that is never dereferenced on the host --
    and the host record array it points to."""
    from pwv_amd import _lib
    host = (ctypes.c_int64 * (len(recs) * _lib.LIVE_TICK_REC))(*[v for r in recs for v in r])
    a = _lib.LiveTickArgs()
    a.wav = a.window = a.mel_basis = a.mel = a.first = a.state = a.max_key = a.scratch = a.sess = a.rec = a.words = 4096
    a.rec_host = ctypes.addressof(host)
    a.wav_cap, a.mel_rows, a.N, a.n_slots, a.n_first, a.n_fft, a.hop, a.n_mels = 64, 16, len(recs), 2, 2, n_fft, hop, 5
    a.amin, a.max_db, a.min_db, a.limit_db = 1e-5, 35.0, -55.0, 25.0
    return a, host


@pytest.mark.parametrize('entry', ['pwv_live_tick_mel', 'pwv_live_tick_commit'])
def test_live_tick_refusals_no_gpu(built_lib, entry):
    """Every refusal of the two entry points returns -1 with its field named, before anything touches a device (this process has none)."""
    from pwv_amd import _lib
    call = getattr(built_lib, entry)

    def refused(a, word):
        code = call(ctypes.byref(a), None)
        msg = built_lib.pwv_last_error()
        assert code == -1 and word in msg and entry.encode() in msg, (code, word, msg)

    assert call(None, None) == -1 and b'NULL' in built_lib.pwv_last_error()
    a, keep = _args([_rec()])
    a.struct_size = 0
    refused(a, b'struct_size')
    a.struct_size = ctypes.sizeof(a) - 4
    refused(a, b'struct_size')
    for field in ('wav', 'window', 'mel_basis', 'mel', 'first', 'state', 'max_key', 'scratch', 'sess', 'rec', 'words'):
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
    for field in ('N', 'n_slots'):
        a, keep = _args([_rec()])
        setattr(a, field, 0)
        refused(a, field.encode())
    # records that would make a kernel read or write outside what the call was given
    first = _lib.LIVE_ACTIVE | _lib.LIVE_FIRST
    for bad, word in ((dict(chunk_len=65), b'chunk'), (dict(chunk_off=60), b'chunk'), (dict(chunk_off=-1), b'chunk'), (dict(frames=17), b'rows'),
                      (dict(out_row=16), b'rows'), (dict(out_row=-1), b'rows'), (dict(slot=2), b'blocks'), (dict(slot=-1), b'blocks'),
                      (dict(flags=first, first_row=2), b'words'), (dict(flags=first, first_row=-1), b'words'), (dict(carry_len=33), b'carry'),
                      (dict(final_len=16), b'final_len')):
        a, keep = _args([_rec(), _rec(**bad)])
        refused(a, word)
        refused(a, b'record 1')
    # an inactive record is skipped whatever it holds, and a frame that goes to `first` takes no row of mel (checked up to the launch only:
    # the accepted call is not made here)
    assert _rec(flags=0, chunk_len=1 << 40)[3] == 1 << 40


def _reads(k, n_fft, hop, L=None):
    """The sample indices frame k reads (csrc/pwv_audio.hip): t = k hop - h .. k hop + h - 1, t < 0 at -t, t >= L at 2 (L - 1) - t, clamped."""
    t = k * hop - n_fft // 2 + np.arange(n_fft)
    t = np.where(t < 0, -t, t)
    if L is not None:
        t = np.clip(np.where(t >= L, 2 * (L - 1) - t, t), 0, L - 1)
    return t


@pytest.mark.parametrize('raised', [False, True], ids=['clean', 'raised_words'])
@pytest.mark.parametrize('hop', [8, 80])
@pytest.mark.parametrize('n_fft', [32, 512])
def test_live_tick_bookkeeping_against_the_ready_and_carry_rules(n_fft, hop, raised):
    """Three sessions through ticks that hold a 0-frame tick (a start whose chunk is below n_fft / 2 + 1 samples), a start, an end in the
    same record as its last chunk, an end without a chunk and a restart of the slot.  Per tick the restatement of the mel kernel
    (audio_frontend.live_tick_rows) writes, per record, exactly the frames K(R before) .. K(R after) - 1 of frames_ready (.. L // hop at
    an end), each once, in row order from the record's row -- the utterance's first frame into `first` --, every frame reading only
    samples in [carry_start(R before), R after), and one carry per continuing session into the block the session does not stand on,
    holding samples carry_start(R after) .. R after - 1; the restatement of the commit (live_tick_commit) then leaves the table at
    {generation flipped, R after, K after} (zeros after an end).  raised_words: every second tick meets a raised word -- the table does not
    move and the same chunks are fed again."""
    from pwv_amd import _lib
    from pwv_amd import audio_frontend as A
    h = n_fft // 2
    n_slots, N = 3, 3
    mel_rows = (6 * n_fft) // hop + 8
    wav_cap = mel_rows * hop + N * (h + hop)
    # (slot, samples, start, end) per tick; slot 2's first chunk brings no frame, slot 1 ends with a chunk, slot 0 without one and restarts
    ticks = [[(0, h + 1 + hop, True, False), (2, h - 3, True, False)],
             [(0, 3 * hop + 1, False, False), (1, 2 * n_fft + 5, True, False), (2, 7, False, False)],
             [(1, hop + 3, False, True), (0, 0, False, True), (2, 2 * hop, False, False)],
             [(0, n_fft, True, False), (2, 1, False, False)],
             [(0, h + 2, False, True), (2, hop, False, True)]]
    sess = np.zeros((n_slots, 4), np.int64)
    sess[1, 0] = 1
    max_key = np.full((n_slots,), A.KEY_NONE, np.int32)
    scratch = np.full((N,), A.KEY_NONE, np.int32)
    total = {s: 0 for s in range(n_slots)}          # frames emitted per utterance, against 1 + L // hop at its end
    attempt = zero_frames = 0
    for tick in ticks:
        while True:
            attempt += 1
            words = (0, 1) if raised and attempt % 2 == 1 else (0, 0)
            recs, want, off, row, entry = np.zeros((N, _lib.LIVE_TICK_REC), np.int64), [], 0, 0, 0
            for i, (s, n, start, end) in enumerate(tick):
                R0, K0 = (0, 0) if start else (int(sess[s, 1]), int(sess[s, 2]))
                r = A.live_record(R0, K0, n, end, n_fft, hop)
                R1 = R0 + n
                K1 = 1 + R1 // hop if end else A.frames_ready(R1, n_fft, hop)          # the rules, stated directly
                assert (r.frames, r.first_frame) == (K1 - K0, K0) and r.carry_first == A.carry_start(R0, n_fft, hop)
                first = K0 == 0 and K1 > 0
                flags = _lib.LIVE_ACTIVE | (_lib.LIVE_START if start else 0) | (_lib.LIVE_FIRST if first else 0)
                recs[i] = (r.carry_first, r.carry_len, off, n, r.first_frame, r.frames, r.final_len, s, flags, row, r.new_carry_first, entry)
                want.append(dict(slot=s, R0=R0, R1=R1, K0=K0, K1=K1, end=end, first=first, row=row, entry=entry, start=start))
                off, row, entry = off + n, row + (K1 - K0) - (1 if first else 0), entry + (1 if K1 > K0 else 0)
            assert off <= wav_cap and row <= mel_rows
            zero_frames += sum(1 for w in want if w['K1'] == w['K0'])
            frames, carries = A.live_tick_rows(recs, sess, n_slots, wav_cap, mel_rows, N, n_fft)
            for i, w in enumerate(want):
                mine = sorted((k, where, r) for (where, r), (j, k, rd) in frames.items() if j == i)
                assert [k for k, _, _ in mine] == list(range(w['K0'], w['K1']))          # every ready frame once, none early
                g = int(sess[w['slot'], 0]) & 1
                for x, (k, where, r) in enumerate(mine):
                    if w['first']:
                        assert (where, r) == (('first', w['entry']) if x == 0 else ('mel', w['row'] + x - 1))
                    else:
                        assert (where, r) == ('mel', w['row'] + x)
                    assert frames[(where, r)][2] == 2 * w['slot'] + g
                    t = _reads(k, n_fft, hop, w['R1'] if w['end'] else None)
                    assert t.min() >= (0 if w['start'] else A.carry_start(w['R0'], n_fft, hop)) and t.max() < w['R1']
                wrote = [(blk, v) for blk, v in carries.items() if v[0] == i]
                if w['end'] or w['R1'] == 0:
                    assert wrote == []
                else:
                    c1 = A.carry_start(w['R1'], n_fft, hop)
                    assert wrote == [(2 * w['slot'] + 1 - g, (i, 2 * w['slot'] + g, c1, w['R1'] - c1))] and w['R1'] - c1 <= n_fft - 1
            assert len(frames) == sum(w['K1'] - w['K0'] for w in want)
            # the commit: scratch maxima of this tick, slot 2 well over the limit in the tick that ends it
            keys = np.array([A._db_to_key(-20.0 + i) for i in range(N)], np.int32)
            if tick is ticks[4]:
                keys[1] = A._db_to_key(30.0)
            before = (sess.copy(), max_key.copy())
            sess2, max2, scratch2 = A.live_tick_commit(sess, max_key, keys, recs, words, 25.0, wav_cap, mel_rows, n_fft)
            assert np.all(scratch2 == A.KEY_NONE)
            if words != (0, 0):
                assert np.array_equal(sess2, before[0]) and np.array_equal(max2, before[1])
                continue          # refused: the same chunks again
            for i, w in enumerate(want):
                s = w['slot']
                assert sess2[s, 0] == before[0][s, 0] ^ 1
                assert tuple(sess2[s, 1:3]) == ((0, 0) if w['end'] else (w['R1'], w['K1']))
                folded = int(keys[i]) if w['start'] else max(int(before[1][s]), int(keys[i]))
                assert max2[s] == (A.KEY_NONE if w['end'] else folded)
                assert sess2[s, 3] == (1 if folded > A._db_to_key(25.0) else before[0][s, 3])
                total[s] = (0 if w['start'] else total[s]) + w['K1'] - w['K0']
                if w['end']:
                    assert total[s] == 1 + w['R1'] // hop
            untouched = [s for s in range(n_slots) if s not in [w['slot'] for w in want]]
            assert np.array_equal(sess2[untouched], before[0][untouched]) and np.array_equal(max2[untouched], before[1][untouched])
            sess, max_key, scratch = sess2, max2, scratch2
            break
    assert zero_frames >= 1          # (slot 2's first chunk)
    assert sess[2, 3] == 1 and sess[0, 3] == 0 and sess[1, 3] == 0 and np.all(sess[:, 1:3] == 0)


def test_live_tick_restatement_clamps_a_stale_table():
    """Garbage records -- any slot, offsets, counts, rows and flags -- give the restatement (and the kernel it restates) only rows inside
    mel and first, blocks inside the state and chunks inside the wav buffer."""
    from pwv_amd import audio_frontend as A
    rng = np.random.default_rng(3)
    n_slots, N, wav_cap, mel_rows, n_fft = 3, 4, 500, 12, 32
    sess = np.zeros((n_slots, 4), np.int64)
    for _ in range(200):
        recs = rng.integers(-40, 600, (N, 12))
        recs[:, 8] = rng.integers(0, 8, N)
        recs[rng.integers(0, N), rng.integers(0, 12)] = rng.choice([-2 ** 63, 2 ** 63 - 1])
        frames, carries = A.live_tick_rows(recs, sess, n_slots, wav_cap, mel_rows, N, n_fft)
        for (where, row) in frames:
            assert 0 <= row < (N if where == 'first' else mel_rows)
        for blk, (i, rd, c1, keep) in carries.items():
            assert 0 <= blk < 2 * n_slots and 0 <= rd < 2 * n_slots and blk != rd and 0 <= keep <= n_fft
        for rec in recs:
            q = A._live_clamped(rec, n_slots, wav_cap, mel_rows, n_fft)
            assert 0 <= q['coff'] and q['coff'] + q['chlen'] <= wav_cap and 0 <= q['clen'] <= n_fft and 0 <= q['slot'] < n_slots
        s2, m2, sc2 = A.live_tick_commit(sess, np.zeros(n_slots, np.int32), np.zeros(N, np.int32), recs, (0, 0), 25.0, wav_cap, mel_rows, n_fft)
        assert s2.shape == sess.shape and np.all(sc2 == A.KEY_NONE)


def test_graphed_live_refuses_a_mismatch_before_any_capture():
    """graphed_live names the field on which the front-end and the stream disagree -- checked on stand-ins: nothing is captured, no
    device is asked for."""
    from types import SimpleNamespace
    from pwv_amd import graph
    from pwv_amd._lib import PwvError
    st = SimpleNamespace(n_slots=3, hop=80, n_mels=80, _zero_block=6)
    for field, fe in (('slots', SimpleNamespace(n_slots=2, hop=80, n_mels=80)), ('hop_length', SimpleNamespace(n_slots=3, hop=16, n_mels=80)),
                      ('n_mels', SimpleNamespace(n_slots=3, hop=80, n_mels=5))):
        with pytest.raises(PwvError, match=field):
            graph.GraphedLiveStream(st, fe, 3, 2400)


def test_live_graph_flag_refusals():
    """generate --live=graph: without --stream, or with --graph as well -> the ValueError naming --live, before a GPU is asked for."""
    from pwv_amd.generate import generate
    with pytest.raises(ValueError, match='--live'):
        generate('bench/c1', live='graph')
    with pytest.raises(ValueError, match='--live'):
        generate('bench/c1', stream=5, graph=True, live='graph')
    with pytest.raises(ValueError, match='--live'):
        generate('bench/c1', stream=5, live='sometimes')
    with pytest.raises(ValueError, match='--live'):
        generate('bench/c1', stream=5, live='graph')                   # data_path: synthetic


def test_live_tick_kernels_use_no_scratch():
    """The compiler's resource remarks (gfx950 device code) for the two new kernels of csrc/pwv_audio.hip: no scratch, no spilled register."""
    from tests.util import kernel_resources
    res = kernel_resources('pwv_audio.hip')
    new = [n for n in res if 'live_tick' in n]
    assert len(new) == 2, sorted(res)
    for name in new:
        r = res[name]
        assert r['scratch'] == 0 and r['vgpr_spills'] == 0 and r['sgpr_spills'] == 0 and not r['dynamic_stack'], (name, r)
