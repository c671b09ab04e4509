"""wav -> normalised dB mel-spectrogram, the input side of the generation path.

Restates, in numpy, the exact recipe `Dataset._get_wav_and_melspec` applies at generation time
(/root/reference/data_load.py:37-56 with audio.py:14-37,102-141,232-243,278-286,327-356), whose
arithmetic lives in librosa 0.5.1 (requirements.txt; not installable here):

    read_wav(sr) -> trim_wav (librosa.effects.trim: top_db 60, frame 2048, hop 512, ref max)
    -> first `length` samples -> fix_length (zero pad) -> STFT (n_fft 512, win 400 periodic hann
    zero-padded to n_fft, hop 80, center, reflect) -> |.| -> Slaney mel filterbank (80 bands,
    0..sr/2, area-normalised) -> amplitude_to_db (amin 1e-5, top_db 80) ->
    (clip((db - min_db)/(max_db - min_db), 0, 1) - 0.5) * 2

so the mel has exactly 1 + length/hop frames and values in [-1, 1], which is what the network
was trained on.  File reading, trimming and padding are host-side data preparation; the spectrogram itself
(STFT -> mel -> dB -> normalisation) also exists as a HIP kernel (`wav_to_mel_device`, csrc/pwv_audio.hip) so that
generate() on wav input keeps the mel on the device.  ROLE OF THE NUMPY FUNCTIONS: `wav2melspec_db` and its helpers are a
CPU restatement of the reference recipe that serves (a) as the host path for .npy / CPU-side inputs and (b) as the CHECKER
of the HIP kernel in tests/test_gpu_unfused_and_e2e.py::test_device_mel_frontend_matches_numpy_restatement -- they are test
reference living in the product package, not an independent oracle; `trim_wav` (librosa.effects.trim) and the resampling in
`read_wav` have property tests only (tests/test_audio_frontend.py).  Parity with librosa is by construction from its documented algorithms (no librosa here to diff against; the
STFT is checked against scipy.signal.stft and the filterbank against hand-derived constants in tests/test_audio_frontend.py);
resampling uses scipy's polyphase filter where librosa used resampy (only matters when the file's
rate differs from hp.signal.sr).
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional

import numpy as np
import torch

from .hparam import hparam as hp


def read_wav(path: str, sr: int) -> np.ndarray:
    """audio.py:14-16 (librosa.load, mono, float32 in [-1, 1], resampled to sr)."""
    from scipy.io import wavfile
    rate, data = wavfile.read(path)
    if data.dtype.kind == 'i':
        data = data.astype(np.float32) / float(np.iinfo(data.dtype).max + 1)
    elif data.dtype.kind == 'u':
        data = (data.astype(np.float32) - 128.0) / 128.0
    else:
        data = data.astype(np.float32)
    if data.ndim > 1:
        data = data.mean(axis=1)
    if rate != sr:
        from math import gcd
        from scipy.signal import resample_poly
        g = gcd(int(rate), int(sr))
        data = resample_poly(data, sr // g, rate // g).astype(np.float32)
    return data


def _frame_rmse_db(y: np.ndarray, frame_length: int, hop_length: int) -> np.ndarray:
    ypad = np.pad(y, frame_length // 2, mode='reflect')
    n = 1 + (len(ypad) - frame_length) // hop_length
    idx = np.arange(frame_length)[None, :] + hop_length * np.arange(n)[:, None]
    mse = np.mean(np.abs(ypad[idx]) ** 2, axis=1)
    ref = max(1e-10, mse.max())
    return 10.0 * np.log10(np.maximum(1e-10, mse)) - 10.0 * np.log10(ref)


def trim_wav(wav: np.ndarray, top_db: float = 60.0, frame_length: int = 2048, hop_length: int = 512) -> np.ndarray:
    """audio.py:29-31 (librosa.effects.trim defaults): drop leading / trailing frames quieter than
    top_db below the loudest frame."""
    if len(wav) == 0:
        return wav
    nonsilent = np.flatnonzero(_frame_rmse_db(wav, frame_length, hop_length) > -top_db)
    if nonsilent.size == 0:
        return wav[:0]
    start = int(nonsilent[0]) * hop_length
    end = min(len(wav), (int(nonsilent[-1]) + 1) * hop_length)
    return wav[start:end]


def fix_length(wav: np.ndarray, length: int) -> np.ndarray:
    """audio.py:34-37 (librosa.util.fix_length: truncate or zero-pad at the end)."""
    if len(wav) >= length:
        return wav[:length]
    return np.pad(wav, (0, length - len(wav)))


def stft_mag(wav: np.ndarray, n_fft: int, win_length: int, hop_length: int) -> np.ndarray:
    """|librosa.stft| (audio.py:133-134): centred, reflect-padded, periodic hann of win_length
    zero-padded to n_fft.  Returns [1 + n_fft/2, 1 + len/hop]."""
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win_length) / win_length)     # scipy get_window('hann', fftbins=True)
    lpad = (n_fft - win_length) // 2
    window = np.pad(win, (lpad, n_fft - win_length - lpad))
    ypad = np.pad(wav.astype(np.float64), n_fft // 2, mode='reflect')
    n_frames = 1 + (len(ypad) - n_fft) // hop_length
    idx = np.arange(n_fft)[None, :] + hop_length * np.arange(n_frames)[:, None]
    return np.abs(np.fft.rfft(ypad[idx] * window[None, :], axis=1)).T


def _hz_to_mel(f):
    f = np.asanyarray(f, dtype=np.float64)
    mels = f / (200.0 / 3)
    log_t = f >= 1000.0
    return np.where(log_t, 15.0 + np.log(np.maximum(f, 1e-10) / 1000.0) / (np.log(6.4) / 27.0), mels)


def _mel_to_hz(m):
    m = np.asanyarray(m, dtype=np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), (200.0 / 3) * m)


def mel_filterbank(sr: int, n_fft: int, n_mels: int) -> np.ndarray:
    """librosa.filters.mel(sr, n_fft, n_mels) (audio.py:241): Slaney scale, fmin 0, fmax sr/2,
    triangles normalised to unit area.  [n_mels, 1 + n_fft/2]."""
    fft_f = np.linspace(0, sr / 2.0, 1 + n_fft // 2)
    mel_f = _mel_to_hz(np.linspace(_hz_to_mel(0.0), _hz_to_mel(sr / 2.0), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fft_f[None, :]
    weights = np.zeros((n_mels, 1 + n_fft // 2))
    for i in range(n_mels):
        lower = -ramps[i] / fdiff[i]
        upper = ramps[i + 2] / fdiff[i + 1]
        weights[i] = np.maximum(0, np.minimum(lower, upper))
    enorm = 2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels])
    return weights * enorm[:, None]


def amplitude_to_db(s: np.ndarray, amin: float = 1e-5, top_db: float = 80.0) -> np.ndarray:
    """librosa.amplitude_to_db (audio.py:347), ref 1.0."""
    db = 10.0 * np.log10(np.maximum(amin ** 2, np.abs(s) ** 2))
    return np.maximum(db, db.max() - top_db)


def normalize_db(db: np.ndarray, max_db: float, min_db: float) -> np.ndarray:
    """audio.py:254-286: [-1, 1]."""
    return (np.clip((db - min_db) / (max_db - min_db), 0, 1) - 0.5) * 2


def wav2melspec_db(wav, sr, n_fft, win_length, hop_length, n_mels, max_db=None, min_db=None) -> np.ndarray:
    """audio.py:341-356 -> [t, n_mels]."""
    mel = mel_filterbank(sr, n_fft, n_mels) @ stft_mag(wav, n_fft, win_length, hop_length)
    db = amplitude_to_db(mel)
    if max_db and min_db:
        db = normalize_db(db, max_db, min_db)
    return db.T.astype(np.float32)


def analysis_window(n_fft: int, win_length: int) -> np.ndarray:
    """Periodic hann of win_length, centred in n_fft (what librosa.stft builds from win_length < n_fft)."""
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win_length) / win_length)
    lpad = (n_fft - win_length) // 2
    return np.pad(win, (lpad, n_fft - win_length - lpad))


_device_consts = {}


def _consts(device, s):
    """(analysis window [n_fft], mel filterbank [n_mels, 1 + n_fft/2]) as fp32 on `device` for the signal settings `s`, built once."""
    key = (device, s.sr, s.n_fft, s.win_length, s.n_mels)
    if key not in _device_consts:
        _device_consts[key] = (torch.from_numpy(analysis_window(s.n_fft, s.win_length).astype(np.float32)).to(device),
                               torch.from_numpy(mel_filterbank(s.sr, s.n_fft, s.n_mels).astype(np.float32)).to(device))
    return _device_consts[key]


def wav_to_mel_device(wav, normalise: Optional[bool] = None):
    """wav [N, L] float32 on the GPU -> (normalised) dB mel [N, 1 + L/hop, n_mels] on the GPU (pwv_wav_to_mel_db_f32),
    with the current hparams' signal settings.  Like audio.wav2melspec_db (audio.py:350) the dB range is normalised only
    when BOTH max_db and min_db are set; `normalise` overrides."""
    from . import _lib, engine
    s = hp.signal
    wav = engine._require_cuda_f32(wav, 'wav')
    if wav.dim() != 2:
        raise ValueError('wav must be [N, L], got %s' % (tuple(wav.shape),))
    n, length = wav.shape
    window, basis = _consts(wav.device, s)
    mel = torch.empty((n, 1 + length // s.hop_length, s.n_mels), dtype=torch.float32, device=wav.device)
    if normalise is None:
        normalise = bool(s.get('max_db', None) and s.get('min_db', None))
    max_db, min_db = (float(s.max_db), float(s.min_db)) if normalise else (1.0, 0.0)      # (unused by the kernel when not normalising)
    _lib.check(_lib.lib().pwv_wav_to_mel_db_f32(wav.data_ptr(), window.data_ptr(), basis.data_ptr(), mel.data_ptr(), n, length, s.n_fft,
                                                s.hop_length, s.n_mels, 1e-5, 80.0, max_db, min_db, int(normalise),
                                                engine._stream()), 'pwv_wav_to_mel_db_f32')
    return mel


# ---- the streaming front-end (include/pwv_hip_mel_stream.h; DESIGN.md section 9, "Streaming the mel front-end") ----
TOP_DB = 80.0       # amplitude_to_db's floor below the utterance maximum (audio.py:347)
AMIN = 1e-5


def frames_ready(received: int, n_fft: int, hop: int) -> int:
    """K(R): the frames of a centred, reflect-padded STFT whose every sample lies among the first `received` of the utterance, no right
    reflection involved.  Frame 0's left reflection reads sample n_fft/2; frame k >= 1 ends at sample k hop + n_fft/2 - 1."""
    h = n_fft // 2
    return 0 if received < h + 1 else 1 + (received - h) // hop


def carry_start(received: int, n_fft: int, hop: int) -> int:
    """c(R): the first sample a session keeps between pushes.  Samples c .. R - 1 hold whatever a later frame can read: the next frame
    to emit begins at K hop - n_fft/2, and a right reflection at any final length L >= R reaches back to 2 (L - 1) - (L + n_fft/2 - 1)
    >= R - n_fft/2 - 1.  Fewer than n_fft samples."""
    h = n_fft // 2
    return max(0, min(frames_ready(received, n_fft, hop) * hop - h, received - h - 1))


def mel_db_bound(sr: int, n_fft: int, win_length: int, n_mels: int) -> float:
    """The raw dB no wav with |samples| <= 1 can exceed: every |STFT| bin is at most sum |window|, so a band is at most its filter's
    row sum times that."""
    return float(20.0 * np.log10(mel_filterbank(sr, n_fft, n_mels).sum(axis=1).max() * np.abs(analysis_window(n_fft, win_length)).sum()))


def _key_to_db(key: int) -> Optional[float]:
    """The float behind an order-preserving max word (None: nothing seen yet)."""
    key = int(key)
    if key == -(1 << 31):
        return None
    bits = key if key >= 0 else key ^ 0x7fffffff
    return float(np.array([bits & 0xffffffff], dtype=np.uint32).view(np.float32)[0])


KEY_NONE = -(1 << 31)      # a max word that has seen nothing


class LiveRecord(NamedTuple):
    """live_record: what one session's part of a tick comes to (the streaming record's arithmetic, StreamingMel._launch)."""
    carry_first: int         # c(R before)
    carry_len: int
    first_frame: int         # K before
    frames: int              # frames the tick emits
    final_len: int           # L when the utterance ends with this chunk, else -1
    new_carry_first: int     # c(R after)
    received: int            # R after (0 after an end: the slot is fresh)
    emitted: int             # K after (0 after an end)


def live_record(received: int, emitted: int, n: int, end: bool, n_fft: int, hop: int) -> LiveRecord:
    """A session that has received `received` samples and emitted `emitted` frames is given `n` more; `end`: its utterance ends with
    them, at L = received + n (L <= n_fft / 2 is a ValueError, as in the one-shot).  Host arithmetic alone."""
    r1 = received + n
    if end and r1 <= n_fft // 2:
        raise ValueError('an utterance of L = %d samples ends: L must exceed n_fft / 2 = %d' % (r1, n_fft // 2))
    k1 = 1 + r1 // hop if end else frames_ready(r1, n_fft, hop)
    c0 = carry_start(received, n_fft, hop)
    frames = max(k1 - emitted, 0)
    return LiveRecord(c0, received - c0, emitted, frames, r1 if end else -1, c0 if end else carry_start(r1, n_fft, hop),
                      0 if end else r1, 0 if end else emitted + frames)


def _live_clamped(rec, n_slots: int, wav_cap: int, mel_rows: int, n_fft: int):
    """(numpy restatement of live_record, csrc/pwv_audio.hip)  Record `rec` (12 int64) as both kernels of a live tick read it."""
    c0, clen, coff, chlen, first, frames, L, slot, flags, row, c1, first_row = [int(v) for v in rec]
    active = bool(flags & 1) and 0 <= slot < n_slots
    clen = 0 if flags & 2 else min(max(clen, 0), n_fft)
    coff = min(max(coff, 0), wav_cap)
    chlen = min(max(chlen, 0), wav_cap - coff)
    frames = min(max(frames, 0), mel_rows + 1) if clen + chlen > 0 else 0
    return dict(active=active, slot=slot if active else 0, flags=flags, c0=min(max(c0, 0), 1 << 62), clen=clen, coff=coff, chlen=chlen,
                first=min(max(first, 0), 1 << 40), frames=frames, L=min(max(L, -1), 1 << 62), c1=min(max(c1, 0), 1 << 62), row=row,
                first_row=first_row, scan_frames=min(max(int(rec[5]), 0), mel_rows + 1))


def live_tick_rows(recs, sess, n_slots: int, wav_cap: int, mel_rows: int, n_first: int, n_fft: int):
    """(numpy restatement of live_tick_mel_kernel's bookkeeping)  What the workgroups of a live tick write, from its records (int64
    [N, 12]) and the front-end session table `sess` (int64 [n_slots, 4]): (frames, carries) with frames = {('mel' | 'first', row): (record,
    frame number of the utterance, state block read)} and carries = {state block written: (record, state block read, first sample kept,
    samples kept)}.  Workgroup b of the mel_rows + 2 N is frame x of the first active record whose frames + 1 it falls into, x == frames
    its carry."""
    recs = np.asarray(recs, np.int64).reshape(-1, 12)
    frames, carries = {}, {}
    for b in range(mel_rows + 2 * len(recs)):
        x, hit = b, None
        for i, rec in enumerate(recs):
            q = _live_clamped(rec, n_slots, wav_cap, mel_rows, n_fft)
            if not q['active']:
                continue
            if x < q['scan_frames'] + 1:
                hit = (i, q)
                break
            x -= q['scan_frames'] + 1
        if hit is None:
            continue
        i, q = hit
        g = int(sess[q['slot']][0]) & 1
        rd, wr = 2 * q['slot'] + g, 2 * q['slot'] + 1 - g
        if x >= q['frames']:
            if x == q['frames'] and q['L'] < 0 and q['clen'] + q['chlen'] > 0:
                keep = q['c0'] + q['clen'] + q['chlen'] - q['c1']
                carries[wr] = (i, rd, q['c1'], max(min(keep, n_fft), 0))
            continue
        if q['flags'] & 4:
            where, row, limit = ('first', q['first_row'], n_first) if x == 0 else ('mel', q['row'] + x - 1, mel_rows)
        else:
            where, row, limit = 'mel', q['row'] + x, mel_rows
        if 0 <= row < limit:
            frames[(where, row)] = (i, q['first'] + x, rd)
    return frames, carries


def live_tick_commit(sess, max_key, scratch, recs, words, limit_db: float, wav_cap: int, mel_rows: int, n_fft: int):
    """(numpy restatement of live_tick_commit_kernel)  (sess, max_key, scratch) after the front-end commit of a live tick: with both sticky
    `words` zero every active record's session flips its generation, advances (a start: sets; an end: zeroes) received and emitted, folds
    the tick's maximum into its word (a start: replaces it), becomes `over` above limit_db and, at an end, has its word put back; with a
    word raised nothing of the sessions changes.  The scratch words are KEY_NONE afterwards either way.  Returns copies."""
    sess, max_key, scratch = np.array(sess, np.int64), np.array(max_key, np.int32), np.array(scratch, np.int32)
    keys, scratch[:] = scratch.copy(), KEY_NONE
    if int(words[0]) != 0 or int(words[1]) != 0:
        return sess, max_key, scratch
    limit = _db_to_key(limit_db)
    for i, rec in enumerate(np.asarray(recs, np.int64).reshape(-1, 12)):
        q = _live_clamped(rec, sess.shape[0], wav_cap, mel_rows, n_fft)
        if not q['active']:
            continue
        s, start = q['slot'], bool(q['flags'] & 2)
        word = int(keys[i]) if start or int(keys[i]) > int(max_key[s]) else int(max_key[s])
        sess[s, 0] ^= 1
        if word > limit:
            sess[s, 3] = 1
        if q['L'] >= 0:
            sess[s, 1], sess[s, 2], word = 0, 0, KEY_NONE
        else:
            sess[s, 1] = (0 if start else sess[s, 1]) + q['chlen']
            sess[s, 2] = (0 if start else sess[s, 2]) + q['frames']
        max_key[s] = word
    return sess, max_key, scratch


def _db_to_key(db: float) -> int:
    """The order-preserving max word of a float (float_key, csrc/pwv_audio.hip)."""
    bits = int(np.array([db], dtype=np.float32).view(np.int32)[0])
    return bits if bits >= 0 else bits ^ 0x7fffffff


class StreamingMel(object):
    """wav chunks in, the frames of `wav_to_mel_device` on the whole utterance out -- bit for bit, as soon as their samples are there:

        fe = StreamingMel(slots=4)
        frames = fe.push([chunk_a, chunk_b], slots=[0, 2])      # [n_i >= 1] float32 on the GPU each -> [f_i, n_mels] each, f_i >= 0
        tail = fe.finish(0)                                     # the frames that had to wait for the utterance's end

    `slots` independent sessions.  A push emits frames K(R before) .. K(R after) - 1 of every session it feeds (frames_ready); finish
    fixes the utterance's length at what was received and emits the rest, 1 + L // hop frames in all.  The pieces are views of one
    packed result and go straight into StreamingVocoder.push_varlen.  push only enqueues.

    NORMALISED mode only (both max_db and min_db set, else ValueError): the one-shot's top_db floor needs the utterance's maximum,
    which a stream does not have yet; after normalisation the floor changes nothing while max - top_db <= min_db.  No floor is applied
    here; every session's largest raw dB is kept on the device, and verify() / finish() raise a PwvError naming top_db for a session
    whose maximum exceeds min_db + top_db: its frames are not the one-shot's.  With the default hparams no wav within [-1, 1] gets
    there (mel_db_bound: 17 dB against 25).

    `signal`: the settings (sr, n_fft, win_length, hop_length, n_mels, max_db, min_db), default hp.signal."""

    def __init__(self, slots: int, signal=None, device=None):
        from . import _lib
        s = hp.signal if signal is None else signal
        get = (lambda k: s.get(k, None)) if hasattr(s, 'get') else (lambda k: getattr(s, k, None))
        if not (get('max_db') and get('min_db')):
            raise ValueError('StreamingMel is the normalised front-end: signal.max_db and signal.min_db must both be set '
                             '(the top_db floor of the raw dB needs the whole utterance)')
        if int(slots) < 1:
            raise ValueError('slots must be >= 1, got %r' % (slots,))
        self.n_slots = int(slots)
        self.sr, self.n_fft, self.win_length = int(get('sr')), int(get('n_fft')), int(get('win_length'))
        self.hop, self.n_mels = int(get('hop_length')), int(get('n_mels'))
        self.max_db, self.min_db = float(get('max_db')), float(get('min_db'))
        if self.n_fft < 2 or self.n_fft % 2 or self.n_fft > 2048 or self.hop < 1 or self.max_db == self.min_db:
            raise ValueError('StreamingMel: n_fft must be even and <= 2048, hop_length >= 1, max_db != min_db')
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self._lib = _lib
        self._window, self._basis = _consts(self.device, _Signal(self.sr, self.n_fft, self.win_length, self.n_mels))
        # two blocks of n_fft floats per slot: a push reads block 2 s + gen and writes block 2 s + 1 - gen
        self._state = torch.zeros((2 * self.n_slots, self.n_fft), dtype=torch.float32, device=self.device)
        self._max = torch.full((self.n_slots,), -(1 << 31), dtype=torch.int32, device=self.device)
        self._gen = [0] * self.n_slots
        self._received = [0] * self.n_slots
        self._emitted = [0] * self.n_slots
        # graph replay of a live tick (graph.GraphedLiveStream): the sessions as the device sees them -- int64 [n_slots, 4] = {generation
        # read, samples received, frames emitted, over the top_db limit} --, per slot what that row is known to hold (None: never written)
        # and the graph whose ticks are in flight
        self._sess = torch.zeros((self.n_slots, 4), dtype=torch.int64, device=self.device)
        self._sess_host = [None] * self.n_slots
        self._live = None

    # -- bookkeeping -----------------------------------------------------------------------------------------------------
    def _slot(self, slot) -> int:
        s = int(slot)
        if not 0 <= s < self.n_slots:
            raise ValueError('slot %r out of range (0 .. %d)' % (slot, self.n_slots - 1))
        return s

    def received(self, slot) -> int:
        """Samples given to `slot` since its last reset."""
        return self._received[self._slot(slot)]

    def emitted(self, slot) -> int:
        """Frames `slot` has returned since its last reset."""
        return self._emitted[self._slot(slot)]

    def state_bytes(self, slot=0) -> int:
        """Bytes of device memory one session holds: two generations of the carry block and the maximum word."""
        self._slot(slot)
        return 2 * self.n_fft * 4 + 4

    def _settled(self, what: str) -> None:
        if self._live is not None:
            raise self._lib.PwvError('StreamingMel.%s: live ticks are in flight (GraphedLiveStream.tick only enqueues, and the sessions '
                                     'are the device\'s meanwhile): call verify() of the live graph first' % what)

    def _note_over(self, slots) -> None:
        """(enqueue-only) The sticky `over` word of the device session table for `slots`, as the commit of a live tick sets it: 1 once the
        session's largest raw dB exceeds min_db + top_db.  The eager form of a live tick calls it behind its pushes."""
        idx = torch.tensor(list(slots), dtype=torch.int64).pin_memory().to(self.device, non_blocking=True)
        over = (self._max.index_select(0, idx) > _db_to_key(self.min_db + TOP_DB)).to(torch.int64)
        self._sess[:, 3].index_copy_(0, idx, torch.maximum(self._sess[:, 3].index_select(0, idx), over))

    def reset(self, slot) -> None:
        """`slot` starts a new utterance (enqueue-only: the carry needs no clearing, its length is zero)."""
        self._settled('reset')
        s = self._slot(slot)
        self._received[s], self._emitted[s] = 0, 0
        self._max[s:s + 1].fill_(-(1 << 31))

    def max_db_seen(self, slot) -> Optional[float]:
        """The largest raw dB of `slot`'s utterance so far (None before its first frame).  Synchronises."""
        return _key_to_db(self._max[self._slot(slot)].item())

    def verify(self, slots=None) -> None:
        """Wait for the pushes so far and raise a PwvError for every session (of `slots`, default all) whose largest raw dB exceeds
        min_db + top_db: the one-shot would have clipped its quiet bands at max - top_db, above min_db, and its frames differ."""
        slots = list(range(self.n_slots)) if slots is None else [self._slot(v) for v in slots]
        keys = self._max.cpu().tolist()
        limit = self.min_db + TOP_DB
        over = [(s, _key_to_db(keys[s])) for s in slots if _key_to_db(keys[s]) is not None and _key_to_db(keys[s]) > limit]
        if over:
            raise self._lib.PwvError('StreamingMel: the top_db floor of the one-shot front-end would have been active for slot(s) %s: largest raw dB %s '
                                     '> min_db + top_db = %g; their frames are not the one-shot\'s (compute those utterances with wav_to_mel_device)'
                                     % ([s for s, _ in over], ['%.2f' % v for _, v in over], limit))

    # -- a push ----------------------------------------------------------------------------------------------------------
    def _launch(self, slots, chunks, finishing: bool):
        """One ragged launch: slots[i] receives chunks[i] (finishing: nothing, and its utterance ends).  Returns the frame pieces."""
        from . import engine
        lib = self._lib
        recs, off, row = [], 0, 0
        after = []
        for s, chunk in zip(slots, chunks):
            n = 0 if finishing else int(chunk.shape[0])
            r0, k0 = self._received[s], self._emitted[s]
            r1 = r0 + n
            k1 = 1 + r1 // self.hop if finishing else frames_ready(r1, self.n_fft, self.hop)
            c0 = carry_start(r0, self.n_fft, self.hop)
            c1 = c0 if finishing else carry_start(r1, self.n_fft, self.hop)
            frames = max(k1 - k0, 0)
            recs.append([c0, r0 - c0, off, n, k0, frames, r1 if finishing else -1, 2 * s + self._gen[s], 2 * s + 1 - self._gen[s], row, c1, s])
            after.append((s, r1, k0 + frames, row, frames))
            off, row = off + n, row + frames
        assert all(len(r) == lib.MEL_STREAM_REC for r in recs)
        wav = None if finishing else (chunks[0] if len(chunks) == 1 else torch.cat(chunks))
        mel = torch.empty((row, self.n_mels), dtype=torch.float32, device=self.device)
        rec_host = torch.tensor(recs, dtype=torch.int64).pin_memory()
        rec = rec_host.to(self.device, non_blocking=True)
        a = lib.MelStreamArgs()
        a.wav, a.wav_len = (None, 0) if wav is None else (wav.data_ptr(), off)
        a.window, a.mel_basis = self._window.data_ptr(), self._basis.data_ptr()
        a.mel, a.mel_rows = (mel.data_ptr() if row else None), row
        a.state, a.max_key = self._state.data_ptr(), self._max.data_ptr()
        a.rec, a.rec_host = rec.data_ptr(), rec_host.data_ptr()
        a.N, a.n_fft, a.hop, a.n_mels = len(slots), self.n_fft, self.hop, self.n_mels
        a.n_blocks, a.n_words = 2 * self.n_slots, self.n_slots
        a.amin, a.max_db, a.min_db = AMIN, self.max_db, self.min_db
        lib.check(lib.lib().pwv_wav_to_mel_db_stream_f32(ctypes.byref(a), engine._stream()), 'pwv_wav_to_mel_db_stream_f32')
        out = []
        for s, r1, k1, first, frames in after:       # the launch is enqueued: the sessions advance (stream order keeps the generations apart)
            self._received[s], self._emitted[s] = r1, k1
            self._gen[s] ^= 1
            out.append(mel[first:first + frames])
        return out

    def push(self, chunks, slots=None):
        """Session slots[i] (default: all slots, in order) receives its next samples chunks[i], [n_i >= 1] float32 on the GPU.  Returns
        the list of [f_i, n_mels] frame tensors that became ready (f_i may be 0), views of one packed result.  Enqueue-only."""
        from . import engine
        self._settled('push')
        if not isinstance(chunks, (list, tuple)) or not chunks:
            raise ValueError('chunks must be a non-empty list of [n] tensors')
        slots = list(range(self.n_slots)) if slots is None else [self._slot(v) for v in slots]
        if len(slots) != len(chunks) or len(set(slots)) != len(slots):
            raise ValueError('slots must be distinct, one per chunk (%d chunks), got %r' % (len(chunks), slots))
        for i, c in enumerate(chunks):
            if not hasattr(c, 'dim') or c.dim() != 1 or c.shape[0] < 1:
                raise ValueError('chunks[%d] must be [n >= 1], got %s' % (i, tuple(getattr(c, 'shape', ()))))
        chunks = [engine._require_cuda_f32(c, 'chunks[%d]' % i) for i, c in enumerate(chunks)]
        return self._launch(slots, chunks, False)

    def finish(self, slot):
        """The utterance of `slot` ends at the samples received, L: returns its last frames (1 + L // hop in all with those returned
        before), the right reflection taken at L.  L <= n_fft / 2 is refused, as by the one-shot.  Verifies the slot (synchronises): a
        PwvError naming top_db if its frames are not the one-shot's.  The slot is fresh afterwards, as after reset."""
        self._settled('finish')
        s = self._slot(slot)
        out = self._launch([s], [None], True)[0]
        try:
            self.verify([s])
        finally:
            self.reset(s)
        return out


class _Signal(object):
    """The signal settings the device constants depend on."""

    def __init__(self, sr, n_fft, win_length, n_mels):
        self.sr, self.n_fft, self.win_length, self.n_mels = sr, n_fft, win_length, n_mels


def load_wav_fixed(path: str, length: int) -> np.ndarray:
    """data_load.py:42-50 at generation time: read, trim, first chunk, zero-pad to exactly `length` samples."""
    wav = trim_wav(read_wav(path, hp.signal.sr))
    return fix_length(wav[:length], length).astype(np.float32)


def wav_to_normalized_mel(path: str, length: int):
    """data_load.py:37-56 at generation time (first chunk): returns (wav [length], mel [1 + length/hop, n_mels])."""
    s = hp.signal
    wav = trim_wav(read_wav(path, s.sr))
    wav = fix_length(wav[:length], length)
    mel = wav2melspec_db(wav, s.sr, s.n_fft, s.win_length, s.hop_length, s.n_mels, max_db=s.max_db, min_db=s.min_db)
    return wav.astype(np.float32), mel
