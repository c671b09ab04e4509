"""generate(case, ckpt, debug): mel-spectrogram -> waveform with the IAF-WaveNet student.

Counterpart of /root/reference/generate.py:16-78 with the same arguments.  Differences that
follow from the platform, not from the math:
  * no TF graph/session: the forward is one call of IAFVocoder on the GPU (the reference's single
    sess.run, generate.py:68);
  * the checkpoint is read by variable NAME (EMA shadows preferred when hp.train.use_ema,
    generate.py:55-66) from a TensorFlow V2 checkpoint (tf_checkpoint.py, no TF needed) or an
    .npz of TF-named arrays; with no checkpoint the model runs with random init exactly like
    the reference ("No checkpoint found", generate.py:65-66);
  * the result is written as .wav / .npy files into hp.logdir (the reference only writes
    TensorBoard audio summaries, generate.py:71-73);
  * `data_path: 'synthetic'` (bench cases) or a glob of .npy mel files replaces the wav dataset;
    wav input uses the torch STFT front-end in audio_frontend.py.
CLI (python-fire style, fire itself is not installed):  python -m pwv_amd.generate <case> [--ckpt=..] [--debug] [--varlen [--seed=S]] [--stream=FRAMES [--graph | --live]] [--score]
"""
from __future__ import absolute_import, division, print_function

import glob
import os
import sys

import numpy as np
import torch

from . import _lib
from .hparam import hparam as hp
from .models import IAFVocoder
from .variables import reset_default_store


def _latest_checkpoint(logdir):
    """tf.train.latest_checkpoint: the TF V2 checkpoint named by <logdir>/checkpoint (or the newest
    *.index), else the newest .npz of TF-named arrays."""
    from .tf_checkpoint import latest_checkpoint
    tf_ck = latest_checkpoint(logdir)
    if tf_ck:
        return tf_ck
    cands = sorted(glob.glob(os.path.join(logdir, '*.npz')), key=os.path.getmtime)
    return cands[-1] if cands else None


def _load_mels(data_path, batch_size, length, device, info=None):
    """(gt_wav or None, melspec[N, t_mel, n_mels]) for the first `batch_size` items.  `info`, a dict, receives 'files': the name of
    every item's input."""
    hop, n_mels = hp.signal.hop_length, hp.signal.n_mels
    t_mel = 1 + length // hop
    info = {} if info is None else info
    if data_path == 'synthetic':
        info['files'] = ['synthetic:%d' % i for i in range(batch_size)]
        g = torch.Generator().manual_seed(0)
        return None, (torch.rand((batch_size, t_mel, n_mels), generator=g) * 2 - 1).to(device)
    files = sorted(glob.glob(data_path))
    if not files:
        raise FileNotFoundError('no input files match data_path %r (use data_path: synthetic for seeded noise mel)' % data_path)
    # like data_load.py:22-25: the last (1 - dataset_ratio) share of the files is the generation split
    split = int(len(files) * hp.train.dataset_ratio)
    files = (files[split:] or files)[:batch_size]
    print('dataset size is {}'.format(len(files)))
    info['files'] = (files + [files[-1]] * batch_size)[:batch_size]
    if all(not f.endswith('.npy') for f in files):
        # wav input: host reads / trims / pads (data_load.py:42-50), then the spectrogram is computed ON THE DEVICE
        # (audio_frontend.wav_to_mel_device) -- the mel never visits the host between the front-end and the network
        from .audio_frontend import load_wav_fixed, wav_to_mel_device
        wavs = [load_wav_fixed(f, length) for f in files]
        while len(wavs) < batch_size:
            wavs.append(wavs[-1])
        gt = np.stack(wavs)
        return gt[..., None], wav_to_mel_device(torch.from_numpy(gt).to(device))
    mels, wavs = [], []
    for f in files:
        if f.endswith('.npy'):
            m = np.load(f).astype(np.float32)
        else:
            from .audio_frontend import wav_to_normalized_mel
            wav, m = wav_to_normalized_mel(f, length)
            wavs.append(wav)
        if m.shape[0] < t_mel:
            m = np.pad(m, [(0, t_mel - m.shape[0]), (0, 0)])
        mels.append(m[:t_mel])
    while len(mels) < batch_size:
        mels.append(mels[-1])
        if wavs:
            wavs.append(wavs[-1])
    gt = np.stack(wavs)[..., None] if wavs else None
    return gt, torch.from_numpy(np.stack(mels)).to(device)


def forward_over_ranks(mel, batch_size, length, device, make_model, noise_window, n_mels, hop, halo, group=None, allow_time_shards=True):
    """The forward of a job started with one process per GPU (WORLD_SIZE > 1; the reference is single-device,
    generate.py:47-49).  Rank 0 passes all mels [batch_size, t_mel, n_mels]; it gets all waveforms [batch_size, length, 1]
    back (other ranks: None).  Utterances shard across the ranks (distributed.generate_sharded); a batch smaller than the
    world shards in TIME instead, exactly (distributed.generate_time_sharded_ranks, halo = timeshard.chain_halo).  Every
    rank draws its share of ONE logistic-noise stream -- utterance i, sample t is counter i * length + t -- so the result
    does not depend on how the job was cut.  allow_time_shards=False (a model with a time-global normaliser, for which
    overlap-and-discard is not exact) keeps a small batch on utterance shards: ranks beyond the batch idle.
      make_model(n, window) -> callable(mel [n, 1 + window/hop, n_mels], z [n, window, 1]) -> [n, window, 1]
      noise_window(n, first_sample, window, first_item) -> z [n, window, 1]"""
    import torch.distributed as dist
    from .distributed import generate_sharded, generate_time_sharded_ranks, shard_bounds
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    models = {}

    def model_for(n, window):
        if (n, window) not in models:
            models[(n, window)] = make_model(n, window)
        return models[(n, window)]

    if batch_size >= world or not allow_time_shards:
        lo, _ = shard_bounds(batch_size, world, rank)
        return generate_sharded(lambda m, zz: model_for(m.shape[0], length)(m, noise_window(m.shape[0], 0, length, lo)),
                                mel, (1 + length // hop, n_mels), length, device, group=group)
    return generate_time_sharded_ranks(lambda m, zz, t0: model_for(m.shape[0], (m.shape[1] - 1) * hop)(m, noise_window(m.shape[0], t0, (m.shape[1] - 1) * hop, 0)),
                                       mel, n_mels, length, hop, halo, device, group=group)


def _load_mels_varlen(data_path, batch_size, device, info=None):
    """--varlen: one [t_mel_i, n_mels] mel per input at the input's OWN length -- a .npy mel as stored (at least 2 frames), a wav
    trimmed (data_load.py:42-44) and cut down to a multiple of hop_length, its mel computed on the device.  'synthetic' has no lengths
    of its own: every utterance is generate.length long.  `info`, a dict, receives 'files' and 'wavs': per input its name and the
    trimmed wav its mel was computed from (None for a mel that was given)."""
    hop = hp.signal.hop_length
    info = {} if info is None else info
    if data_path == 'synthetic':
        mels = list(_load_mels(data_path, batch_size, hp.generate.length, device, info)[1].unbind(0))
        info['wavs'] = [None] * len(mels)
        return mels
    files = sorted(glob.glob(data_path))
    if not files:
        raise FileNotFoundError('no input files match data_path %r (use data_path: synthetic for seeded noise mel)' % data_path)
    split = int(len(files) * hp.train.dataset_ratio)
    files = (files[split:] or files)[:batch_size]
    mels, wavs = [], []
    info['files'], info['wavs'] = files, wavs
    for f in files:
        if f.endswith('.npy'):
            m = np.load(f).astype(np.float32)
            if m.ndim != 2 or m.shape[0] < 2:
                raise ValueError('%s: a mel needs at least 2 frames, got shape %s' % (f, m.shape))
            mels.append(torch.from_numpy(m).to(device))
            wavs.append(None)
        else:
            from .audio_frontend import read_wav, trim_wav, wav_to_mel_device
            wav = trim_wav(read_wav(f, hp.signal.sr))
            wav = wav[:len(wav) // hop * hop].astype(np.float32)
            if len(wav) == 0:
                raise ValueError('%s: shorter than one hop (%d samples) after trimming' % (f, hop))
            mels.append(wav_to_mel_device(torch.from_numpy(wav[None]).to(device))[0])
            wavs.append(wav)
    print('dataset size is {}'.format(len(mels)))
    return mels


def _score_outputs(pred, gt_wavs, mels, files, logdir, device):
    """--score: the forward's result against what went in, on the device (score.py), under the reference's names.
      pred      [N, L, 1] (tensor or array), or a list of [len_i, 1]
      gt_wavs   the ground-truth wavs laid out as `pred` ([N, L, 1] / a list of [len_i]; None entries allowed in a list), or None
      mels      the input mels ([N, t_mel, n_mels] or a list of [t_mel_i, n_mels]); None: computed from the ground truth
    Prints loss/likelihood, loss/power and loss/total of the batch and writes scores.json into `logdir`: those three, weight_power_loss,
    and per input file, samples, l1, frames, power and mel_l1 -- the L1 between the mel of the prediction (the device front-end) and the
    input mel.  l1 and power are null where an input has no ground-truth wav; the batch numbers cover the inputs that have one.  mel_l1 is
    null only for a prediction too short for the front-end (n_fft / 2 samples or fewer).  Returns the dict it wrote."""
    import json
    from . import score as S
    from .audio_frontend import wav_to_mel_device

    def dev(a):
        return (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))).to(device)

    uniform = not isinstance(pred, (list, tuple))
    preds = [p.reshape(-1, 1) for p in (dev(pred).unbind(0) if uniform else [dev(p) for p in pred])]
    n = len(preds)
    gts = [None] * n if gt_wavs is None else [None if g is None else dev(g).reshape(-1, 1) for g in gt_wavs]
    mels = [None] * n if mels is None else list(mels.unbind(0) if isinstance(mels, torch.Tensor) else mels)
    half = int(hp.signal.n_fft) // 2
    for i in range(n):
        if mels[i] is None and gts[i] is not None and gts[i].shape[0] > half:
            mels[i] = wav_to_mel_device(gts[i].reshape(1, -1))[0]

    def clean(v):
        v = float(v)
        return v if np.isfinite(v) else None

    have = [i for i in range(n) if gts[i] is not None]
    per = [dict(file=files[i] if files else None, samples=int(preds[i].shape[0]), l1=None, frames=0, power=None, mel_l1=None) for i in range(n)]
    weight = float(hp.train.weight_power_loss)
    batch = dict(likelihood=None, power=None, total=None)
    if have:
        if uniform and len(have) == n:
            s = S.score(torch.stack(preds), torch.stack(gts))
        else:
            s = S.score_varlen([preds[i] for i in have], [gts[i] for i in have])
        l1, power, frames = s.l1, s.power, s.frames
        for k, i in enumerate(have):
            per[i].update(l1=clean(l1[k]), power=clean(power[k]), frames=int(frames[k]))
        batch = dict(likelihood=clean(s.likelihood), power=clean(s.power_loss), total=clean(s.total(weight)))
    able = [i for i in range(n) if mels[i] is not None and preds[i].shape[0] > half]
    if able:
        pred_mels = [wav_to_mel_device(preds[i].reshape(1, -1))[0] for i in able]
        m = S.mel_l1(pred_mels, [mels[i].to(device).float() for i in able]).l1
        for k, i in enumerate(able):
            per[i]['mel_l1'] = clean(m[k])
    out = {'loss/likelihood': batch['likelihood'], 'loss/power': batch['power'], 'loss/total': batch['total'], 'weight_power_loss': weight,
           'win_length': int(hp.signal.win_length), 'hop_length': int(hp.signal.hop_length), 'inputs': per}
    for name in ('loss/likelihood', 'loss/power', 'loss/total'):
        print('%s: %s' % (name, 'n/a (no ground-truth wav)' if out[name] is None else '%.6g' % out[name]))
    try:
        os.makedirs(logdir, exist_ok=True)
        with open(os.path.join(logdir, 'scores.json'), 'w') as f:
            json.dump(out, f, indent=1)
    except OSError as e:
        print('could not write scores.json to %s: %s' % (logdir, e))
    return out


def generate(case='default', ckpt=None, debug=False, varlen=False, seed=None, stream=None, graph=False, live=False, score=False):
    '''
    :param case: experiment case name
    :param ckpt: checkpoint to load model
    :param debug: print per-stage timing (the reference hooks tfdbg here).
    :param varlen: vocode every input at its own length in ONE packed forward (IAFVocoder.generate_varlen) instead of every
        utterance at hp.generate.length; writes pred_i.wav at each length.
    :param seed: (with varlen) every utterance draws its noise from stream `seed` at counter 0, so a file's audio depends only on
        its mel and the seed -- not on the other files of the run or their order.
    :param stream: vocode every input at its own length as a STREAM (IAFVocoder.open_stream): one session per input, fed in pushes
        of `stream` mel frames; writes the files --varlen writes.  A case with cond_upsample_method 'transposed_conv' streams too (on
        per-layer launches; --graph and --live=graph are refused for it by name), and so does a case with use_skip_connection.
    :param graph: (with stream) every tick is one replay of a captured ragged tick (StreamingVocoder.graphed_varlen at a capacity of one
        slot per input and inputs x `stream` frames), the first one included: it starts the sessions (tick(starts=)); only an input too
        short for that starts with the eager one-frame push; same files.
    :param live: (with stream, wav inputs) the front-end streams too: every tick gives each unfinished input its next `stream` x hop
        SAMPLES through audio_frontend.StreamingMel, and the frames that became ready to the sessions; same files.  --live=graph:
        every such tick is one replay of a captured live tick (StreamingVocoder.graphed_live).
    :param score: (every mode) after the forward, score the result on the device against the ground-truth wavs and the input mels
        (_score_outputs): prints loss/likelihood, loss/power and loss/total and writes scores.json next to the waveforms.
    '''
    if live and (stream is None or graph or live not in (True, 'graph')):
        raise ValueError('--live (or --live=graph) applies to --stream=FRAMES without --graph (wav chunks in, wav chunks out)')
    if graph and stream is None:
        raise ValueError('--graph applies to --stream=FRAMES (graph replay of the ragged ticks)')
    if stream is not None:
        stream = int(stream)
        if stream < 1:
            raise ValueError('--stream must be a number of frames >= 1, got %d' % stream)
        if varlen or seed is not None:
            raise ValueError('--stream excludes --varlen / --seed')
    if seed is not None:
        if not varlen:
            raise ValueError('--seed applies to --varlen (one noise stream per utterance)')
        seed = int(seed)
        if not 0 <= seed < (1 << 64):
            raise ValueError('--seed must be in [0, 2**64), got %d' % seed)
    hp.set_hparam_yaml(case)
    if stream is not None and hp.model.use_skip_connection and (graph or live == 'graph'):
        raise _lib.PwvError('--graph / --live=graph: skip accumulation (use_skip_connection) streams on per-layer launches only; a graphed '
                            'tick needs the whole-flow persistent launch (use --stream=FRAMES or --stream=FRAMES --live)')
    if stream is not None and hp.model.cond_upsample_method == 'transposed_conv' and (graph or live == 'graph'):
        raise _lib.PwvError('--graph / --live=graph: per-sample (transposed-conv) conditioning streams on per-layer launches only; a graphed '
                            'tick needs the whole-flow persistent launch (use --stream=FRAMES or --stream=FRAMES --live)')
    live_files = _live_inputs(hp.data_path, hp.generate.batch_size) if live else None
    if not torch.cuda.is_available():
        raise RuntimeError('generate() needs an MI355X: the HIP path has no CPU fallback')
    if int(os.environ.get('WORLD_SIZE', '1')) > 1:
        torch.cuda.set_device(int(os.environ.get('LOCAL_RANK', '0')))       # one process per GPU
    device = torch.device('cuda', torch.cuda.current_device())
    logdir = os.environ.get('PWV_LOGDIR', hp.logdir)

    store = reset_default_store(device=device)              # fresh "graph"
    batch_size, length = hp.generate.batch_size, hp.generate.length
    world, rank = int(os.environ.get('WORLD_SIZE', '1')), int(os.environ.get('RANK', '0'))
    if world > 1:
        if varlen or stream:
            raise ValueError('--varlen / --stream run on one GPU (a packed batch or a set of sessions is not sharded over ranks)')
        # one process per GPU (torchrun): utterances -- or, for a batch smaller than the world, time slices -- shard over
        # the ranks; rank 0 reads the inputs and writes the outputs
        return _generate_over_ranks(store, batch_size, length, device, logdir, ckpt, debug, score)
    info = {}                  # what --score needs of the inputs: their names and, where they are audio, the trimmed wavs
    if live:
        gt_wav, melspec, wavs = None, None, _load_wavs_live(live_files)
        info.update(files=live_files, wavs=wavs)
        batch_size, length = 1, sum(len(w) for w in wavs)
    elif varlen or stream:
        gt_wav, melspec = None, _load_mels_varlen(hp.data_path, batch_size, device, info)
        batch_size, length = 1, sum(int(m.shape[0] - 1) * hp.signal.hop_length for m in melspec)     # (the timing line: all samples)
    else:
        gt_wav, melspec = _load_mels(hp.data_path, batch_size, length, device, info)

    model = IAFVocoder(batch_size=batch_size, length=length, store=store)

    # load model
    ckpt = '{}/{}'.format(logdir, ckpt) if ckpt else (_latest_checkpoint(logdir) if os.path.isdir(logdir) else None)
    if ckpt:
        n = store.load_checkpoint(ckpt, use_ema=bool(hp.train.use_ema))
    else:
        print('No checkpoint found at {}.'.format(logdir))

    if debug:
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    # feed forward (generate.py:68).  The call returns a verified result: a persistent launch that gave up is rerun on per-layer
    # launches, a forward that left the range of the split-fp16 arithmetic in exact fp32 -- on the same noise
    # (engine.verified_call); what comes back is what the reference's fp32 sess.run would have produced, or an exception.
    # verify=True is EXPLICIT: it outranks PWV_ASYNC=1 (whose default is enqueue-only) -- nothing unverified is written to disk
    if live:
        pred = (_generate_stream_live_graph if live == 'graph' else _generate_stream_live)(model, wavs, stream, device)
    elif stream:
        pred = _generate_stream_graph(model, melspec, stream) if graph else _generate_stream(model, melspec, stream)
    elif varlen:
        pred = model.generate_varlen(melspec, verify=True, seeds=None if seed is None else [seed] * len(melspec))
    else:
        pred = model(gt_wav, melspec, is_training=False, verify=True)
    if ckpt:
        # tf.train.Saver.restore fails on a variable the checkpoint lacks (generate.py:59-63); here variables are
        # created lazily by the forward, so the coverage check comes after it
        missing = store.not_restored()
        if missing:
            raise KeyError('checkpoint %s does not hold %d of the model\'s %d variables (they would be random-initialised): %s%s'
                           % (ckpt, len(missing), len(store.vars), ', '.join(missing[:6]), ' ...' if len(missing) > 6 else ''))
        no_shadow = store.ema_missing() if hp.train.use_ema else []
        if no_shadow:
            # with use_ema the reference restores EVERY trainable variable of 'iaf_vocoder' from its shadow (generate.py:59-63);
            # a checkpoint without one fails there, it does not fall back to the raw variable
            raise KeyError('checkpoint %s has no ExponentialMovingAverage shadow for %d model variable(s) although train.use_ema is '
                           'set: %s%s' % (ckpt, len(no_shadow), ', '.join(no_shadow[:6]), ' ...' if len(no_shadow) > 6 else ''))
        print('Successfully loaded checkpoint {} ({} variables)'.format(ckpt, n))
    if debug:
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        print('forward: %.2f ms, %.3g samples/s (first call includes weight packing)' % (ms, batch_size * length / ms * 1e3))
    if varlen or stream:
        pred_wav = [p.cpu().numpy() for p in pred]
        _write_outputs_varlen(pred_wav, logdir)
        if score:
            _score_outputs(list(pred), info.get('wavs'), melspec, info.get('files'), logdir, device)
        print('Done.')
        return pred_wav
    pred_wav = pred.cpu().numpy()
    _write_outputs(pred_wav, logdir)
    if score:
        _score_outputs(pred, gt_wav, melspec, info.get('files'), logdir, device)
    print('Done.')
    return pred_wav


def _open_stream(model, slots):
    """The stream of --stream: a case with model.cond_upsample_method 'transposed_conv' makes the request for its streaming form
    (IAFVocoder.open_stream(transposed_conv=True)), a case with model.use_skip_connection for its own (use_skip_connection=True), as the
    train command line asks for skip / shared."""
    return model.open_stream(slots=slots, transposed_conv=hp.model.cond_upsample_method == 'transposed_conv',
                             use_skip_connection=bool(hp.model.use_skip_connection))


def _generate_stream(model, mels, frames):
    """--stream: input i is session i of one StreamingVocoder; every tick gives each unfinished session its next `frames` frames (the
    rest at its end) in ONE ragged push (push_varlen: fresh and running sessions and short last chunks share the launch; verify=True:
    explicit, as above).  Returns the [len_i, 1] waveforms."""
    s = _open_stream(model, len(mels))
    pos, outs = [0] * len(mels), [[] for _ in mels]
    while any(p < m.shape[0] for p, m in zip(pos, mels)):
        slots = [i for i, m in enumerate(mels) if pos[i] < m.shape[0]]
        counts = [min(frames, mels[i].shape[0] - pos[i]) for i in slots]
        got = s.push_varlen([mels[i][pos[i]:pos[i] + f] for i, f in zip(slots, counts)], slots=slots, verify=True)
        for k, (i, f) in enumerate(zip(slots, counts)):
            outs[i].append(got[k])
            pos[i] += f
    return [torch.cat(o) for o in outs]


def _live_inputs(data_path, batch_size):
    """--stream --live: the files _load_mels_varlen would read.  Inputs that are no audio (.npy mels, 'synthetic') have nothing to stream
    a front-end over: ValueError."""
    files = [] if data_path == 'synthetic' else sorted(glob.glob(data_path))
    if data_path != 'synthetic' and not files:
        raise FileNotFoundError('no input files match data_path %r' % data_path)
    split = int(len(files) * hp.train.dataset_ratio)
    files = (files[split:] or files)[:batch_size]
    if not files or any(f.endswith('.npy') for f in files):
        raise ValueError('--live streams the mel front-end over wav inputs: data_path %r holds %s' % (data_path, '.npy mels' if files else 'no audio'))
    return files


def _load_wavs_live(files):
    """--stream --live: the inputs as SAMPLES -- every wav trimmed (data_load.py:42-44) and cut down to a multiple of hop_length, as
    _load_mels_varlen cuts it."""
    from .audio_frontend import read_wav, trim_wav
    hop = hp.signal.hop_length
    wavs = []
    for f in files:
        wav = trim_wav(read_wav(f, hp.signal.sr))
        wav = wav[:len(wav) // hop * hop].astype(np.float32)
        if len(wav) == 0:
            raise ValueError('%s: shorter than one hop (%d samples) after trimming' % (f, hop))
        wavs.append(wav)
    print('dataset size is {}'.format(len(wavs)))
    return wavs


def _generate_stream_live(model, wavs, frames, device):
    """--stream=FRAMES --live: input i is session i of one StreamingMel and of one StreamingVocoder.  Every tick gives each unfinished
    input its next frames x hop samples in ONE ragged front-end push; an input whose samples are used up is finished in the same tick
    (its last frames, the right reflection at its length); the frames of the tick go to the sessions in ONE push_varlen (verify=True, as
    _generate_stream).  A session with no frame yet -- the front-end emits its first frame after n_fft / 2 + 1 samples -- sits the tick
    out.  Returns the [len_i, 1] waveforms: 1 + len_i / hop frames each, so len_i samples, as --varlen."""
    from .audio_frontend import StreamingMel
    n, step = len(wavs), frames * int(hp.signal.hop_length)
    fe, s = StreamingMel(n, device=device), _open_stream(model, n)
    wavs = [torch.from_numpy(w).to(device) for w in wavs]
    pos, done, outs = [0] * n, [False] * n, [[] for _ in wavs]
    while not all(done):
        feed = [i for i in range(n) if pos[i] < wavs[i].shape[0]]
        ready = dict(zip(feed, fe.push([wavs[i][pos[i]:pos[i] + step] for i in feed], slots=feed)))
        for i in feed:
            pos[i] += step
            if pos[i] >= wavs[i].shape[0]:
                ready[i], done[i] = torch.cat([ready[i], fe.finish(i)]), True
        slots = [i for i in feed if ready[i].shape[0]]
        if slots:
            got = s.push_varlen([ready[i] for i in slots], slots=slots, verify=True)
            for k, i in enumerate(slots):
                outs[i].append(got[k])
    return [torch.cat(o) for o in outs]


def _generate_stream_live_graph(model, wavs, frames, device, depth=4):
    """--stream=FRAMES --live=graph: the loop of _generate_stream_live on graphed live ticks (graph.GraphedLiveStream at a capacity of
    one slot per input and, per input, `frames` frames and those its end adds): an input's first tick names it in `starts` (its seed
    drawn here, in input order), its last one in `ends`, with the last chunk.  The ticks only enqueue; one verify() every `depth` ticks.  Where it reports refused
    ticks both halves of every session stand behind the committed ones: the inputs go back to where the first refused tick found them,
    that tick runs as the verified eager sequence (fe.push / fe.finish / push_varlen(verify=True), which reruns it as --live would), and
    the ticks go on from there.  A tick that does not fit the capture runs eagerly inside tick()."""
    from . import _lib, engine
    from .audio_frontend import StreamingMel
    from .graph import packed_filler_rows
    hop = int(hp.signal.hop_length)
    n, step = len(wavs), frames * hop
    # one slot more than inputs, for the filler of a tick of all inputs; per input the frames of a chunk and those an end adds to them
    fe, s = StreamingMel(n + 1, device=device), _open_stream(model, n + 1)
    seeds = [engine.os_seed() for _ in wavs]
    tail = (int(hp.signal.n_fft) // 2 // hop + 1) * hop
    live = s.graphed_live(fe, n, n * (step + tail) + packed_filler_rows(hop), sample=True, depth=depth)
    wavs = [torch.from_numpy(w).to(device) for w in wavs]
    pos, outs = [0] * n, [[] for _ in wavs]
    window = []                # the inputs fed by every tick enqueued since the last verify()

    def plan():
        feed = [i for i in range(n) if pos[i] < wavs[i].shape[0]]
        return (feed, [wavs[i][pos[i]:pos[i] + step] for i in feed], {i: seeds[i] for i in feed if pos[i] == 0},
                [i for i in feed if pos[i] + step >= wavs[i].shape[0]])

    def advance(feed, got, clone):
        for k, i in enumerate(feed):
            outs[i].append(got[k].clone() if clone else got[k])      # (a view of the graph's output buffer: the next tick overwrites it)
            pos[i] += step

    def eager_tick():
        feed, chunks, starts, ends = plan()
        began = {i: i not in starts and fe.emitted(i) > 0 for i in feed}
        for i in starts:
            fe.reset(i)
        ready = dict(zip(feed, fe.push(chunks, slots=feed)))
        for i in ends:
            ready[i] = torch.cat([ready[i], fe.finish(i)])
        slots = [i for i in feed if ready[i].shape[0]]
        for i in slots:
            if not began[i]:
                s.reset(i, seeds[i])
        got = dict(zip(slots, s.push_varlen([ready[i] for i in slots], slots=slots, verify=True))) if slots else {}
        advance(feed, [got.get(i, torch.empty((0, 1), dtype=torch.float32, device=device)) for i in feed], False)

    def refused(e):
        """The ticks behind the committed prefix are taken back; the first of them runs eagerly, verified."""
        if not hasattr(e, 'committed') or e.committed >= len(window):
            raise e
        for feed in reversed(window[e.committed:]):
            for i in feed:
                pos[i] -= step
                outs[i].pop()
        del window[:]
        eager_tick()

    while True:
        busy = any(pos[i] < wavs[i].shape[0] for i in range(n))
        if not busy and not window:
            break
        try:
            if busy:
                feed, chunks, starts, ends = plan()
                got = live.tick(chunks, feed, starts=starts, ends=ends)          # (settles what is in flight itself where it runs eagerly)
                advance(feed, got, True)
                window.append(feed)
            if window and (not busy or len(window) >= depth):
                live.verify()
                del window[:]
        except _lib.PwvError as e:
            refused(e)
    return [torch.cat(o) for o in outs]


def _generate_stream_graph(model, mels, frames, depth=4):
    """--stream=FRAMES --graph: the sessions of _generate_stream advanced by graphed ragged ticks (graph.GraphedRaggedStream at a capacity
    of len(mels) slots and len(mels) * frames frames: a tick of all sessions at `frames` frames fills it, a tick with sessions that have
    ended is filled up by filler sessions, and one that does not fit -- short last chunks in every slot -- runs eagerly inside tick()).
    A session's first tick STARTS it (tick(starts=): its first frame and its next `frames` frames, the samples of the latter); only an
    input whose first chunk has fewer than min_frames + 1 frames starts with the eager one-frame push (its frame is kept: nothing to generate yet).  The
    seeds are drawn here, one per input in input order, as the first push of _generate_stream draws them.  The ticks only enqueue; one
    verify() every `depth` ticks.  Where verify() reports refused ticks (a chunk outside the range of the split-fp16 arithmetic, a
    persistent launch that gave up) the sessions stand behind the committed ones: the first refused tick is pushed again with the
    verified eager push_varlen -- which reruns it as the plain --stream would -- and the ticks go on from there."""
    from . import _lib, engine
    n, hop = len(mels), int(hp.signal.hop_length)
    s = _open_stream(model, n)
    seeds = [engine.os_seed() for _ in mels]
    g = s.graphed_varlen(n, n * frames * hop, sample=True, depth=depth)
    short = [i for i, m in enumerate(mels) if min(frames, m.shape[0] - 1) < g.min_frames]          # (no start a graphed tick takes)
    pos, outs = [0] * n, [[] for _ in mels]
    if short:
        first = s.push_varlen([mels[i][:1] for i in short], slots=short, seeds=[seeds[i] for i in short], verify=True)
        for k, i in enumerate(short):
            pos[i], outs[i] = 1, [first[k]]
    window = []                # the ticks enqueued since the last verify(): (slots, counts, the slots the tick started)

    def chunk(slots, counts):
        """The frames of a tick and the slots it starts: a session that has been given nothing yet brings its first frame too."""
        return ([mels[i][pos[i]:pos[i] + f + (1 if pos[i] == 0 else 0)] for i, f in zip(slots, counts)],
                {i: seeds[i] for i in slots if pos[i] == 0})

    def advance(slots, counts, got, clone):
        for k, (i, f) in enumerate(zip(slots, counts)):
            outs[i].append(got[k].clone() if clone else got[k])      # (a view of the graph's output buffer: the next tick overwrites it)
            pos[i] += f + (1 if pos[i] == 0 else 0)

    def settle():
        try:
            g.verify()
        except _lib.PwvError as e:
            if not hasattr(e, 'committed'):
                raise
            for slots, counts, started in window[e.committed:]:        # what the refused ticks returned is not the sessions' audio
                for i, f in zip(slots, counts):
                    pos[i] -= f + (1 if i in started else 0)
                    outs[i].pop()
            slots, counts, _ = window[e.committed]
            given, starts = chunk(slots, counts)
            for i, seed in starts.items():
                s.reset(i, seed)
            advance(slots, counts, s.push_varlen(given, slots=slots, verify=True), False)
        del window[:]

    while any(p < m.shape[0] for p, m in zip(pos, mels)):
        slots = [i for i, m in enumerate(mels) if pos[i] < m.shape[0]]
        counts = [min(frames, mels[i].shape[0] - max(pos[i], 1)) for i in slots]          # (the samples' frames: a first frame brings none)
        if window and (not g.fits(counts) or engine.persist_suspended()):
            settle()                                 # (tick() would settle them itself, and raise from there)
            continue
        given, starts = chunk(slots, counts)
        advance(slots, counts, g.tick(given, slots, starts=starts or None), True)
        window.append((slots, counts, set(starts)))
        if len(window) >= depth:
            settle()
    if window:
        settle()
    return [torch.cat(o) for o in outs]


def _write_outputs(pred_wav, logdir):
    try:
        os.makedirs(logdir, exist_ok=True)
        from scipy.io import wavfile
        for i in range(pred_wav.shape[0]):
            wavfile.write(os.path.join(logdir, 'pred_%d.wav' % i), hp.signal.sr, np.clip(pred_wav[i, :, 0], -1, 1))
        np.save(os.path.join(logdir, 'pred_wav.npy'), pred_wav)
        print('wrote %d waveform(s) to %s' % (pred_wav.shape[0], logdir))
    except OSError as e:
        print('could not write outputs to %s: %s' % (logdir, e))


def _write_outputs_varlen(pred_wavs, logdir):
    """--varlen: pred_i.wav at utterance i's own length, and every waveform in pred_wav_varlen.npz (as pred_i)."""
    try:
        os.makedirs(logdir, exist_ok=True)
        from scipy.io import wavfile
        for i, w in enumerate(pred_wavs):
            wavfile.write(os.path.join(logdir, 'pred_%d.wav' % i), hp.signal.sr, np.clip(w[:, 0], -1, 1))
        np.savez(os.path.join(logdir, 'pred_wav_varlen.npz'), **{'pred_%d' % i: w for i, w in enumerate(pred_wavs)})
        print('wrote %d waveform(s) of %s samples to %s' % (len(pred_wavs), [len(w) for w in pred_wavs], logdir))
    except OSError as e:
        print('could not write outputs to %s: %s' % (logdir, e))


def _generate_over_ranks(store, batch_size, length, device, logdir, ckpt, debug, score=False):
    """generate() under a launcher (WORLD_SIZE > 1): see forward_over_ranks.  --score: rank 0 scores the gathered result."""
    import torch.distributed as dist
    from . import engine
    from .timeshard import chain_halo
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    if not dist.is_initialized():
        dist.init_process_group(backend='nccl', device_id=device)      # 'nccl' IS RCCL on ROCm (xGMI)
    rank = dist.get_rank()
    hop, n_mels = hp.signal.hop_length, hp.signal.n_mels
    info = {}
    gt_wav, melspec = _load_mels(hp.data_path, batch_size, length, device, info) if rank == 0 else (None, None)
    ckpt = '{}/{}'.format(logdir, ckpt) if ckpt else (_latest_checkpoint(logdir) if os.path.isdir(logdir) else None)
    if ckpt:
        store.load_checkpoint(ckpt, use_ema=bool(hp.train.use_ema))
    elif rank == 0:
        print('No checkpoint found at {}.'.format(logdir))
    seed = torch.tensor([int(os.environ.get('PWV_NOISE_SEED') or engine.os_seed())], dtype=torch.int64, device=device)
    dist.broadcast(seed, src=0)                                         # one noise stream for the whole job
    seed = int(seed.item())
    halo = chain_halo(hp.model.dilations, hp.model.filter_width, hp.model.n_iaf, hop)

    errors = []

    def make_model(n, window):
        # A failure anywhere in this rank's share -- the constructor (length not a multiple of the hop), the forward, its
        # verification -- must not leave the other ranks alone in the gather: hand back zeros, keep the collectives paired,
        # and let the failure bit below stop every rank before anything is written
        try:
            m = IAFVocoder(batch_size=n, length=window, store=store)
        except Exception as e:
            errors.append(e)
            m = None

        def run(mel, z):
            # a verified call (explicitly: verify=True outranks PWV_ASYNC=1): this rank's share is complete and checked --
            # rerun on per-layer launches / in exact fp32 if need be -- BEFORE it is gathered
            try:
                if m is None:
                    raise errors[0]
                return m(None, mel, is_training=False, z=z, verify=True)
            except Exception as e:
                if not errors or errors[-1] is not e:
                    errors.append(e)
                return torch.zeros((mel.shape[0], window, 1), dtype=torch.float32, device=device)
        return run

    def noise_window(n, first_sample, window, first_item):
        try:
            return engine.logistic_noise_window(n, length, first_sample, window, device, seed, first_item)
        except Exception as e:
            errors.append(e)
            return torch.zeros((n, window, 1), dtype=torch.float32, device=device)

    # a normaliser that reduces over time (modules.py:274-284) makes a time slice depend on the whole utterance: such a model
    # shards by utterance only (ranks beyond the batch idle) -- timeshard.py is exact for causal FIR structure, nothing else
    time_ok = 'in' not in (hp.model.normalize, hp.model.normalize_cond, hp.model.normalize_wavenet)
    pred = forward_over_ranks(melspec, batch_size, length, device, make_model, noise_window, n_mels, hop, halo, allow_time_shards=time_ok)
    flag = torch.tensor([1 if errors else 0], dtype=torch.int32, device=device)
    dist.all_reduce(flag, op=dist.ReduceOp.MAX)          # rank 0 writes only what EVERY rank has verified
    if int(flag.item()):
        if errors:
            raise errors[0]
        raise RuntimeError('generate(): the forward failed on another rank; nothing was written')
    if ckpt and store.not_restored():
        missing = store.not_restored()
        raise KeyError('checkpoint %s does not hold %d of the model\'s %d variables: %s' % (ckpt, len(missing), len(store.vars), ', '.join(missing[:6])))
    if ckpt and hp.train.use_ema and store.ema_missing():
        raise KeyError('checkpoint %s has no ExponentialMovingAverage shadow for: %s' % (ckpt, ', '.join(store.ema_missing()[:6])))
    if rank != 0:
        return None
    pred_wav = pred.cpu().numpy()
    _write_outputs(pred_wav, logdir)
    if score:
        _score_outputs(pred, gt_wav, melspec, info.get('files'), logdir, device)
    print('Done.')
    return pred_wav


def _fire(fn, argv):
    """Minimal python-fire work-alike: positionals, --name=value, --name value, --flag (a bare flag may be followed by
    another option: `generate c --debug --ckpt foo`)."""
    pos, kw = [], {}
    i = 0
    while i < len(argv):
        a = argv[i]
        i += 1
        if not a.startswith('--'):
            pos.append(a)
            continue
        k, eq, v = a[2:].partition('=')
        k = k.replace('-', '_')
        if not eq:
            if i < len(argv) and not argv[i].startswith('--'):
                v = argv[i]
                i += 1
            else:
                kw[k] = True           # bare flag; the next token (if any) is an option of its own
                continue
        kw[k] = {'True': True, 'False': False}.get(v, v)
    return fn(*pos, **kw)


if __name__ == '__main__':
    _fire(generate, sys.argv[1:])
