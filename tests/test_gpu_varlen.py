"""GPU: packed ("varlen") batches -- utterances of different lengths in one unpadded forward (IAFVocoder.generate_varlen,
engine.run_flow_varlen, pwv_persist_args.cu_rows).  Every utterance of a packed forward equals its own single-utterance forward bit
for bit, the oracle within the fp32 bar, and the padded fallback gives the same bits."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import iaf_oracle as O
from tests.guarded import Guard
from tests.util import TOL_F32, set_hparams, small_cfg

pytestmark = pytest.mark.gpu


def _small():
    # (every flow at least 4 layers: shorter stacks have no persistent form, packed or not)
    return small_cfg(dilations=[[1, 2, 4, 8], [1, 2, 4, 8, 16, 32]])


def _model(gpu, cfg, precision=None, seed=2):
    from pwv_amd.models import IAFVocoder
    from pwv_amd.variables import VariableStore
    set_hparams(cfg)
    w = O.init_weights(cfg, seed=seed)
    store = VariableStore(device=gpu)
    store.load_dict(w)
    return IAFVocoder(batch_size=1, length=80, store=store, precision=precision), w


def _inputs(cfg, lengths, seed=0):
    rng = np.random.default_rng(seed)
    mels = [rng.uniform(-1, 1, (L // cfg.hop_length + 1, cfg.n_mels)).astype(np.float32) for L in lengths]
    zs = [np.clip(rng.logistic(0, 1, (L, 1)), -20, 20).astype(np.float32) for L in lengths]
    return mels, zs


@pytest.fixture()
def launches(monkeypatch):
    """(pwv_persist_args fields, short-input verdict) of every persistent launch, and the count of padded flows."""
    from pwv_amd import _lib, engine
    seen = []

    def hook(pa):
        seen.append(dict(cu_rows=pa.cu_rows, cu_frames=pa.cu_frames, unit_map=pa.unit_map, rows=pa.varlen_rows, N=pa.N,
                         short=_lib.lib().pwv_persist_short_input(ctypes.byref(pa))))
    monkeypatch.setattr(engine, 'PERSIST_ARGS_HOOK', hook)
    monkeypatch.setattr(engine, 'VARLEN_PADDED', 0)
    return seen


@pytest.mark.parametrize('precision', ['f16x3', 'f32'])
def test_packed_equals_single_utterance_forwards(gpu, precision, launches):
    """Default model; one utterance shorter than the largest dilation, several ending inside a 32-row unit: every piece of the
    packed forward is torch.equal to IAFVocoder(1, len_i) on the same mel and z; all launches carry the packed fields (general
    instantiation: R = 152240 rows), no flow was padded."""
    from pwv_amd import engine
    from pwv_amd.models import IAFVocoder
    cfg = O.ModelConfig()
    lengths = [16000, 80, 4000, 32080, 100080]
    model, _ = _model(gpu, cfg, precision)
    mels, zs = _inputs(cfg, lengths)
    mel_t = [torch.from_numpy(m).to(gpu) for m in mels]
    z_t = [torch.from_numpy(z).to(gpu) for z in zs]
    out = model.generate_varlen(mel_t, z=z_t)
    torch.cuda.synchronize()
    R = sum(lengths)
    assert tuple(out.packed.shape) == (R, 1) and [tuple(o.shape) for o in out] == [(L, 1) for L in lengths]
    assert engine.VARLEN_PADDED == 0 and len(launches) == 4
    assert all(a['cu_rows'] and a['cu_frames'] and a['unit_map'] and a['rows'] == R and a['N'] == len(lengths) and a['short'] == 0
               for a in launches)
    engine.PERSIST_ARGS_HOOK = None
    for L, m, z, o in zip(lengths, mel_t, z_t, out):
        one = IAFVocoder(batch_size=1, length=L, store=model.store, precision=precision)
        want = one(None, m[None], is_training=False, z=z[None])[0]
        assert torch.equal(o, want), (L, float((o - want).abs().max()))


@pytest.mark.parametrize('precision', ['f16x3', 'f32'])
def test_packed_matches_oracle_short_input(gpu, precision, launches):
    """[800, 2400, 1600] against the fp64 oracle per utterance (fp32 bar); R = 4800 rows take the short-input instantiation."""
    from pwv_amd import engine
    cfg = O.ModelConfig()
    lengths = [800, 2400, 1600]
    model, w = _model(gpu, cfg, precision)
    mels, zs = _inputs(cfg, lengths, seed=1)
    out = model.generate_varlen([torch.from_numpy(m).to(gpu) for m in mels], z=torch.from_numpy(np.concatenate(zs)).to(gpu),
                                verify=False)
    model.verify()
    assert engine.VARLEN_PADDED == 0 and launches and all(a['short'] == 1 and a['unit_map'] for a in launches)
    for m, z, o in zip(mels, zs, out):
        want = O.iaf_vocoder_forward(w, m[None], z[None], cfg)[0]
        err = float(np.abs(o.cpu().numpy() - want).max())
        assert err <= TOL_F32, err


@pytest.mark.parametrize('why', ['persist_off', 'above_auto_rows'])
def test_padded_fallback_same_bits(gpu, launches, monkeypatch, why):
    """PWV_PERSIST=0, or more rows than PERSIST_AUTO_MAX_ROWS: every flow takes the padded fallback (no persistent launch) and the result
    is the packed path's, bit for bit."""
    from pwv_amd import engine
    cfg = _small()
    lengths = [480, 80, 1360, 800]
    model, _ = _model(gpu, cfg)
    mels, zs = _inputs(cfg, lengths, seed=2)
    mel_t = [torch.from_numpy(m).to(gpu) for m in mels]
    z = torch.from_numpy(np.concatenate(zs)).to(gpu)
    packed = model.generate_varlen(mel_t, z=z).packed
    assert engine.VARLEN_PADDED == 0 and launches
    del launches[:]
    if why == 'persist_off':
        monkeypatch.setattr(engine, 'PERSIST', False)
    else:
        monkeypatch.setattr(engine, 'PERSIST_AUTO_MAX_ROWS', sum(lengths) - 1)
    padded = model.generate_varlen(mel_t, z=z).packed
    assert engine.VARLEN_PADDED == cfg.n_iaf and not launches
    assert torch.equal(packed, padded)


def test_unit_map_matches_numpy(gpu, built_lib):
    from pwv_amd import _lib, engine
    lengths = [37, 4000, 33, 1653, 32, 80]
    geom = engine.VarlenGeometry(lengths, 1, gpu)
    got = geom.unit_map().cpu().numpy().reshape(-1, _lib.VARLEN_REC_INTS)
    cu_r, cu_f = np.array(geom.cu_rows_host), np.array(geom.cu_frames_host)
    units = (cu_r[-1] + 31) // 32
    n = np.searchsorted(cu_r, np.arange(units) * 32, side='right') - 1
    want = np.zeros((units, _lib.VARLEN_REC_INTS), np.int32)
    want[:, 0], want[:, 1], want[:, 2], want[:, 3], want[:, 4] = n, cu_r[n], cu_f[n], cu_r[n + 1], cu_f[n + 1]
    assert np.array_equal(got, want)


@pytest.mark.parametrize('precision', ['f16x3', 'f32'])
def test_guard_bands_around_the_packed_output(gpu, precision):
    """The affine output of a packed flow written inside a poisoned buffer (tests/guarded.py): the bands in front of and behind it stay untouched
    (bounded buffer descriptors drop out-of-range stores silently; a parity test alone would not see an off-by-one), and every
    utterance equals its own uniform flow.  Odd lengths without a condition: units straddle every boundary."""
    from pwv_amd import engine
    from pwv_amd.modules import LinearIAFLayer, WaveNet
    from pwv_amd.variables import VariableStore
    set_hparams(O.ModelConfig())
    store = VariableStore(device=gpu)
    kw = dict(batch_size=1, dilations=[1, 2, 4, 8, 16, 32, 64, 128, 256, 512], filter_width=2, residual_channels=64, dilation_channels=64,
              skip_channels=128, use_skip_connection=False, is_training=False, store=store, precision=precision, quantization_channels=1)
    flow = LinearIAFLayer(1, WaveNet(name='scalar', **kw), WaveNet(name='shifter', **kw))
    lengths = [37, 4000, 1653, 33, 2080]
    geom = engine.VarlenGeometry(lengths, 1, gpu)
    R = geom.rows
    torch.manual_seed(0)
    x = torch.randn((R, 1), device=gpu)
    for n in flow.nets():           # create the variables (a uniform call), small random weights
        n(x[:64][None], None)
    for k, v in store.vars.items():
        v.copy_(torch.randn_like(v) * 0.1)
    store.version += 1
    bands = Guard(band_bytes=16384)            # the output as a NaN payload between two 0xFF bands, compared byte for byte afterwards
    out = bands.allocate((1, R, 1), torch.float32, gpu, None)
    res = engine._run_nets(flow.nets(), x.view(1, R, 1), None, precision, 0, out, geom)
    torch.cuda.synchronize()
    assert res is not None and res[1], 'the packed flow must run as persistent launches with the affine inside'
    bands.check()
    assert not bool(torch.isnan(out).any())
    for a, b in zip(geom.cu_rows_host, geom.cu_rows_host[1:]):
        want = engine.run_flow(flow.nets(), x[a:b][None], None, precision=precision)
        assert torch.equal(out[0, a:b], want[0])


def test_noise_continues_the_stream_and_range_rerun_is_exact_f32(gpu):
    """Two calls without z draw consecutive counter ranges (row r of a call = counter offset + r); a split-fp16 forward that trips the
    range guard is rerun in exact fp32 on the same noise and equals precision='f32'."""
    from pwv_amd import engine
    from pwv_amd.models import IAFVocoder
    cfg = _small()
    lengths = [480, 160, 800]
    model, _ = _model(gpu, cfg)
    model.noise_seed = 11
    mels, _ = _inputs(cfg, lengths, seed=3)
    mel_t = [torch.from_numpy(m).to(gpu) for m in mels]
    R = sum(lengths)
    first, second = model.generate_varlen(mel_t).packed, model.generate_varlen(mel_t).packed
    assert model.noise_offset == 2 * R
    for k, got in enumerate((first, second)):
        z = engine.logistic_noise_op((R, 1), gpu, seed=11, offset=k * R)
        assert torch.equal(got, model.generate_varlen(mel_t, z=z).packed)
    big = [m * 1e5 for m in mel_t]
    model.noise_seed, model.noise_offset = 12, 0
    with pytest.warns(UserWarning, match='rerun in exact fp32'):
        got = model.generate_varlen(big).packed
    z = engine.logistic_noise_op((R, 1), gpu, seed=12, offset=0)
    m32 = IAFVocoder(batch_size=1, length=80, store=model.store, precision='f32')
    assert torch.equal(got, m32.generate_varlen(big, z=z).packed)


def test_generate_cli_varlen(gpu, tmp_path, monkeypatch):
    """`generate default --varlen` on three .npy mels of different lengths writes three waveforms of (t_mel - 1) * hop samples."""
    from scipy.io import wavfile
    from pwv_amd.generate import _fire, generate
    from pwv_amd.hparam import hparam as hp
    rng = np.random.default_rng(4)
    frames = [3, 21, 9]
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
    pred = _fire(generate, ['default', '--varlen'])
    assert [p.shape for p in pred] == [((f - 1) * 80, 1) for f in frames]
    for i, f in enumerate(frames):
        rate, data = wavfile.read(str(logdir / ('pred_%d.wav' % i)))
        assert data.shape == ((f - 1) * 80,)
