"""CPU: the yardsticks of tests/test_gpu_train_shapes.py -- tests/train_oracle.py and tests/train_varlen_oracle.py parametrised by the
batch shape and the hop length.  With their default arguments they return what the module constants gave before they took arguments;
the front-backward restatement is pinned by float64 autograd; the model-level problems keep their input margins.  Nothing here needs a
GPU."""
import numpy as np
import pytest
import torch

from oracle import iaf_oracle as O
from tests import train_oracle as TO
from tests import train_varlen_oracle as VO

UNIFORM = [(3, 208, 16), (3, 240, 80), (5, 16, 16), (1, 16, 16), (2, 200, 40)]
PACKED = [((208, 16, 48, 128), 16), ((240, 80, 80), 80), ((16,), 16), ((208, 208, 208), 16)]


def _equal(a, b, path=''):
    """np.array_equal over nested tuples, lists and dicts; a dict `a` may hold keys that `b` lacks."""
    if isinstance(b, dict):
        assert set(b) <= set(a), path
        for k in b:
            _equal(a[k], b[k], '%s/%s' % (path, k))
    elif isinstance(b, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _equal(x, y, '%s/%d' % (path, i))
    elif b is None or isinstance(b, (int, float, str)):
        assert a == b, (path, a, b)
    else:
        assert np.array_equal(np.asarray(a), np.asarray(b)), path


def test_default_arguments_are_the_module_constants():
    """problem(), reference(), layer_case() and layer_grads() without arguments = the same with (N, T, HOP) = (2, 208, 16) spelt out, and
    their inputs are what the constants gave: the weights of seed 3, O.synthetic_inputs(2, 208), the wav of seed 5, 14 frames."""
    assert (TO.N, TO.T, TO.HOP) == (2, 208, 16) and TO.small_cfg().hop_length == 16
    cfg, w, mel, z, wav = TO.problem()
    _equal(TO.problem(TO.N, TO.T, TO.HOP)[1:], (w, mel, z, wav))
    _equal(w, O.init_weights(TO.small_cfg(), seed=3))
    _equal((mel, z), O.synthetic_inputs(2, 208, TO.small_cfg()))
    assert np.array_equal(wav, (0.3 * np.random.RandomState(5).randn(2, 208, 1)).astype(np.float32))
    ref = TO.reference()
    _equal(TO.reference(TO.N, TO.T, TO.HOP), ref)
    l64, p64, g64 = TO.loss_and_grads(w, mel, z, wav, cfg, torch.float64)
    _equal(ref, {'loss': l64, 'pred': p64, 'g64': g64})
    for d in (1, 48):
        c = TO.layer_case(d)
        assert c['frames'] == 14 and c['x'].shape == (2, 208, 64) and c['P'].shape == (28, 128) and c['offset'] == 8
        _equal(TO.layer_case(d, hop=16, N=2, T=208, offset=8), c)
        rng = np.random.RandomState(11 + d)             # the draws in their order: x, P, then the weights
        assert np.array_equal(c['x'], rng.randn(2, 208, 64).astype(np.float32))
        assert np.array_equal(c['P'], (0.5 * rng.randn(28, 128)).astype(np.float32))
        for last in (False, True):
            _equal(TO.layer_grads(TO.layer_case(d, hop=16, N=2, T=208, offset=8), last, torch.float64), TO.layer_grads(c, last, torch.float64))


def test_a_cpu_store_leaves_the_yardsticks_weights_alone():
    """The weights of problem() are shared by every training test, and a CPU VariableStore once aliased the arrays it was loaded from
    (torch.as_tensor of a float32 array, .to('cpu')): an optimiser step on such a store (tests/test_train_host.py) then rewrote the
    yardstick's weights for every test after it.  The store keeps a copy of its own."""
    from pwv_amd import train as TR
    from pwv_amd.variables import VariableStore
    w = TO.problem()[1]
    store = VariableStore(device='cpu')
    store.load_dict(w)
    names = sorted(w)
    vars = [store.vars[n] for n in names]
    assert not any(np.shares_memory(v.numpy(), w[n]) for n, v in zip(names, vars))
    TR.adam_ema_update(vars, [torch.ones_like(v) for v in vars], None, 1e-2)
    assert all(not np.array_equal(v.numpy(), w[n]) for n, v in zip(names, vars))
    _equal(w, O.init_weights(TO.small_cfg(), seed=3))


def test_packed_default_arguments_are_the_module_constants():
    """The same for the packed oracle: LENGTHS at hop 16, wavs of seeds 60 + i, the weights of the uniform problem."""
    assert (VO.LENGTHS, VO.HOP) == ([208, 16, 48, 144], 16)
    cfg, w, mels, zs, wavs = VO.problem()
    _equal(VO.problem(tuple(VO.LENGTHS), VO.HOP)[1:], (w, mels, zs, wavs))
    assert w is TO.problem()[1] and cfg.hop_length == 16
    for i, T in enumerate(VO.LENGTHS):
        _equal((mels[i], zs[i]), O.synthetic_inputs(1, T, cfg, mel_seed=20 + i, z_seed=40 + i))
        assert np.array_equal(wavs[i], (0.3 * np.random.RandomState(60 + i).randn(1, T, 1)).astype(np.float32))
    _equal(VO.reference(lengths=tuple(VO.LENGTHS), hop=VO.HOP), VO.reference())
    for d in (1, 48):
        c = VO.layer_case(d)
        _equal(VO.layer_case(d, lengths=tuple(VO.LENGTHS), hop=VO.HOP), c)
        assert c['frames'] == VO.FRAMES and c['cu_rows'] == VO.CU_ROWS and c['x'].shape == (VO.ROWS, 64)
        _equal({k: c[k] for k in ('filter', 'gate', 'dense', 'skip', 'post1', 'post2', 'post2_bias')}, {k: TO.layer_case(d)[k] for k in ('filter', 'gate', 'dense', 'skip', 'post1', 'post2', 'post2_bias')})


@pytest.mark.parametrize('N, T, hop, offset, frames', [(2, 208, 7, 3, 31), (2, 100, 7, 3, 15), (3, 48, 32, 31, 3), (1, 300, 256, 128, 2), (2, 200, 80, 40, 3)])
def test_layer_case_counts_frames_when_the_hop_does_not_divide_T(N, T, hop, offset, frames):
    """frames = (T - 1 + offset) // hop + 1: the frame of the last sample, + 1; every frame is read, none beyond them."""
    c = TO.layer_case(1, hop=hop, N=N, T=T, offset=offset)
    assert c['frames'] == frames and c['P'].shape == (N * frames, 128)
    g = TO.layer_grads(c, False, torch.float64)
    per_frame = np.abs(g['P']).reshape(N, frames, 128).max(axis=2)
    assert (per_frame > 0).all()


FRONT = [([208] * 3, 1), ([208] * 3, 3), ([200] * 2, 3), ([16] * 5, 1), ([16], 3), ([16], 48), ([208, 16, 48, 128], 3), ([240, 80, 80], 1)]


@pytest.mark.parametrize('lengths, dn', FRONT, ids=['%s-dn%d' % ('-'.join(map(str, l)), dn) for l, dn in FRONT])
def test_front_restatement_matches_float64_autograd(lengths, dn):
    """tests.train_oracle.front_backward in float64 against autograd of in -> x_0 through oracle.torch_cpu.causal_conv_torch, every
    utterance on its own, to 1e-12 of each output's largest entry, for the three ways d_in starts; the float32 restatement is the
    same arithmetic (within 1e-5)."""
    c = TO.front_case(lengths, dn)
    for base in TO.FRONT_BASES:
        got, want, single = TO.front_backward(c, base), TO.front_backward_autograd(c, base), TO.front_backward(c, base, np.float32)
        for k in ('cf', 'd_in'):
            assert got[k].shape == want[k].shape and got[k].dtype == np.float64 and single[k].dtype == np.float32
            assert TO.rel_err(got[k], want[k]) <= 1e-12, (base, k)
            assert 0 < TO.rel_err(single[k], want[k]) <= 1e-5, (base, k)
    bases = [TO.front_base(c, b) for b in TO.FRONT_BASES]
    assert np.abs(bases[0]).max() == 0 and not np.array_equal(bases[1], bases[2]) and np.abs(bases[1]).min() > 0
    if dn >= max(lengths):          # nothing is gathered
        assert np.array_equal(TO.look_ahead(c['U'], c['V'], dn, c['cu_rows']), c['U'])


@pytest.mark.parametrize('shape', UNIFORM, ids=lambda s: '-'.join(map(str, s)))
def test_uniform_problems_keep_their_input_margins(shape):
    """Every conditioning pre-activation at least RELU_MARGIN from the ReLU's kink and every prediction at least SIGN_MARGIN = 5 x
    TOL_F32 from its target in float64 (conditions on the inputs: below them a float32 evaluation may legitimately take the other
    branch); 149 variables with a gradient, 32 without."""
    from tests.util import TOL_F32
    assert TO.SIGN_MARGIN == pytest.approx(5 * TOL_F32)
    cfg, w, mel, z, wav = TO.problem(*shape)
    assert cfg.hop_length == shape[2] and wav.shape == (shape[0], shape[1], 1) and mel.shape[1] == 1 + shape[1] // shape[2]
    _equal(w, TO.problem()[1])              # the weights do not depend on the shape
    ref = TO.reference(*shape)
    assert TO.relu_margin(w, mel) >= TO.RELU_MARGIN
    assert np.abs(ref['pred'] - wav).min() >= TO.SIGN_MARGIN
    assert sum(v is not None for v in ref['g64'].values()) == 149 and sum(v is None for v in ref['g64'].values()) == 32
    assert 0 < ref['E32'] < 1e-5


@pytest.mark.parametrize('lengths, hop', PACKED, ids=['-'.join(map(str, l)) for l, _ in PACKED])
def test_packed_problems_keep_their_input_margins(lengths, hop):
    cfg, w, mels, zs, wavs = VO.problem(lengths, hop)
    assert cfg.hop_length == hop and [y.shape for y in wavs] == [(1, T, 1) for T in lengths]
    ref = VO.reference(lengths=lengths, hop=hop)
    assert min(TO.relu_margin(w, m) for m in mels) >= TO.RELU_MARGIN
    assert min(float(np.abs(p - y.reshape(-1)).min()) for p, y in zip(ref['preds'], wavs)) >= TO.SIGN_MARGIN
    assert sum(v is not None for v in ref['g64'].values()) == 149 and 0 < ref['E32'] < 1e-5


def test_the_wav_seed_moves_on_where_a_prediction_sits_on_its_target():
    """3 x 80 at hop 80: seed 5 leaves a sample within SIGN_MARGIN of its prediction, so problem() draws from a later seed -- the rule
    is the margin, not the seed."""
    cfg, w, mel, z, wav = TO.problem(3, 80, 80)
    pred = TO.pred64(w, mel, z, cfg)
    first = (0.3 * np.random.RandomState(TO.WAV_SEED).randn(3, 80, 1)).astype(np.float32)
    assert np.abs(pred - first).min() < TO.SIGN_MARGIN
    assert not np.array_equal(wav, first) and np.abs(pred - wav).min() >= TO.SIGN_MARGIN
