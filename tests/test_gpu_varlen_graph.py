"""GPU: per-utterance noise streams of packed batches (IAFVocoder.generate_varlen(seeds=...), pwv_logistic_noise_packed_f32) and
their graph replay (graph.GraphedPackedVocoder).  Every comparison is torch.equal: an utterance's result depends on its mel and its
stream only -- not on its companions, its position, the route the batch takes, or whether it ran eagerly or from a graph."""
import numpy as np
import pytest
import torch

from oracle import iaf_oracle as O
from tests.util import set_hparams, small_cfg

pytestmark = pytest.mark.gpu

SEEDS = [2 ** 64 - 1, 7, 2 ** 63 + 12345, 0]
OFFSETS = [0, 2 ** 40 - 3, 17, 2 ** 40 + 5]


def _model(gpu, cfg, precision=None, seed=2):
    from pwv_amd.models import IAFVocoder
    from pwv_amd.variables import VariableStore
    set_hparams(cfg)
    store = VariableStore(device=gpu)
    store.load_dict(O.init_weights(cfg, seed=seed))
    return IAFVocoder(batch_size=1, length=80, store=store, precision=precision)


def _mels(cfg, lengths, gpu, seed=0):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy(rng.uniform(-1, 1, (L // cfg.hop_length + 1, cfg.n_mels)).astype(np.float32)).to(gpu) for L in lengths]


def _single(model, mel, seed, offset):
    """The reference of the contract: the utterance alone, IAFVocoder(1, len) drawing from (seed, offset)."""
    from pwv_amd.hparam import hparam as hp
    from pwv_amd.models import IAFVocoder
    one = IAFVocoder(batch_size=1, length=(mel.shape[0] - 1) * hp.signal.hop_length, store=model.store, precision=model.precision)
    one.noise_seed, one.noise_offset = seed, offset
    return one(None, mel[None], is_training=False)[0]


@pytest.mark.parametrize('n', [1, 257])
def test_packed_sampler_equals_per_utterance_draws(gpu, n):
    """Odd lengths (utterances end inside a 256-row block, several inside one), seeds >= 2**63, offsets near 2**40."""
    from pwv_amd import engine
    rng = np.random.default_rng(n)
    lengths = [int(v) for v in rng.integers(1, 700, n)]
    seeds = [int(v) + (2 ** 63 if i % 2 == 0 else 0) for i, v in enumerate(rng.integers(0, 2 ** 62, n))]
    offsets = [2 ** 40 - 300 + int(v) for v in rng.integers(0, 600, n)]
    geom = engine.VarlenGeometry(lengths, 1, gpu)
    table = geom.stream_table(list(zip(seeds, offsets)))
    want = torch.cat([engine.logistic_noise_op((L, 1), gpu, seed=s, offset=o) for L, s, o in zip(lengths, seeds, offsets)])
    assert torch.equal(engine.logistic_noise_packed_op(geom.cu_rows, table, geom.rows), want)
    out = torch.full((geom.rows, 1), float('nan'), device=gpu)
    engine.logistic_noise_packed_op(geom.cu_rows, table, geom.rows, out=out)
    assert torch.equal(out, want)


@pytest.mark.parametrize('precision', ['f16x3', 'f32'])
def test_seeded_pieces_are_batch_invariant(gpu, precision):
    """Default model (general instantiation) and a short-input mix: every piece equals its single-utterance forward on
    (seed_i, offset_i), in any order and with other companions; the model's own noise_offset does not move."""
    from pwv_amd import engine
    cfg = O.ModelConfig()
    model = _model(gpu, cfg, precision)
    model.noise_seed, model.noise_offset = 5, 123
    padded0 = engine.VARLEN_PADDED
    for lengths in ([16000, 80, 4000, 32080], [800, 2400, 1600, 160]):
        mels = _mels(cfg, lengths, gpu)
        out = model.generate_varlen(mels, seeds=SEEDS, offsets=OFFSETS)
        for m, s, o, piece in zip(mels, SEEDS, OFFSETS, out):
            assert torch.equal(piece, _single(model, m, s, o))
        perm = [2, 0, 3, 1]
        again = model.generate_varlen([mels[i] for i in perm], seeds=[SEEDS[i] for i in perm], offsets=[OFFSETS[i] for i in perm])
        for k, i in enumerate(perm):
            assert torch.equal(again[k], out[i])
        other = _mels(cfg, [4000, 1200], gpu, seed=9)             # other companions, utterance 0 in the middle
        mix = model.generate_varlen([other[0], mels[0], other[1]], seeds=[3, SEEDS[0], 4], offsets=[0, OFFSETS[0], 0])
        assert torch.equal(mix[1], out[0])
    assert model.noise_offset == 123 and engine.VARLEN_PADDED == padded0


@pytest.mark.parametrize('route', ['persist_off', 'instance_norm'])
def test_seeded_pieces_on_the_fallback_routes(gpu, monkeypatch, route):
    """PWV_PERSIST=0 (every flow on the padded batch) and an 'in' config (utterance by utterance): the same contract."""
    from pwv_amd import engine
    cfg = small_cfg(dilations=[[1, 2, 4, 8], [1, 2, 4, 8, 16, 32]], normalize='in' if route == 'instance_norm' else '')
    model = _model(gpu, cfg)
    if route == 'persist_off':
        monkeypatch.setattr(engine, 'PERSIST', False)
    mels = _mels(cfg, [480, 80, 1360, 800], gpu, seed=2)
    padded0 = engine.VARLEN_PADDED
    out = model.generate_varlen(mels, seeds=SEEDS, offsets=OFFSETS)
    assert engine.VARLEN_PADDED == padded0 + (cfg.n_iaf if route == 'persist_off' else 0)
    for m, s, o, piece in zip(mels, SEEDS, OFFSETS, out):
        assert torch.equal(piece, _single(model, m, s, o))


def _graph(gpu, slots, rows, precision='f16x3'):
    from pwv_amd.graph import GraphedPackedVocoder
    cfg = O.ModelConfig()
    model = _model(gpu, cfg, precision)
    return cfg, model, GraphedPackedVocoder(model, slots, rows)


def _replay(graphed, mels, seeds, offsets=None):
    out = graphed(mels, seeds, offsets)
    graphed.verify()
    return [o.clone() for o in out]


@pytest.mark.parametrize('precision', ['f16x3', 'f32'])
def test_graph_replays_any_layout_with_the_eager_bits(gpu, precision):
    """One capture at 4 slots / 24000 rows: an exact fit, a layout with fillers, the same one reordered and one with two fillers
    each equal the eager seeded call."""
    from pwv_amd import engine
    cfg, model, g = _graph(gpu, 4, 24000, precision)
    padded0 = engine.VARLEN_PADDED
    a = _mels(cfg, [8000, 4000, 80, 11920], gpu, seed=0)
    b = _mels(cfg, [16000, 4000], gpu, seed=1)
    c = _mels(cfg, [160, 800, 2400], gpu, seed=3)
    layouts = [(a, SEEDS, OFFSETS), (b, [11, 2 ** 63 + 1], [0, 2 ** 40]), (b[::-1], [2 ** 63 + 1, 11], [2 ** 40, 0]), (c, [1, 2, 3], None)]
    results = []
    for mels, seeds, offsets in layouts:
        got = _replay(g, mels, seeds, offsets)
        want = model.generate_varlen(mels, seeds=seeds, offsets=offsets)
        assert len(got) == len(mels)
        for m, x, y in zip(mels, got, want):
            assert tuple(x.shape) == ((m.shape[0] - 1) * 80, 1) and torch.equal(x, y)
        results.append(got)
    assert torch.equal(results[2][0], results[1][1]) and torch.equal(results[2][1], results[1][0])
    assert g.captures == 1 and g.eager_calls == 0 and engine.VARLEN_PADDED == padded0


def test_graph_recaptures_after_a_weight_change(gpu):
    cfg, model, g = _graph(gpu, 3, 8000)
    mels = _mels(cfg, [4000, 2400], gpu)
    before = _replay(g, mels, [1, 2])
    for v in model.store.vars.values():
        v.mul_(0.9)
    model.store.version += 1
    after = _replay(g, mels, [1, 2])
    assert g.captures == 2 and g.eager_calls == 0
    want = model.generate_varlen(mels, seeds=[1, 2])
    for x, y, old in zip(after, want, before):
        assert torch.equal(x, y) and not torch.equal(x, old)


@pytest.mark.parametrize('change, why', [(dict(cond_upsample_method='transposed_conv'), 'transposed_conv'),
                                         (dict(use_skip_connection=True), 'skip accumulation'),
                                         (dict(dilations=[[1, 2, 4]], n_iaf=1), 'per layer')])
def test_graph_refuses_configs_without_a_packed_persistent_route(gpu, change, why):
    from pwv_amd import _lib
    from pwv_amd.graph import GraphedPackedVocoder
    kw = dict(dilations=[[1, 2, 4, 8], [1, 2, 4, 8, 16, 32]])
    kw.update(change)
    model = _model(gpu, small_cfg(**kw))
    with pytest.raises(_lib.PwvError, match=why):
        GraphedPackedVocoder(model, 2, 1600)


def test_graph_give_up_runs_eagerly_then_recaptures(gpu):
    """A give-up (the status word poked from the host, as a launch that gave up would leave it): verify() raises PwvPersistError,
    the next call runs eagerly with the same bits, and once the suspension ends the graph is captured again.  A poked range word
    makes verify() raise PwvRangeError."""
    from pwv_amd import _lib, engine
    cfg, model, g = _graph(gpu, 3, 12000)
    mels = _mels(cfg, [4000, 2400], gpu)
    want = [p.clone() for p in model.generate_varlen(mels, seeds=[5, 6])]
    try:
        g(mels, [5, 6])
        torch.cuda.synchronize()
        engine.poke_persist_status(3)
        with pytest.raises(_lib.PwvPersistError):
            g.verify()
        assert engine.persist_suspended()
        got = _replay(g, mels, [5, 6])
        assert g.eager_calls == 1 and g.captures == 1
        assert all(torch.equal(x, y) for x, y in zip(got, want))
        engine.resume_persist()
        got = _replay(g, mels, [5, 6])
        assert g.captures == 2 and g.eager_calls == 1
        assert all(torch.equal(x, y) for x, y in zip(got, want))
        g(mels, [5, 6])
        torch.cuda.synchronize()
        engine.current_words().range = 1
        with pytest.raises(_lib.PwvRangeError):
            g.verify()
    finally:
        engine.resume_persist()
        engine.clear_persist_status()
        engine.clear_range_flag()


def test_graph_layout_that_does_not_fit_runs_eagerly(gpu):
    cfg, model, g = _graph(gpu, 2, 8000)
    mels = _mels(cfg, [4000, 2400, 800], gpu)                  # 3 utterances for 2 slots
    got = _replay(g, mels, [1, 2, 3])
    want = model.generate_varlen(mels, seeds=[1, 2, 3])
    assert g.eager_calls == 1 and g.captures == 1 and all(torch.equal(x, y) for x, y in zip(got, want))


def test_generate_cli_seed_is_batch_invariant(gpu, tmp_path, monkeypatch):
    """`generate --varlen --seed=S`: a file's wav is the same whether it is vocoded alone or with other files in another order."""
    from scipy.io import wavfile
    from pwv_amd.generate import _fire, generate
    from pwv_amd.hparam import hparam as hp
    rng = np.random.default_rng(4)
    for name, f in (('b.npy', 21), ('a.npy', 3), ('c.npy', 9)):
        np.save(str(tmp_path / name), rng.uniform(-1, 1, (f, 80)).astype(np.float32))
    orig = type(hp).set_hparam_yaml
    pattern = {}

    def patched(self, case, *a, **k):          # what a user's hparams.yaml case would override
        r = orig(self, case, *a, **k)
        self.data_path = pattern['p']
        self.train.dataset_ratio, self.generate.batch_size = 0.0, 3
        self.model.n_iaf, self.model.dilations = 1, [[1, 2, 4, 8]]
        return r

    monkeypatch.setattr(type(hp), 'set_hparam_yaml', patched)
    runs = {}
    for key, pat in (('alone', 'b.npy'), ('all', '*.npy')):
        pattern['p'] = str(tmp_path / pat)
        monkeypatch.setenv('PWV_LOGDIR', str(tmp_path / key))
        _fire(generate, ['default', '--varlen', '--seed=77'])
        runs[key] = tmp_path / key
    _, alone = wavfile.read(str(runs['alone'] / 'pred_0.wav'))
    _, with_others = wavfile.read(str(runs['all'] / 'pred_1.wav'))        # sorted: a.npy, b.npy, c.npy
    assert alone.shape == (20 * 80,) and np.array_equal(alone, with_others)
