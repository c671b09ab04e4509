"""GPU: the capture lifecycle the three graph wrappers share (graph._Captured; DESIGN.md section 9, "The capture lifecycle"), pinned on
each of them at its smallest shapes: one capture at construction, replays with the eager bits, a re-capture after new weights and
after another value of a launch knob, verify() clean and no eager call throughout."""
import numpy as np
import pytest
import torch

from oracle import iaf_oracle as O
from tests.util import set_hparams, small_cfg

pytestmark = pytest.mark.gpu
HOP = 80


def _uniform(gpu, model, cfg):
    from pwv_amd.graph import GraphedVocoder
    from pwv_amd.models import IAFVocoder
    one = IAFVocoder(batch_size=2, length=480, store=model.store)
    mel_np, z_np = O.synthetic_inputs(2, 480, cfg)
    mel, z = torch.from_numpy(mel_np).to(gpu), torch.from_numpy(z_np).to(gpu)
    g = GraphedVocoder(one)

    def call():
        got = g(mel, z=z).clone()
        g.verify()
        return [got], [one(None, mel, is_training=False, z=z)]
    return g, call


def _packed(gpu, model, cfg):
    from pwv_amd.graph import GraphedPackedVocoder
    rng = np.random.default_rng(0)
    mels = [torch.from_numpy(rng.uniform(-1, 1, (L // HOP + 1, cfg.n_mels)).astype(np.float32)).to(gpu) for L in (320, 160)]
    seeds = [2 ** 63 + 5, 7]
    g = GraphedPackedVocoder(model, 3, 800)

    def call():
        got = [p.clone() for p in g(mels, seeds)]
        g.verify()
        return got, list(model.generate_varlen(mels, seeds=seeds))
    return g, call


def _stream(gpu, model, cfg):
    rng = np.random.default_rng(1)

    def rand(*shape):
        return torch.from_numpy(rng.uniform(-1, 1, shape).astype(np.float32)).to(gpu)
    a, b = model.open_stream(slots=2), model.open_stream(slots=2)
    first = rand(2, 1, cfg.n_mels)
    for s in (a, b):                                   # a session starts with the eager one-frame push
        assert tuple(s.push(first, z=torch.zeros((2, 0, 1), device=gpu)).shape) == (2, 0, 1)
    g = a.graphed(2, 2, sample=False)

    def call():
        mel, z = rand(2, 2, cfg.n_mels), rand(2, 2 * HOP, 1)
        got = g.tick(mel, [0, 1], z=z).clone()
        assert g.verify() == 1
        want = b.push(mel, z=z)                        # the second stream: advanced by push from the same state
        assert [a.emitted(i) for i in range(2)] == [b.emitted(i) for i in range(2)]
        return [got], [want]
    return g, call


@pytest.mark.parametrize('wrapper', [_uniform, _packed, _stream], ids=['GraphedVocoder', 'GraphedPackedVocoder', 'GraphedStream'])
def test_capture_lifecycle(gpu, monkeypatch, wrapper):
    from pwv_amd import engine
    from pwv_amd.models import IAFVocoder
    from pwv_amd.variables import VariableStore
    cfg = small_cfg(dilations=[[1, 2, 4, 8], [1, 2, 4, 8]], n_iaf=2)      # L = 4 in every flow: the least the persistent route takes
    set_hparams(cfg)
    store = VariableStore(device=gpu)
    store.load_dict(O.init_weights(cfg, seed=4))
    engine.resume_persist()
    g, call = wrapper(gpu, IAFVocoder(batch_size=1, length=HOP, store=store), cfg)

    def same(captures):
        got, want = call()
        assert g.captures == captures and g.eager_calls == 0
        assert len(got) == len(want) and all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(got, want))
        return got

    assert g.captures == 1
    first = same(1)
    same(1)                                            # a second call replays the same capture
    name = 'iaf_vocoder/iaf0/scalar/postprocessing/postprocess2_bias'
    store.assign(name, (store.vars[name] + 0.25).cpu().numpy())
    again = same(2)                                    # new weights: the captured launches point at stale packs
    if wrapper is not _stream:                         # (same inputs as before: the new weights show)
        assert not any(torch.equal(x, y) for x, y in zip(again, first))
    monkeypatch.setattr(engine, 'FUSE_PROLOGUE', not engine.FUSE_PROLOGUE)
    same(3)                                            # another launch knob (bit-identical either way, every flow stays persistent)
    g.verify()
    assert g.captures == 3 and g.eager_calls == 0
