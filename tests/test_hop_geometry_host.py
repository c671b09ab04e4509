"""CPU: the conditioning geometry at hop lengths other than 80 (the GPU side: tests/test_gpu_hop_geometry.py).

First, that the GPU cases have teeth: for every (hop, length) of the one-shot cases (tests/util.HOP_CASES) a condition that is off by
one SAMPLE (offset +- 1) or by one FRAME moves the fp64 oracle's output by at least 100 x TOL_F32 -- a kernel that reads the wrong P row
cannot hide under the parity bar.  Then the host logic that carries a hop, against plain-Python restatements: stream.ragged_plan /
push_samples, timeshard.shard_plan / chain_halo, the filler arithmetic of graph.GraphedPackedVocoder and the frame-count guard of
engine.RepeatedCondition at its boundary."""
import numpy as np
import pytest

from oracle import iaf_oracle as O
from tests.util import HOP_CASES, HOPS, TOL_F32, hop_cfg

HOST_HOPS = (2, 16, 48, 256)


def _forward_with_condition(weights, cfg, frames, z, offset, frame_shift=0):
    """The oracle's flows (models.py:34-70) on the condition frames[:, (t + offset) // hop + frame_shift] (frame_shift wraps around)."""
    hop, length = cfg.hop_length, z.shape[1]
    idx = ((np.arange(length) + offset) // hop + frame_shift) % frames.shape[1]
    cond = frames[:, idx, :]
    x = z.astype(np.float64)
    for i in range(cfg.n_iaf):
        x = O.linear_iaf(weights, 'iaf_vocoder/iaf%d' % i, x, cond, dilations=cfg.dilations[i], use_biases=cfg.use_biases,
                         use_skip_connection=cfg.use_skip_connection)
    return x


@pytest.mark.parametrize('hop', HOPS)
def test_the_gpu_cases_have_teeth(hop):
    cfg = hop_cfg(hop)
    n, length = HOP_CASES[hop]
    assert length % hop == 0 and length // hop >= 3 and n in (2, 3) and n * length <= 1536
    weights = O.init_weights(cfg, seed=2)
    mel, z = O.synthetic_inputs(n, length, cfg)
    want = O.iaf_vocoder_forward(weights, mel, z, cfg)
    frames = O.frame_cond_repeat(weights, mel)
    # (the restatement is the oracle's own condition at offset hop // 2)
    assert np.array_equal(_forward_with_condition(weights, cfg, frames, z, hop // 2), want)
    for what, kw in (('offset + 1', dict(offset=hop // 2 + 1)), ('offset - 1', dict(offset=hop // 2 - 1)),
                     ('one frame', dict(offset=hop // 2, frame_shift=1))):
        moved = np.abs(_forward_with_condition(weights, cfg, frames, z, **kw) - want).max()
        assert moved >= 100 * TOL_F32, (hop, what, moved)


# ---- stream.push_samples / ragged_plan ---------------------------------------------------------------------------------------------
def _plan_restated(frames, fresh, hop):
    samples, launch, cu_rows, cu_frames = [], [], [0], [0]
    for i, (f, fr) in enumerate(zip(frames, fresh)):
        t = f * hop - (hop if fr else 0)          # a fresh session keeps its last frame back
        samples.append(t)
        if t > 0:
            launch.append(i)
            cu_rows.append(cu_rows[-1] + t)
            cu_frames.append(cu_frames[-1] + (f if fr else f + 1))      # a running one brings its kept frame
    return samples, launch, cu_rows, cu_frames


@pytest.mark.parametrize('hop', HOST_HOPS)
def test_ragged_plan_at_other_hops(hop):
    from pwv_amd.stream import push_samples, ragged_plan
    assert push_samples(1, True, hop) == 0 and push_samples(1, False, hop) == hop and push_samples(5, True, hop) == 4 * hop
    rng = np.random.RandomState(hop)
    for _ in range(20):
        n = int(rng.randint(1, 7))
        frames = [int(v) for v in rng.randint(1, 9, n)]
        fresh = [bool(v) for v in rng.randint(0, 2, n)]
        plan = ragged_plan(frames, fresh, hop)
        assert (plan.samples, plan.launch, plan.cu_rows, plan.cu_frames) == _plan_restated(frames, fresh, hop)
        # the packed layout's t_mel = len / hop + 1, whatever the hop
        assert all(b - a == (plan.samples[i] // hop) + 1 for i, a, b in zip(plan.launch, plan.cu_frames, plan.cu_frames[1:]))
    with pytest.raises(ValueError):
        ragged_plan([0], [True], hop)


# ---- timeshard.chain_halo / shard_plan ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hop', HOST_HOPS)
def test_shard_plan_and_chain_halo_at_other_hops(hop):
    from pwv_amd.timeshard import chain_halo, shard_plan
    cfg = hop_cfg(hop)
    reach = sum(sum(d) + 1 for d in cfg.dilations)        # W = 2: a net sees sum(d) + 1 past samples
    halo = chain_halo(cfg.dilations, cfg.filter_width, cfg.n_iaf, hop)
    assert halo % hop == 0 and reach <= halo < reach + hop
    for frames, shards in ((3, 3), (7, 3), (7, 10), (40, 4), (41, 6)):
        length = frames * hop
        plan = shard_plan(length, shards, halo, hop)
        assert len(plan) == min(shards, frames)
        assert plan[0][1] == 0 and plan[-1][2] == length
        for (c0, a, b), nxt in zip(plan, plan[1:] + [None]):
            assert a % hop == b % hop == c0 % hop == 0 and a < b and c0 == max(0, a - halo)
            assert nxt is None or nxt[1] == b
        sizes = [(b - a) // hop for _, a, b in plan]
        assert max(sizes) - min(sizes) <= 1
    with pytest.raises(ValueError):
        shard_plan(3 * hop + 1, 2, halo, hop)


# ---- graph.GraphedPackedVocoder's filler ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hop,want', [(2, 32), (16, 32), (48, 48), (256, 256), (6, 36), (32, 32), (34, 34), (80, 80)])
def test_filler_rows(hop, want):
    from pwv_amd import _lib
    from pwv_amd.graph import packed_filler_rows
    got = packed_filler_rows(hop)
    assert got == want
    # the smallest length that is a legal utterance of a packed persistent launch: a positive multiple of hop of at least 32 rows
    assert got == min(v for v in range(hop, 40 * hop + 1, hop) if v >= _lib.VARLEN_MIN_ROWS)


# ---- engine.RepeatedCondition's frame-count guard ------------------------------------------------------------------------------------
@pytest.mark.parametrize('hop', HOST_HOPS)
def test_repeated_condition_guard_at_its_boundary(hop):
    import torch
    from pwv_amd.engine import RepeatedCondition
    for offset in (0, hop // 2, hop - 1):
        for n_frames in (1, 4):
            frames = torch.zeros((2, n_frames, 8))
            longest = n_frames * hop - offset          # sample t reads frame (t + offset) // hop: the last one serves t < longest
            assert RepeatedCondition(frames, hop, offset, longest).shape == (2, longest, 8)
            with pytest.raises(ValueError, match='needs more than %d frames' % n_frames):
                RepeatedCondition(frames, hop, offset, longest + 1)
    # IAFVocoder's own geometry: (t_mel - 1) * hop samples at offset hop // 2 need all t_mel frames and no more
    for t_mel in (2, 5):
        frames = torch.zeros((1, t_mel, 8))
        RepeatedCondition(frames, hop, hop // 2, (t_mel - 1) * hop)
        with pytest.raises(ValueError):
            RepeatedCondition(frames[:, :-1], hop, hop // 2, (t_mel - 1) * hop)
