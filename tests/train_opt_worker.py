"""The child processes of tests/test_gpu_train_opt.py (a process group is a per-process thing, and a rank is a fresh process):

    python -m tests.train_opt_worker nccl1 OUT.json     world size 1 over nccl: DataParallelTrainer against Trainer(fused=True), 3 steps
    python -m tests.train_opt_worker rank  OUTDIR       one of WORLD_SIZE ranks (RANK in the environment): ONE utterance of the N = 2
                                                        problem of tests/train_oracle.py per rank, 3 steps

A rank uses GPU rank % device_count(), and `nccl` when every rank has a GPU of its own, else `gloo` through the host copy on the shared
GPU.  Everything a test compares is written to files; a failure is an exception and a non-zero exit status."""
import json
import os
import socket
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import train_oracle as TO          # noqa: E402
from tests.util import set_hparams            # noqa: E402

STEPS = 3


def _model(device, n, seed=None):
    from pwv_amd.models import IAFVocoder
    from pwv_amd.variables import VariableStore
    cfg, w, _, _, _ = TO.problem()
    set_hparams(cfg)
    store = VariableStore(device=device)
    store.load_dict(w)
    model = IAFVocoder(batch_size=n, length=TO.T, store=store, precision='f32')
    model.noise_seed = seed
    return model, store


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _state(tr):
    """{kind/name: numpy} of everything a trainer holds after its steps."""
    out = {}
    for n, v, m, s, sh in zip(tr.names, [tr.store.vars[n] for n in tr.names], tr.state['m'], tr.state['v'], tr.state['shadow']):
        out['var/' + n], out['m/' + n], out['v/' + n], out['shadow/' + n] = (t.detach().cpu().numpy() for t in (v, m, s, sh))
    return out


def nccl1(out_path):
    from pwv_amd import train as TR
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(s.getsockname()[1]), RANK='0', WORLD_SIZE='1')
    s.close()
    device = torch.device('cuda', 0)
    torch.cuda.set_device(device)
    dist.init_process_group(backend='nccl', device_id=device)
    try:
        _, _, mel, _, wav = TO.problem()
        wav, mel = _dev(wav, device), _dev(mel, device)
        kw = dict(lr=TO.LR, beta2=TO.BETA2, ema_decay=TO.DECAY)
        # the noise is drawn, not given: at world size 1 the schedule of the ranks is the running offset of one process
        m_dp, _ = _model(device, TO.N, seed=7)
        dp = TR.DataParallelTrainer(m_dp, **kw)
        losses_dp = [float(dp.step(wav, mel)) for _ in range(STEPS)]
        mean = float(dp.mean_loss())
        m_one, _ = _model(device, TO.N, seed=7)
        one = TR.Trainer(m_one, fused=True, **kw)
        losses_one = [float(one.step(wav, mel)) for _ in range(STEPS)]
        a, b = _state(dp), _state(one)
        differ = sorted(k for k in a if not np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)))
        res = dict(backend=dist.get_backend(), world=dp.world, steps=dp.steps, losses_dp=losses_dp, losses_one=losses_one, mean_loss=mean,
                   arrays=len(a), differ=differ, offsets=[m_dp.noise_offset, m_one.noise_offset])
    finally:
        dist.destroy_process_group()
    with open(out_path, 'w') as f:
        json.dump(res, f)


def rank_main(out_dir):
    from pwv_amd import train as TR
    rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
    count = torch.cuda.device_count()
    device = torch.device('cuda', rank % count)
    torch.cuda.set_device(device)
    if count >= world:
        dist.init_process_group(backend='nccl', device_id=device)
    else:
        dist.init_process_group(backend='gloo')
    try:
        _, _, mel, z, wav = TO.problem()
        assert world == TO.N
        wav, mel, z = (_dev(a[rank:rank + 1], device) for a in (wav, mel, z))
        model, _ = _model(device, 1)
        tr = TR.DataParallelTrainer(model, lr=TO.LR, beta2=TO.BETA2, ema_decay=TO.DECAY)
        losses = [float(tr.step(wav, mel, z=z))]
        grads = {n: g.detach().cpu().numpy().copy() for n, g in tr.gradients().items()}          # the SUM over the ranks
        np.savez(os.path.join(out_dir, 'grads_rank%d.npz' % rank), **grads)
        losses += [float(tr.step(wav, mel, z=z)) for _ in range(STEPS - 1)]
        np.savez(os.path.join(out_dir, 'state_rank%d.npz' % rank), **_state(tr))
        tr.save(os.path.join(out_dir, 'ckpt_rank%d.npz' % rank))                                  # every rank calls it; rank 0 writes
        with open(os.path.join(out_dir, 'info_rank%d.json' % rank), 'w') as f:
            json.dump(dict(backend=dist.get_backend(), world=tr.world, rank=tr.rank, device=str(device), steps=tr.steps, losses=losses,
                           mean_loss=float(tr.mean_loss())), f)
    finally:
        dist.destroy_process_group()


if __name__ == '__main__':
    {'nccl1': nccl1, 'rank': rank_main}[sys.argv[1]](sys.argv[2])
