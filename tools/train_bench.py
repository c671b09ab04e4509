"""What a training step costs ("Training"): the default model, random weights, 8 x 4000 samples (the reference's
training batch, hparams/default.yaml), one GPU.

Legs, each the median over --steps calls (at least 20) after --warmup calls (at least 3) of the time between two events recorded on the
stream around the call:
  forward_f32          the generation forward IAFVocoder(8, 4000, precision='f32'), enqueue-only: what the forward kernels take
  train_forward        the training forward alone: every layer's input kept (pwv_train_*_fwd_f32), the loss not formed
  loss_and_grad        forward with saved activations + backward + the frame-rate work
  trainer_step         loss_and_grad + Adam + EMA (torch._foreach) + VariableStore.touch()
  forward_after_step   the generation forward right after a touch(): it re-packs every weight first
  repack               forward_after_step - forward_f32
There is no threshold: the file records a first measurement.  Writes profiles/train_bench.json and prints it as one JSON line.

    python tools/train_bench.py [--steps 20] [--warmup 3]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--length', type=int, default=4000)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'train_bench.json'))
    args = ap.parse_args()
    steps, warmup = max(args.steps, 20), max(args.warmup, 3)

    import numpy as np
    import torch
    from oracle import iaf_oracle as O
    from pwv_amd import train as TR
    from pwv_amd.models import IAFVocoder
    from pwv_amd.variables import VariableStore
    from tests.util import set_hparams

    dev = torch.device('cuda', 0)
    cfg = O.ModelConfig()
    set_hparams(cfg)
    store = VariableStore(device=dev)
    store.load_dict(O.init_weights(cfg, seed=2))
    n, length = args.batch, args.length
    mel_np, z_np = O.synthetic_inputs(n, length, cfg)
    mel, z = torch.from_numpy(mel_np).to(dev), torch.from_numpy(z_np).to(dev)
    wav = torch.from_numpy((0.3 * np.random.RandomState(5).randn(n, length)).astype(np.float32)).to(dev)
    model = IAFVocoder(batch_size=n, length=length, store=store, precision='f32')
    trainer = TR.Trainer(model)

    def timed(fn, before=None):
        ms = []
        for k in range(warmup + steps):
            if before is not None:
                before()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if k >= warmup:
                ms.append(e0.elapsed_time(e1))
        return statistics.median(ms), min(ms), max(ms)

    def forward():
        model(None, mel, z=z, verify=False)

    def train_forward():
        flows = TR.model_nets(model, store)
        nets = [net for pair in flows for net in pair]
        geo = TR._Geometry(n, length, mel.shape[1], sum(128 * len(net.dilations) for net in nets), 0)
        geo.P = train_forward.P
        x = z.reshape(-1)
        for pair in flows:
            s = [TR._net_forward(net, geo, x, geo.P) for net in pair]
            x = x * s[0][2] + s[1][2]

    cols = 128 * 2 * sum(len(d) for d in cfg.dilations)
    train_forward.P = torch.zeros((n * mel.shape[1], cols), dtype=torch.float32, device=dev)

    legs = {}
    legs['forward_f32'] = timed(forward)
    model.verify()
    legs['train_forward'] = timed(train_forward)
    legs['loss_and_grad'] = timed(lambda: TR.loss_and_grad(model, wav, mel, z=z))
    legs['trainer_step'] = timed(lambda: trainer.step(wav, mel, z=z))
    legs['forward_after_step'] = timed(forward, before=store.touch)
    model.verify()
    peak = torch.cuda.max_memory_allocated() / 2 ** 20
    out = {'model': 'default (4 flows, 10 + 10 + 10 + 30 layers, 2 nets each)', 'batch': n, 'length': length, 'steps': steps, 'warmup': warmup,
           'device': torch.cuda.get_device_name(0), 'peak_allocated_MiB': round(peak, 1)}
    for k, (med, lo, hi) in legs.items():
        out[k + '_ms'] = {'median': round(med, 3), 'min': round(lo, 3), 'max': round(hi, 3)}
    out['repack_ms'] = round(legs['forward_after_step'][0] - legs['forward_f32'][0], 3)
    out['backward_over_train_forward'] = round((legs['loss_and_grad'][0] - legs['train_forward'][0]) / legs['train_forward'][0], 2)
    out['loss_and_grad_over_forward_f32'] = round(legs['loss_and_grad'][0] / legs['forward_f32'][0], 2)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
