"""What scoring costs next to the forward it scores ("Scoring on the device"): default model, random weights, one GPU.

Two cells, each with two legs timed in the same process:
  uniform   3 x 64000 samples: `score(pred, gt)` against the verified forward IAFVocoder(3, 64000)(mel, verify=True)
  varlen    8 utterances of mixed lengths summing to 64000 samples: `score_varlen(preds, gts)` on the forward's own output object against
            the verified IAFVocoder.generate_varlen
A leg = the median over --steps calls (at least 20) after --warmup calls (at least 3) of the time between two events recorded on the
stream around the call.  `share` = score / (score + forward): what part of a `generate --score` run's device time the scoring is (the
mel L1 of --score, a second front-end pass, is not in it).  There is no threshold: the file records a first measurement.
Writes profiles/score_bench.json and prints it as one JSON line.

    python tools/score_bench.py [--steps 20] [--warmup 3] [--precision f16x3]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARLEN_LENGTHS = (2400, 4000, 5600, 7200, 8800, 10400, 12000, 13600)      # 8 mixed lengths, 64000 samples


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--precision', default='f16x3', choices=['f16x3', 'f32'])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'score_bench.json'))
    args = ap.parse_args()
    steps, warmup = max(args.steps, 20), max(args.warmup, 3)

    import numpy as np
    import torch
    from oracle import iaf_oracle as O
    from pwv_amd import score as S
    from pwv_amd.models import IAFVocoder
    from pwv_amd.variables import VariableStore
    from tests.util import set_hparams

    dev = torch.device('cuda', 0)
    cfg = O.ModelConfig()
    hp = set_hparams(cfg)
    store = VariableStore(device=dev)
    store.load_dict(O.init_weights(cfg, seed=2))
    hop, n_mels = cfg.hop_length, cfg.n_mels
    win = int(hp.signal.win_length)
    rng = np.random.default_rng(0)

    def rand(*shape):
        return torch.from_numpy(rng.uniform(-1, 1, shape).astype(np.float32)).to(dev)

    def timed(fn):
        ms = []
        for k in range(warmup + steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if k >= warmup:
                ms.append(e0.elapsed_time(e1))
        return statistics.median(ms)

    def cell(forward_ms, score_ms, scores):
        return dict(forward_ms=round(forward_ms, 4), score_ms=round(score_ms, 4), share=round(score_ms / (score_ms + forward_ms), 4),
                    likelihood=scores.likelihood, power_loss=scores.power_loss, frames=[int(f) for f in scores.frames])

    result = dict(tool='score_bench', device=torch.cuda.get_device_name(0), precision=args.precision, steps=steps, warmup=warmup,
                  win_length=win, hop_length=hop, timing='median of event-timed calls, ms')

    n, length = 3, 64000
    assert sum(VARLEN_LENGTHS) == length and len(VARLEN_LENGTHS) == 8
    model = IAFVocoder(batch_size=n, length=length, store=store, precision=args.precision)
    mel, gt = rand(n, 1 + length // hop, n_mels), 0.5 * rand(n, length, 1)
    pred = model(None, mel, is_training=False, verify=True)
    forward_ms = timed(lambda: model(None, mel, is_training=False, verify=True))
    score_ms = timed(lambda: S.score(pred, gt))
    result['uniform_3x64000'] = cell(forward_ms, score_ms, S.score(pred, gt))

    packed = IAFVocoder(batch_size=1, length=length, store=store, precision=args.precision)
    mels = [rand(1 + t // hop, n_mels) for t in VARLEN_LENGTHS]
    gts = [0.5 * rand(t, 1) for t in VARLEN_LENGTHS]
    preds = packed.generate_varlen(mels, verify=True)
    forward_ms = timed(lambda: packed.generate_varlen(mels, verify=True))
    score_ms = timed(lambda: S.score_varlen(preds, gts))
    result['varlen_8_mixed_64000'] = cell(forward_ms, score_ms, S.score_varlen(preds, gts))
    result['varlen_lengths'] = list(VARLEN_LENGTHS)

    line = json.dumps(result)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
