"""Packed batches with one noise stream per utterance: the eager packed forward on the model's own stream, the eager one with seeds,
and the replay of a graph.GraphedPackedVocoder captured at exactly the batch's rows ("Graph replay of packed
batches").

Mixes (hparams/default.yaml model, random weights):
  short    8 utterances of 2000 .. 9600 samples (R = 26000: the short-input instantiation)
  general  8000 * k samples, k = 1 .. 8 (R = 288000)
Every leg only enqueues (verify=False); after --warmup calls, --steps calls are enqueued back to back and the host clock is read
around them and a final synchronisation: ms per forward as a server that keeps the GPU fed sees it (the host's enqueue cost
included).  Prints one JSON line: per mix and leg ms per forward and real samples per second, the rows the graph computes against the
real ones, and per mix whether the launches took the short-input instantiation.

    python tools/varlen_graph_bench.py [--steps 20] [--warmup 5] [--precision f16x3]
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MIXES = {'short': [2000, 2400, 2000, 3200, 2000, 2800, 2000, 9600], 'general': [8000 * k for k in range(1, 9)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--precision', default='f16x3', choices=['f16x3', 'f32'])
    args = ap.parse_args()

    import numpy as np
    import torch
    from oracle import iaf_oracle as O
    from pwv_amd import _lib, engine
    from pwv_amd.graph import GraphedPackedVocoder
    from pwv_amd.models import IAFVocoder
    from pwv_amd.variables import VariableStore
    from tests.util import set_hparams

    dev = torch.device('cuda', 0)
    cfg = O.ModelConfig()
    set_hparams(cfg)
    store = VariableStore(device=dev)
    store.load_dict(O.init_weights(cfg, seed=2))
    rng = np.random.default_rng(0)
    out = {'precision': args.precision, 'steps': args.steps, 'warmup': args.warmup}
    for mix, lengths in MIXES.items():
        R = sum(lengths)
        mels = [torch.from_numpy(rng.uniform(-1, 1, (L // cfg.hop_length + 1, cfg.n_mels)).astype(np.float32)).to(dev) for L in lengths]
        seeds = list(range(1, len(lengths) + 1))
        model = IAFVocoder(batch_size=1, length=80, store=store, precision=args.precision)
        graphed = GraphedPackedVocoder(model, len(lengths), R)
        legs = {
            'eager_stream': lambda: model.generate_varlen(mels, verify=False),
            'eager_seeds': lambda: model.generate_varlen(mels, seeds=seeds, verify=False),
            'graph_replay': lambda: graphed(mels, seeds),
        }
        res = {'lengths': lengths, 'real_rows': R, 'graph_rows': graphed.rows}
        for name, fn in legs.items():
            for _ in range(args.warmup):
                fn()
            engine.verify_enqueued(name)
            t0 = time.perf_counter()
            for _ in range(args.steps):
                fn()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / args.steps
            engine.verify_enqueued(name)      # (a give-up or a range trip invalidates the leg: raise instead of reporting it)
            res[name] = {'ms': round(ms, 4), 'real_samples_per_s': round(R / ms * 1e3, 1)}
        assert graphed.captures == 1 and graphed.eager_calls == 0
        short = []
        engine.PERSIST_ARGS_HOOK = lambda pa: short.append(_lib.lib().pwv_persist_short_input(ctypes.byref(pa)))
        model.generate_varlen(mels, seeds=seeds)
        engine.PERSIST_ARGS_HOOK = None
        res['short_input_instantiation'] = bool(short) and all(v == 1 for v in short)
        res['replay_vs_eager_seeds'] = round(res['eager_seeds']['ms'] / res['graph_replay']['ms'], 3)
        out[mix] = res
    print(json.dumps(out))


if __name__ == '__main__':
    main()
