"""Mixed-length batches: one packed forward (IAFVocoder.generate_varlen) against padding every utterance to the longest and
against a loop of single-utterance forwards, with a uniform batch of the same total rows as the reference point.

Workload: the default model (hparams/default.yaml, random weights), utterances of 8000 * k samples, k = 1 .. 8 (R = 288000 real
samples).  Every leg is a graph-free eager forward (verify=False: only enqueues) on fixed inputs; after --warmup forwards, --steps
forwards are bracketed by HIP events each.  Prints one JSON line: ms per forward (median) and real samples per second per leg, and
the ratios the acceptance targets are stated in (padded / varlen >= 1.5, varlen within 5 % of the uniform batch's samples/s).

    python tools/varlen_bench.py [--steps 20] [--warmup 5] [--precision f16x3] [--unit 8000]

--unit 24000 (R = 864000, above engine.PERSIST_AUTO_MAX_ROWS) times the padded fallback of the packed call instead: every flow then
runs on the padded batch, and `varlen_padded_flows` counts them.  `fallback_index_ms` is what a fresh batch layout costs in front of
that (the layout, the device-side row and frame maps, one pad and one gather; host clock around a synchronised call).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--precision', default='f16x3', choices=['f16x3', 'f32'])
    ap.add_argument('--unit', type=int, default=8000, help='utterance k has unit * k samples, k = 1 .. 8 (a multiple of 80)')
    args = ap.parse_args()

    import numpy as np
    import torch
    from oracle import iaf_oracle as O
    from pwv_amd import engine
    from pwv_amd.models import IAFVocoder
    from pwv_amd.variables import VariableStore
    from tests.util import set_hparams

    dev = torch.device('cuda', 0)
    cfg = O.ModelConfig()
    set_hparams(cfg)
    store = VariableStore(device=dev)
    store.load_dict(O.init_weights(cfg, seed=2))
    hop, n_mels = cfg.hop_length, cfg.n_mels
    lengths = [args.unit * k for k in range(1, 9)]
    R, n, L_max = sum(lengths), len(lengths), max(lengths)
    rng = np.random.default_rng(0)
    mels = [torch.from_numpy(rng.uniform(-1, 1, (L // hop + 1, n_mels)).astype(np.float32)).to(dev) for L in lengths]
    zs = [torch.from_numpy(np.clip(rng.logistic(0, 1, (L, 1)), -20, 20).astype(np.float32)).to(dev) for L in lengths]
    z_packed = torch.cat(zs)

    def model(batch, length):
        return IAFVocoder(batch_size=batch, length=length, store=store, precision=args.precision)

    # varlen: one packed forward
    mv = model(1, 80)
    # padded: every utterance zero-padded to the longest (mel frames and noise), one uniform forward
    mp = model(n, L_max)
    mel_pad = torch.zeros((n, L_max // hop + 1, n_mels), device=dev)
    z_pad = torch.zeros((n, L_max, 1), device=dev)
    for i, (m, z) in enumerate(zip(mels, zs)):
        mel_pad[i, :m.shape[0]] = m
        z_pad[i, :z.shape[0]] = z
    # loop: one forward per utterance
    singles = [model(1, L) for L in lengths]
    # uniform: the same R real rows as n equal utterances
    Lu = R // n
    mu = model(n, Lu)
    mel_u = torch.from_numpy(rng.uniform(-1, 1, (n, Lu // hop + 1, n_mels)).astype(np.float32)).to(dev)
    z_u = torch.from_numpy(np.clip(rng.logistic(0, 1, (n, Lu, 1)), -20, 20).astype(np.float32)).to(dev)

    legs = {
        'varlen': lambda: mv.generate_varlen(mels, z=z_packed, verify=False),
        'padded': lambda: mp(None, mel_pad, is_training=False, z=z_pad, verify=False),
        'loop': lambda: [s(None, m[None], is_training=False, z=z[None], verify=False) for s, m, z in zip(singles, mels, zs)],
        'uniform_same_rows': lambda: mu(None, mel_u, is_training=False, z=z_u, verify=False),
    }
    padded0 = engine.VARLEN_PADDED
    out = {'lengths': lengths, 'real_samples': R, 'precision': args.precision, 'steps': args.steps, 'warmup': args.warmup}
    for name, fn in legs.items():
        for _ in range(args.warmup):
            fn()
        engine.verify_enqueued(name)
        times = []
        for _ in range(args.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            times.append((e0, e1))
        engine.verify_enqueued(name)         # (a give-up or a range trip invalidates the leg: raise instead of reporting it)
        ms = statistics.median(a.elapsed_time(b) for a, b in times)
        out[name] = {'ms': round(ms, 4), 'real_samples_per_s': round(R / ms * 1e3, 1)}
    out['varlen_padded_flows'] = engine.VARLEN_PADDED - padded0      # 0: every flow of the packed forward ran unpadded
    idx = []
    for _ in range(args.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        geom = engine.VarlenGeometry(lengths, hop, dev)
        geom.unpad_rows(geom.pad_rows(z_packed))
        geom.pad_frames(torch.cat(mels))
        torch.cuda.synchronize()
        idx.append((time.perf_counter() - t0) * 1e3)
    out['fallback_index_ms'] = round(statistics.median(idx), 4)
    out['speedup_vs_padded'] = round(out['padded']['ms'] / out['varlen']['ms'], 3)
    out['speedup_vs_loop'] = round(out['loop']['ms'] / out['varlen']['ms'], 3)
    out['varlen_vs_uniform'] = round(out['varlen']['real_samples_per_s'] / out['uniform_same_rows']['real_samples_per_s'], 4)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
