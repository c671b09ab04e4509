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

--power measures what the STFT power loss adds instead (same model, batch and machine, one run): loss_and_grad with
power_weight=0.0005 (the loss head is pwv_train_loss_f32, csrc/pwv_train_loss.hip) and with power_weight=None (the L1 in torch), the two
ALTERNATING call by call so that clock and co-tenants treat them alike, and the loss head alone (the C call on a fixed pred, timed over
runs of 20 calls) at weight 0.0005 and at weight 0 (the L1 alone).  Writes profiles/train_power_bench.json.

    python tools/train_bench.py --power [--steps 20] [--warmup 3]

--varlen measures packed training ("Packed training"; train.loss_and_grad_varlen -> pwv_train_varlen_*), four legs
ALTERNATING call by call in one run, same model and z:
  a_uniform_8x4000         loss_and_grad at 8 x 4000
  b_packed_equal           loss_and_grad_varlen at eight equal lengths of 4000: what the per-unit lookup of the packed kernels costs
  c_packed_mixed           loss_and_grad_varlen at eight mixed lengths that sum to 32000
  d_uniform_padded_mixed   loss_and_grad on the same mixed lengths zero-padded to the longest: what a user pays today
Writes profiles/train_varlen_bench.json.

    python tools/train_bench.py --varlen [--steps 20] [--warmup 3]

--tran measures training of the transposed-conv conditioning ("Training the transposed-conv conditioning";
include/pwv_hip_train_cond.h) against the default 'repeat' conditioning: the default model at 8 x 4000 with either conditioning, same
mel, z and wav, the two loss_and_grad ALTERNATING call by call in one run, and the conditioning stages alone (the three transposed-conv
GEMMs + ReLU forward, their backward in torch on a fixed d_cond), whose share of the step is reported.  There is no threshold.  Writes
profiles/train_tran_bench.json.

    python tools/train_bench.py --tran [--steps 20] [--warmup 3]

--opt measures the fused optimiser ("Data-parallel training"; include/pwv_hip_train_opt.h): Trainer.step with
fused=False (adam_ema_update's torch._foreach passes) and with fused=True (one pack launch + one Adam + EMA launch), two trainers over
two copies of the model ALTERNATING call by call in one run, and alone, timed over runs of 20 calls: the pack of a step's gradients
(the upload of its table of addresses included), the Adam + EMA launch, an unpack of the variables, and adam_ema_update on the same
gradients.  With --gpus N it also starts, for every world size in {1, 2, 4, 8} up to N that the machine has devices for, that many
fresh processes, one per GPU, and measures DataParallelTrainer.step per rank at the same per-rank batch and the all-reduce of the
gradient arena alone (the slowest rank's median).  There is no threshold.  Writes profiles/train_dp_bench.json.

    python tools/train_bench.py --opt [--gpus N] [--steps 20] [--warmup 3]

--skip measures training of the skip-connection architecture ("Training the skip-connection architecture";
include/pwv_hip_train_skip.h) against the default one: the default model at 8 x 4000 with and without model.use_skip_connection, the
same weights, mel, z and wav, the two loss_and_grad ALTERNATING call by call in one run, and the residual layer-backward launch alone
(kernel + reduction, dilation 1, timed over runs of 20 calls) in both forms.  There is no threshold.  Writes
profiles/train_skip_bench.json.

    python tools/train_bench.py --skip [--steps 20] [--warmup 3]

--shared measures training of the shared-net architecture ("Training the shared-net architecture";
include/pwv_hip_train_shared.h) against the default one: the default model (8 nets) and bench/c2's model (model.shared_nets: 4 nets,
weights of its own) at 8 x 4000 on the same mel, z and wav, the two loss_and_grad ALTERNATING call by call in one run, and the head
backward launch alone (kernel + reduction, timed over runs of 20 calls): the existing one-output head against the two-output one on
the same o.  There is no threshold.  Writes profiles/train_shared_bench.json.

    python tools/train_bench.py --shared [--steps 20] [--warmup 3]
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
    ap.add_argument('--power', action='store_true', help='measure loss_and_grad with and without the STFT power loss instead')
    ap.add_argument('--varlen', action='store_true', help='measure packed batches against uniform and padded ones instead')
    ap.add_argument('--tran', action='store_true', help='measure transposed-conv conditioning against repeat conditioning instead')
    ap.add_argument('--opt', action='store_true', help='measure the fused optimiser against the torch._foreach one instead')
    ap.add_argument('--skip', action='store_true', help='measure the skip-connection architecture against the default one instead')
    ap.add_argument('--shared', action='store_true', help='measure the shared-net architecture against the default one instead')
    ap.add_argument('--gpus', type=int, default=1, help='with --opt: also measure data-parallel steps at world sizes up to this')
    ap.add_argument('--dp-rank', action='store_true', help=argparse.SUPPRESS)          # one rank of a --gpus measurement
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.out is None:
        name = ('train_dp_bench.json' if args.opt else 'train_power_bench.json' if args.power else 'train_varlen_bench.json' if args.varlen else 'train_tran_bench.json' if args.tran
                else 'train_skip_bench.json' if args.skip else 'train_shared_bench.json' if args.shared else 'train_bench.json')
        args.out = os.path.join(ROOT, 'profiles', name)
    steps, warmup = max(args.steps, 20), max(args.warmup, 3)

    import numpy as np
    import torch
    from oracle import iaf_oracle as O
    from pwv_amd import train as TR
    from pwv_amd.models import IAFVocoder
    from pwv_amd.variables import VariableStore
    from tests.util import set_hparams

    dev = torch.device('cuda', int(os.environ.get('LOCAL_RANK', '0')) if args.dp_rank else 0)
    torch.cuda.set_device(dev)
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
        geo = TR._Geometry(TR._Uniform(n, length, mel.shape[1]), TR._Projected(), sum(128 * len(net.dilations) for net in nets), 0)
        geo.cond.P = train_forward.P
        x = z.reshape(-1)
        for pair in flows:
            s = [TR._net_forward(net, geo, x) for net in pair]
            x = x * s[0][2] + s[1][2]

    cols = 128 * 2 * sum(len(d) for d in cfg.dilations)
    train_forward.P = torch.zeros((n * mel.shape[1], cols), dtype=torch.float32, device=dev)

    if args.dp_rank:
        return dp_rank(args, TR, model, wav, mel, z, steps, warmup)
    if args.opt:
        return opt_legs(args, TR, O, cfg, store, model, wav, mel, z, steps, warmup)
    if args.power:
        return power_legs(args, TR, model, wav, mel, z, steps, warmup)
    if args.varlen:
        return varlen_legs(args, TR, O, cfg, store, model, wav, mel, z, steps, warmup)
    if args.tran:
        return tran_legs(args, TR, O, cfg, store, model, wav, mel, z, steps, warmup)
    if args.skip:
        return skip_legs(args, TR, O, cfg, store, model, wav, mel, z, steps, warmup)
    if args.shared:
        return shared_legs(args, TR, O, cfg, store, model, wav, mel, z, steps, warmup)

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


def power_legs(args, TR, model, wav, mel, z, steps, warmup, weight=0.0005):
    import ctypes
    import torch
    from pwv_amd import _lib
    from pwv_amd.hparam import hparam as hp

    def once(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    variants = {'loss_and_grad_power': lambda: TR.loss_and_grad(model, wav, mel, z=z, power_weight=weight),
                'loss_and_grad_l1': lambda: TR.loss_and_grad(model, wav, mel, z=z)}
    ms = {k: [] for k in variants}
    for k in range(warmup + steps):
        for name, fn in variants.items():            # alternating: A B A B ...
            t = once(fn)
            if k >= warmup:
                ms[name].append(t)

    # the loss head alone, on the prediction of the model: 20 calls per timed window (one call is tens of microseconds)
    n, length = args.batch, args.length
    _, pred, _ = TR.loss_and_grad(model, wav, mel, z=z)
    pred, y = pred.reshape(-1).contiguous(), wav.reshape(-1).contiguous()
    win, hop = int(hp.signal.win_length), int(hp.signal.hop_length)
    lib, stream, calls = _lib.lib(), torch.cuda.current_stream().cuda_stream, 20
    head = {}
    for name, w in (('loss_head_power', weight), ('loss_head_l1', 0.0)):
        a = _lib.TrainLossArgs(out=pred.data_ptr(), y=y.data_ptr(), n=n, T=length, win_length=win, hop_length=hop, weight_l1=1.0, weight_power=w)
        need = int(lib.pwv_train_loss_workspace_bytes(ctypes.byref(a)))
        d_out = torch.empty(n * length, dtype=torch.float32, device=pred.device)
        table = torch.empty((n, 4), dtype=torch.float64, device=pred.device)
        work = torch.empty(need // 8, dtype=torch.float64, device=pred.device)
        a.d_out, a.result, a.workspace, a.workspace_bytes = d_out.data_ptr(), table.data_ptr(), work.data_ptr(), need

        def run(a=a):
            for _ in range(calls):
                _lib.check(lib.pwv_train_loss_f32(ctypes.byref(a), stream), 'pwv_train_loss_f32')

        head[name] = [once(run) / calls for k in range(warmup + steps)][warmup:]
    frames = 1 + (length - win) // hop
    nfft = 1
    while nfft < win:
        nfft *= 2
    out = {'model': 'default (4 flows, 10 + 10 + 10 + 30 layers, 2 nets each)', 'batch': n, 'length': length, 'steps': steps, 'warmup': warmup,
           'device': torch.cuda.get_device_name(0), 'power_weight': weight, 'win_length': win, 'hop_length': hop, 'frames_per_utterance': frames,
           'loss_head_f64_fma': n * frames * (4 * (nfft // 2) * win + 2 * (nfft // 2 + 1) * win)}
    for k, v in list(ms.items()) + list(head.items()):
        out[k + '_ms'] = {'median': round(statistics.median(v), 4), 'min': round(min(v), 4), 'max': round(max(v), 4)}
    out['power_minus_l1_ms'] = round(statistics.median(ms['loss_and_grad_power']) - statistics.median(ms['loss_and_grad_l1']), 4)
    out['paired_difference_ms'] = {'median': round(statistics.median(a - b for a, b in zip(ms['loss_and_grad_power'], ms['loss_and_grad_l1'])), 4)}
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps(out))


MIXED = [8000, 6400, 4800, 4000, 3200, 2400, 1600, 1600]       # sum 32000 = 8 x 4000; padded to the longest: 64000 rows


def varlen_legs(args, TR, O, cfg, store, model, wav, mel, z, steps, warmup):
    import numpy as np
    import torch
    from pwv_amd.models import IAFVocoder
    dev = wav.device
    n, length, hop = args.batch, args.length, cfg.hop_length
    assert sum(MIXED) == n * length and all(T % hop == 0 for T in MIXED), 'the mixed lengths are for --batch 8 --length 4000'

    def once(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    eq = ([wav[i] for i in range(n)], [mel[i] for i in range(n)], [z[i] for i in range(n)])
    longest = max(MIXED)
    mel_p, z_p = O.synthetic_inputs(n, longest, cfg, mel_seed=7, z_seed=8)
    wav_p = (0.3 * np.random.RandomState(9).randn(n, longest)).astype(np.float32)
    for i, T in enumerate(MIXED):                       # the padded batch: zeros behind every utterance's end
        wav_p[i, T:] = 0
    mel_p, z_p, wav_p = (torch.from_numpy(a).to(dev) for a in (mel_p, z_p, wav_p))
    mixed = ([wav_p[i, :T] for i, T in enumerate(MIXED)], [mel_p[i, :1 + T // hop] for i, T in enumerate(MIXED)],
             [z_p[i, :T] for i, T in enumerate(MIXED)])
    padded_model = IAFVocoder(batch_size=n, length=longest, store=store, precision='f32')
    variants = {'a_uniform_8x4000': lambda: TR.loss_and_grad(model, wav, mel, z=z),
                'b_packed_equal': lambda: TR.loss_and_grad_varlen(model, eq[0], eq[1], z=eq[2]),
                'c_packed_mixed': lambda: TR.loss_and_grad_varlen(model, mixed[0], mixed[1], z=mixed[2]),
                'd_uniform_padded_mixed': lambda: TR.loss_and_grad(padded_model, wav_p, mel_p, z=z_p)}
    ms = {k: [] for k in variants}
    for k in range(warmup + steps):
        for name, fn in variants.items():            # alternating: A B C D A B C D ...
            t = once(fn)
            if k >= warmup:
                ms[name].append(t)
    out = {'model': 'default (4 flows, 10 + 10 + 10 + 30 layers, 2 nets each)', 'batch': n, 'length': length, 'steps': steps, 'warmup': warmup,
           'device': torch.cuda.get_device_name(0), 'mixed_lengths': MIXED, 'rows_packed': sum(MIXED), 'rows_padded': n * longest}
    for k, v in ms.items():
        out[k + '_ms'] = {'median': round(statistics.median(v), 3), 'min': round(min(v), 3), 'max': round(max(v), 3)}
    med = {k: statistics.median(v) for k, v in ms.items()}
    out['b_over_a'] = round(med['b_packed_equal'] / med['a_uniform_8x4000'], 4)
    out['paired_b_minus_a_ms'] = {'median': round(statistics.median(b - a for a, b in zip(ms['a_uniform_8x4000'], ms['b_packed_equal'])), 3)}
    out['d_over_c'] = round(med['d_uniform_padded_mixed'] / med['c_packed_mixed'], 4)
    out['rows_padded_over_packed'] = round(n * longest / float(sum(MIXED)), 4)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps(out))


def tran_legs(args, TR, O, cfg, store, model, wav, mel, z, steps, warmup):
    import torch
    from pwv_amd.models import IAFVocoder
    from pwv_amd.variables import VariableStore
    from tests.util import set_hparams
    dev = wav.device
    n, length = args.batch, args.length
    tcfg = O.ModelConfig(cond_upsample_method='transposed_conv')
    set_hparams(tcfg)
    tstore = VariableStore(device=dev)
    tstore.load_dict(O.init_weights(tcfg, seed=2))
    tmodel = IAFVocoder(batch_size=n, length=length, store=tstore, precision='f32')

    def once(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    # the conditioning stages alone, on a fixed d_cond of the condition's shape
    mel2 = mel.reshape(-1, mel.shape[2]).contiguous()
    C = tcfg.condition_channels
    stages = TR._tconv_forward(tstore, mel2, C)
    d_cond = torch.randn(n, length + tcfg.hop_length, C, device=dev)
    variants = {'repeat': (cfg, lambda: TR.loss_and_grad(model, wav, mel, z=z)),
                'transposed_conv': (tcfg, lambda: TR.loss_and_grad(tmodel, wav, mel, z=z)),
                'cond_stages_forward': (tcfg, lambda: TR._tconv_forward(tstore, mel2, C)),
                'cond_stages_backward': (tcfg, lambda: TR._tconv_backward(stages, d_cond, {}))}
    ms = {k: [] for k in variants}
    for k in range(warmup + steps):
        for name, (c, fn) in variants.items():            # alternating: A B C D A B C D ...
            set_hparams(c)                                  # (outside the timed window)
            t = once(fn)
            if k >= warmup:
                ms[name].append(t)
    set_hparams(cfg)
    out = {'model': 'default (4 flows, 10 + 10 + 10 + 30 layers, 2 nets each)', 'batch': n, 'length': length, 'steps': steps, 'warmup': warmup,
           'device': torch.cuda.get_device_name(0), 'condition_channels': C, 'peak_allocated_MiB': round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)}
    for k, v in ms.items():
        key = 'loss_and_grad_%s_ms' % k if k in ('repeat', 'transposed_conv') else k + '_ms'
        out[key] = {'median': round(statistics.median(v), 3), 'min': round(min(v), 3), 'max': round(max(v), 3)}
    med = {k: statistics.median(v) for k, v in ms.items()}
    out['transposed_over_repeat'] = round(med['transposed_conv'] / med['repeat'], 4)
    out['paired_ratio'] = {'median': round(statistics.median(b / a for a, b in zip(ms['repeat'], ms['transposed_conv'])), 4)}
    out['cond_stages_share'] = round((med['cond_stages_forward'] + med['cond_stages_backward']) / med['transposed_conv'], 4)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps(out))


def skip_legs(args, TR, O, cfg, store, model, wav, mel, z, steps, warmup):
    import ctypes
    import torch
    from pwv_amd import _lib
    from tests.util import set_hparams
    dev = wav.device
    n, length = args.batch, args.length
    scfg = O.ModelConfig(use_skip_connection=True)          # the same variables: the two architectures differ in what they read

    def once(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    variants = {'default': (cfg, lambda: TR.loss_and_grad(model, wav, mel, z=z)),
                'skip': (scfg, lambda: TR.loss_and_grad(model, wav, mel, z=z, use_skip_connection=True))}
    ms = {k: [] for k in variants}
    for k in range(warmup + steps):
        for name, (c, fn) in variants.items():            # alternating: A B A B ...
            set_hparams(c)                                  # (outside the timed window)
            t = once(fn)
            if k >= warmup:
                ms[name].append(t)
    set_hparams(cfg)
    peak = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)

    # the residual layer-backward launch alone (kernel + reduction), both forms, on buffers of the step's size: 20 calls per window
    rows, frames, hop = n * length, mel.shape[1], cfg.hop_length
    kmax = (hop + 30) // 32 + 1
    t64 = lambda: torch.randn(((rows + 31) // 32) * 32 * 64, device=dev)
    x, u, v, un, vn = t64(), t64(), t64(), t64(), t64()
    dS = torch.randn(((rows + 31) // 32) * 32 * 128, device=dev)
    P, dP = 0.5 * torch.randn(n * frames, 128, device=dev), torch.zeros(n * frames * kmax, 128, device=dev)
    w = {k: 0.1 * torch.randn(*shape, device=dev) for k, shape in (('filter', (2, 64, 64)), ('gate', (2, 64, 64)), ('dense', (1, 64, 64)),
                                                                   ('skip', (1, 64, 128)))}
    d = {k: torch.empty_like(t) for k, t in w.items()}
    d['dense_bias'] = torch.empty(64, device=dev)
    base = dict(N=n, T=length, cond_hop=hop, cond_offset=hop // 2, cond_frames=frames, proj_row_stride=128, d_proj_row_stride=128, dilation=1,
                next_dilation=1, form=_lib.TRAIN_RESIDUAL)
    lib, stream, calls = _lib.lib(), torch.cuda.current_stream().cuda_stream, 20
    ws = torch.empty(lib.pwv_train_skip_workspace_bytes(ctypes.byref(_lib.TrainSkipArgs(**base))) // 4, device=dev)
    ptrs = dict(x=x, proj=P, filter=w['filter'], gate=w['gate'], dense=w['dense'], u_next=un, v_next=vn, u=u, v=v, d_proj=dP,
                d_filter=d['filter'], d_gate=d['gate'], d_dense=d['dense'], d_dense_bias=d['dense_bias'], workspace=ws)
    ptrs = {k: t.data_ptr() for k, t in ptrs.items()}
    plain = _lib.TrainArgs(workspace_bytes=ws.numel() * 4, **base, **ptrs)
    skip = _lib.TrainSkipArgs(workspace_bytes=ws.numel() * 4, skip=w['skip'].data_ptr(), d_skip_sum=dS.data_ptr(), d_skip=d['skip'].data_ptr(),
                              **base, **ptrs)
    launches = (('layer_bwd_default', 'pwv_train_layer_bwd_f32', plain), ('layer_bwd_skip', 'pwv_train_skip_layer_bwd_f32', skip))
    ms.update({name: [] for name, _, _ in launches})
    for k in range(warmup + steps):                         # alternating windows of 20 calls
        for name, entry, a in launches:
            def run(entry=entry, a=a):
                for _ in range(calls):
                    _lib.check(getattr(lib, entry)(ctypes.byref(a), stream), entry)
            t = once(run) / calls
            if k >= warmup:
                ms[name].append(t)
    out = {'model': 'default (4 flows, 10 + 10 + 10 + 30 layers, 2 nets each)', 'batch': n, 'length': length, 'steps': steps, 'warmup': warmup,
           'device': torch.cuda.get_device_name(0), 'peak_allocated_MiB': peak}
    for k, vals in ms.items():
        key = 'loss_and_grad_%s_ms' % k if k in variants else k + '_ms'
        out[key] = {'median': round(statistics.median(vals), 4), 'min': round(min(vals), 4), 'max': round(max(vals), 4)}
    med = {k: statistics.median(vals) for k, vals in ms.items()}
    out['skip_over_default'] = round(med['skip'] / med['default'], 4)
    out['paired_ratio'] = {'median': round(statistics.median(b / a for a, b in zip(ms['default'], ms['skip'])), 4)}
    out['layer_bwd_skip_over_default'] = round(med['layer_bwd_skip'] / med['layer_bwd_default'], 4)
    out['layer_bwd_estimate_by_operation_count'] = 1.25
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps(out))


def shared_legs(args, TR, O, cfg, store, model, wav, mel, z, steps, warmup):
    import ctypes
    import torch
    from pwv_amd import _lib
    from pwv_amd.models import IAFVocoder
    from pwv_amd.variables import VariableStore
    from tests.util import set_hparams
    dev = wav.device
    n, length = args.batch, args.length
    scfg = O.ModelConfig(shared_nets=True)                  # bench/c2: one net per flow, variables of its own
    set_hparams(scfg)
    sstore = VariableStore(device=dev)
    sstore.load_dict(O.init_weights(scfg, seed=2))
    smodel = IAFVocoder(batch_size=n, length=length, store=sstore, precision='f32')

    def once(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    variants = {'default': (cfg, lambda: TR.loss_and_grad(model, wav, mel, z=z)),
                'shared': (scfg, lambda: TR.loss_and_grad(smodel, wav, mel, z=z, shared_nets=True))}
    ms = {k: [] for k in variants}
    for k in range(warmup + steps):
        for name, (c, fn) in variants.items():            # alternating: A B A B ...
            set_hparams(c)                                  # (outside the timed window)
            t = once(fn)
            if k >= warmup:
                ms[name].append(t)
    set_hparams(cfg)
    peak = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)

    # the head backward launch alone (kernel + reduction), one output against two, on buffers of the step's size: 20 calls per window
    rows = n * length
    o, d_o = (torch.randn(((rows + 31) // 32) * 32 * 64, device=dev) for _ in range(2))
    d_out, d_mul = torch.randn(rows, device=dev), torch.randn(rows, device=dev)
    shapes = (('skip', (1, 64, 128)), ('skip_bias', (128,)), ('post1', (1, 128, 128)), ('post1_bias', (128,)))
    w = {k: 0.1 * torch.randn(*shape, device=dev) for k, shape in shapes + (('post2', (1, 128, 2)), ('post2_bias', (2,)))}
    d = {k: torch.empty_like(t) for k, t in w.items()}
    lib, stream, calls = _lib.lib(), torch.cuda.current_stream().cuda_stream, 20
    ws = torch.empty(lib.pwv_train_shared_workspace_bytes(ctypes.byref(_lib.TrainSharedArgs(N=n, T=length))) // 4, device=dev)
    ptrs = dict(x=o, d_out=d_out, d_mul=d_mul, d_o_out=d_o, workspace=ws, **w, **{'d_' + k: t for k, t in d.items()})
    ptrs = {k: t.data_ptr() for k, t in ptrs.items()}
    one = _lib.TrainArgs(N=n, T=length, workspace_bytes=ws.numel() * 4, **ptrs)      # (reads column 0 of post2 alone: 128 of its floats)
    two = _lib.TrainSharedArgs(N=n, T=length, workspace_bytes=ws.numel() * 4, head_in=_lib.TRAIN_HEAD_IN_GATED, **ptrs)
    launches = (('head_bwd_default', 'pwv_train_head_bwd_f32', one), ('head_bwd_shared', 'pwv_train_shared_head_bwd_f32', two))
    ms.update({name: [] for name, _, _ in launches})
    for k in range(warmup + steps):                         # alternating windows of 20 calls
        for name, entry, a in launches:
            def run(entry=entry, a=a):
                for _ in range(calls):
                    _lib.check(getattr(lib, entry)(ctypes.byref(a), stream), entry)
            t = once(run) / calls
            if k >= warmup:
                ms[name].append(t)
    out = {'model': 'default (4 flows, 10 + 10 + 10 + 30 layers, 2 nets each) against shared_nets (1 net each)', 'batch': n, 'length': length,
           'steps': steps, 'warmup': warmup, 'device': torch.cuda.get_device_name(0), 'peak_allocated_MiB': peak}
    for k, vals in ms.items():
        key = 'loss_and_grad_%s_ms' % k if k in variants else k + '_ms'
        out[key] = {'median': round(statistics.median(vals), 4), 'min': round(min(vals), 4), 'max': round(max(vals), 4)}
    med = {k: statistics.median(vals) for k, vals in ms.items()}
    out['shared_over_default'] = round(med['shared'] / med['default'], 4)
    out['paired_ratio'] = {'median': round(statistics.median(b / a for a, b in zip(ms['default'], ms['shared'])), 4)}
    out['head_bwd_shared_over_default'] = round(med['head_bwd_shared'] / med['head_bwd_default'], 4)
    out['estimate_by_operation_count'] = 0.5
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps(out))


def opt_legs(args, TR, O, cfg, store, model, wav, mel, z, steps, warmup):
    import subprocess
    import torch
    from pwv_amd.models import IAFVocoder
    from pwv_amd.variables import VariableStore
    dev = wav.device
    n, length = args.batch, args.length

    def once(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    store2 = VariableStore(device=dev)
    store2.load_dict(O.init_weights(cfg, seed=2))
    model2 = IAFVocoder(batch_size=n, length=length, store=store2, precision='f32')
    unfused, fused = TR.Trainer(model), TR.Trainer(model2, fused=True)
    variants = {'trainer_step_unfused': lambda: unfused.step(wav, mel, z=z), 'trainer_step_fused': lambda: fused.step(wav, mel, z=z)}
    ms = {k: [] for k in variants}
    for k in range(warmup + steps):
        for name, fn in variants.items():            # alternating: A B A B ...
            t = once(fn)
            if k >= warmup:
                ms[name].append(t)

    # the launches alone, on the gradients of one step: 20 calls per timed window
    _, _, grads = TR.loss_and_grad(model2, wav, mel, z=z)
    ar, calls = fused.arenas, 20
    vars1 = [store.vars[k] for k in unfused.names]
    glist, state = [grads[k] for k in unfused.names], [None]

    def foreach():
        state[0] = TR.adam_ema_update(vars1, glist, state[0], unfused.lr, unfused.beta1, unfused.beta2, TR.ADAM_EPS, unfused.ema_decay)

    alone = {'pack': lambda: ar.pack_grads(grads), 'adam_ema': lambda: ar.adam_ema(1e-4, 0.9, 0.999, 1e-8, 0.998, 1.0),
             'unpack': lambda: ar.pack(ar.vars, ar.shadow, unpack=True), 'foreach_update': foreach}
    for name, fn in alone.items():
        def run(fn=fn):
            for _ in range(calls):
                fn()
        ms[name] = [once(run) / calls for k in range(warmup + steps)][warmup:]
    lay = ar.layout
    out = {'model': 'default (4 flows, 10 + 10 + 10 + 30 layers, 2 nets each)', 'batch': n, 'length': length, 'steps': steps, 'warmup': warmup,
           'device': torch.cuda.get_device_name(0), 'variables': len(lay.names), 'arena_floats': lay.total,
           'parameters': sum(lay.counts), 'packed_tensors': ar._grad_tables[2].n, 'blocks': ar.vars.blocks,
           'adam_ema_bytes': 4 * sum(lay.counts) * 9}
    for k, v in ms.items():
        out[k + '_ms'] = {'median': round(statistics.median(v), 4), 'min': round(min(v), 4), 'max': round(max(v), 4)}
    out['fused_minus_unfused_ms'] = {'median': round(statistics.median(b - a for a, b in zip(ms['trainer_step_unfused'], ms['trainer_step_fused'])), 4)}
    out['adam_ema_GBps'] = round(out['adam_ema_bytes'] / (statistics.median(ms['adam_ema']) * 1e-3) / 1e9, 1)

    # data-parallel steps: N fresh processes per world size, one per GPU
    visible = torch.cuda.device_count()
    out['visible_devices'] = visible
    out['data_parallel'] = {}
    for world in (1, 2, 4, 8):
        if world > min(args.gpus, visible):
            continue
        import socket
        s = socket.socket()
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
        s.close()
        procs = []
        for r in range(world):
            env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
            cmd = [sys.executable, os.path.abspath(__file__), '--dp-rank', '--steps', str(steps), '--warmup', str(warmup), '--batch', str(n),
                   '--length', str(length)]
            procs.append(subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL, text=True))
        text, _ = procs[0].communicate(timeout=900)
        codes = [p.wait(timeout=60) for p in procs]
        if any(codes):
            raise SystemExit('a rank of the world size %d measurement exited with %r' % (world, codes))
        out['data_parallel'][str(world)] = json.loads([l for l in text.splitlines() if l.startswith('{')][-1])
    if visible < 2 or args.gpus < 2:
        out['scaling'] = 'unmeasured: %d device(s) visible, --gpus %d' % (visible, args.gpus)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps(out))


def dp_rank(args, TR, model, wav, mel, z, steps, warmup):
    """One rank of a data-parallel measurement: DataParallelTrainer.step on this rank's batch and the all-reduce of the gradient arena
    alone; every figure is the MAX over the ranks of the ranks' medians.  Rank 0 prints one JSON line."""
    import torch
    import torch.distributed as dist
    dev = wav.device
    dist.init_process_group(backend='nccl', device_id=dev)
    try:
        tr = TR.DataParallelTrainer(model)

        def once(fn):
            torch.cuda.synchronize()
            dist.barrier()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)

        step = [once(lambda: tr.step(wav, mel, z=z)) for k in range(warmup + steps)][warmup:]
        calls = 20

        def reduce():
            for _ in range(calls):
                TR.allreduce_sum_(tr.arenas.grad, tr.group)

        alone = [once(reduce) / calls for k in range(warmup + steps)][warmup:]
        meds = torch.tensor([statistics.median(step), statistics.median(alone)], dtype=torch.float64, device=dev)
        dist.all_reduce(meds, op=dist.ReduceOp.MAX)
        res = {'world': tr.world, 'backend': dist.get_backend(), 'per_rank_batch': args.batch, 'step_ms': round(float(meds[0]), 3),
               'allreduce_ms': round(float(meds[1]), 4), 'arena_MB': round(4 * tr.arenas.grad.numel() / 1e6, 2)}
    finally:
        dist.destroy_process_group()
    if tr.rank == 0:
        print(json.dumps(res))


if __name__ == '__main__':
    main()
