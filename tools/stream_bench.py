"""Streaming against overlap-and-discard ("Streaming"): what one TICK of a server costs that advances
`sessions` sessions by `chunk` samples each, default model (or --case: 'bench/c2' = the shared-net architecture, one two-output net per
flow, at the default dilations; 'bench/c5' = transposed-conv conditioning, whose stream is per-layer launches with the condition GEMM
inside -- its `stream` leg is that route and there is no `stream_layers` leg; the graph modes refuse it; 'bench/skip' = the skip-connection
architecture, whose stream is a streaming front, per-layer launches on per-chunk skip accumulators and the head launch -- one route, no
`stream_layers` leg and no graph modes either), random weights, one GPU, steady state (every session has emitted more
than timeshard.chain_halo samples).

Legs of a cell (sessions x chunk):
  stream    StreamingVocoder.push of all slots: sessions x chunk rows, one persistent streaming launch per flow (engine.run_flow_stream's
            default route; the cell's `launches` says what an untimed push enqueued)
  stream_layers  the same push with engine.PERSIST = False: the streaming per-layer kernels, L launches per flow + the affine
  overlap   the same new samples through the one-shot API only: one uniform forward IAFVocoder(sessions, chunk + chain_halo), the
            first chain_halo samples discarded (timeshard.py: exact) -- code that runs unchanged without the streaming feature
  rows      sessions x chunk rows as a plain uniform forward IAFVocoder(sessions, chunk): what the kept rows alone cost (the floor;
            its audio is the one-shot left edge, not a continuation)
A tick = the leg's launches enqueued (verify=False, explicit z) and ONE synchronisation; `ms` is the median over --steps ticks after
--warmup ticks, `enqueue_ms` the median host time up to the synchronisation.  The legs of a cell run one after the other in the
same process, the whole round twice ('ms' holds both medians: their difference is the spread).  Per cell, from engine.EVENT_LOG and a
count of the library's launch calls in one untimed push per streaming leg: `launches` = {leg: {calls, per-flow routes, short-input
instantiation per persistent launch}}.  Prints one JSON line.

    python tools/stream_bench.py [--case default] [--steps 20] [--warmup 5] [--precision f16x3] [--sessions 1,8,32] [--chunks 800,1600,8000]

--ragged ("Ragged pushes"): a tick whose sessions get DIFFERENT numbers of frames.  Cells: S = 8 and 32 running
sessions, session i given 800 * (1 + i % 4) samples (four distinct lengths, R = 2000 S rows), and one "utterance ends" cell: 31 x 1600
and 1 x 80.  Legs, same protocol (verify=False, one synchronisation at the end of the tick, median of --steps after --warmup, the round
twice):
  ragged    ONE push_varlen of all sessions
  grouped   what a caller did before push_varlen: one push per distinct length (the API settles a push before the next: verify=False
            and verify() per group; the last verify() is the tick's synchronisation)
  uniform   one push of S sessions x the mean length (rounded up to a frame): about the same rows without raggedness, the floor
`ragged_over_grouped` / `ragged_over_uniform` per round, and `spread` = the largest difference between the two medians of a leg.

    python tools/stream_bench.py --ragged [--steps 20] [--warmup 5] [--precision f16x3]

--graph ("Graph replay of a streaming tick"): the tick as ONE graph replay with the commit on the device
(StreamingVocoder.graphed).  Cells (sessions x chunk): 1 x 800, 1 x 1600, 2 x 800, 8 x 800, 32 x 1600.  Legs, same protocol (explicit z,
one synchronisation per tick, median of --steps after --warmup, the legs of a cell one after the other in one process, the round twice):
  stream           the eager push(verify=False) + verify(): the baseline, unchanged code
  graph            one tick() + verify()
  graph_pipelined  8 ticks enqueued back to back (no host synchronisation between them, the default depth of 4 ticks in flight), one
                   verify(), divided by 8
  overlap          overlap-and-discard, as above
`spread` = the largest difference between the two medians of a leg; `graph_not_slower_than_stream`: graph <= stream + spread in both
rounds.  `graph_over_stream`, `graph_pipelined_over_stream`, `overlap_over_graph` per round.

    python tools/stream_bench.py --graph [--steps 20] [--warmup 5] [--precision f16x3]

--ragged-graph ("Graph replay of a ragged tick"): the ragged tick as ONE graph replay with the frame counts and the
commit on the device (StreamingVocoder.graphed_varlen).  The three cells of --ragged, each captured at exactly its sessions and rows.
Legs, same protocol (explicit z, one synchronisation per tick, median of --steps after --warmup, the legs of a cell one after the other
in one process, the round twice):
  ragged                  the eager push_varlen(verify=False) + verify(): the baseline, unchanged code
  ragged_graph            one tick() + verify()
  ragged_graph_varying    one tick() + verify() where consecutive ticks differ in their frame counts (two sessions exchange theirs) and
                          z comes as a list of pieces: the entries are uploaded with every tick, as on a server whose counts change
  ragged_graph_pipelined  8 ticks enqueued back to back, one verify(), divided by 8
  uniform                 one push of S sessions x the mean length, as in --ragged
On the mixed cells a CHURN leg besides: in every tick one session ends and another starts on its slot, `churn_sync` with verify(), reset
and the eager one-frame push in front of the tick (the protocol without starts), `churn_starts` with tick(starts=);
`starts_not_slower_than_sync`: churn_starts <= churn_sync + spread in both rounds.
`spread` = the largest difference between the two medians of a leg; `graph_not_slower_than_ragged`: ragged_graph <= ragged + spread in
both rounds (`ragged_graph`, whose ticks repeat one table, is the graph's best case: see ragged_graph_varying).

    python tools/stream_bench.py --ragged-graph [--steps 20] [--warmup 5] [--precision f16x3]

--live ("Streaming the mel front-end"): what the streaming front-end (audio_frontend.StreamingMel) adds to a tick.
One cell: 8 running sessions x 10 frames (800 samples each).  Legs, same protocol (explicit z, one synchronisation per tick, median of
--steps after --warmup, the legs one after the other in one process, the round twice):
  vocoder    push_varlen(verify=False) of 8 x 10 ready-made frames + verify(): the tick without a front-end
  live       StreamingMel.push of 8 x 800 samples, its 8 x 10 frames into the same push_varlen + verify(): wav chunks in, wav chunks out
  live_graph the same tick as ONE graph launch (StreamingVocoder.graphed_live: front-end, ragged tick and both commits on the device) +
             verify(); `live_graph_below_live`: every live_graph median is below every live median of the run
  frontend   StreamingMel.push alone + a synchronisation
  one_shot   wav_to_mel_device on the same [8, 800] samples + a synchronisation: the whole-utterance kernel on a tick's worth (11 frames
             each, both edges reflected -- not the frames of a stream)
`spread` = the largest difference between the two medians of a leg; `live_over_vocoder` per round.

    python tools/stream_bench.py --live [--steps 20] [--warmup 5] [--precision f16x3]
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
    ap.add_argument('--sessions', default='1,8,32')
    ap.add_argument('--chunks', default='800,1600,8000')
    ap.add_argument('--ragged', action='store_true', help='the ragged-tick cells (push_varlen against grouped pushes) instead of the default legs')
    ap.add_argument('--graph', action='store_true', help='the graphed-tick cells (StreamingVocoder.graphed against the eager push) instead of the default legs')
    ap.add_argument('--ragged-graph', action='store_true',
                    help='the ragged-tick cells as graph replays (StreamingVocoder.graphed_varlen against the eager push_varlen) instead of the default legs')
    ap.add_argument('--live', action='store_true', help='the streaming mel front-end in front of push_varlen (audio_frontend.StreamingMel) instead of the default legs')
    ap.add_argument('--case', default='default', help="the hparams case whose model streams: 'default', 'bench/c2' for the shared-net "
                    "architecture (one two-output net per flow), 'bench/c5' for transposed-conv conditioning, 'bench/skip' for the skip-connection "
                    "architecture; the result line names it")
    args = ap.parse_args()

    import numpy as np
    import torch
    from oracle import iaf_oracle as O
    from pwv_amd import _lib, engine
    from pwv_amd.models import IAFVocoder
    from pwv_amd.timeshard import chain_halo
    from pwv_amd.variables import VariableStore
    from pwv_amd.hparam import hparam as hp
    from tests.util import set_hparams

    dev = torch.device('cuda', 0)
    hp.set_hparam_yaml(args.case)
    cfg = O.ModelConfig.from_hparam(hp)
    set_hparams(cfg)
    store = VariableStore(device=dev)
    store.load_dict(O.init_weights(cfg, seed=2))
    hop = cfg.hop_length
    halo = chain_halo(cfg.dilations, cfg.filter_width, cfg.n_iaf, hop)
    rng = np.random.default_rng(0)

    # a transposed-conv case ('bench/c5') makes the request for its streaming form: per-layer launches with the condition GEMM inside
    per_sample = cfg.cond_upsample_method == 'transposed_conv'
    # ... and a skip-connection case ('bench/skip') for its own: the front, per-layer launches on the chunk's skip accumulators, the head
    skip = bool(cfg.use_skip_connection)

    def open_stream(model, slots):
        return model.open_stream(slots=slots, transposed_conv=per_sample, use_skip_connection=skip)

    def rand(*shape):
        return torch.from_numpy(rng.uniform(-1, 1, shape).astype(np.float32)).to(dev)

    def timed(fn, sync):
        host, total = [], []
        for k in range(args.warmup + args.steps):
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()
            sync()
            t2 = time.perf_counter()
            if k >= args.warmup:
                host.append((t1 - t0) * 1e3)
                total.append((t2 - t0) * 1e3)
        return statistics.median(total), statistics.median(host)

    persist_default, real_lib = engine.PERSIST, _lib.lib
    # library calls that enqueue nothing (sizes, plans, error text)
    NOT_LAUNCHES = ('pwv_persist_workspace_bytes', 'pwv_persist_short_input', 'pwv_tile32_floats', 'pwv_last_error', 'pwv_version',
                    'pwv_layer_packed_floats', 'pwv_head_packed_floats', 'pwv_persist_status', 'pwv_status_words_alloc')

    def counting(calls):
        lib = real_lib()

        class Counting(object):
            def __getattr__(self, name):
                fn = getattr(lib, name)
                if not name.startswith('pwv_'):
                    return fn

                def wrapped(*a):
                    calls.append(name)
                    return fn(*a)
                return wrapped
        return Counting()

    if args.live:
        from pwv_amd.audio_frontend import StreamingMel, wav_to_mel_device
        S, frames = 8, 10
        chunk = frames * hop
        out = {'mode': 'live', 'case': args.case, 'precision': args.precision, 'steps': args.steps, 'warmup': args.warmup, 'sessions': S, 'frames': frames, 'chunk': chunk}
        model = IAFVocoder(batch_size=S, length=hop, store=store, precision=args.precision)
        stream = open_stream(model, S)
        warm = -(-(halo + hop) // hop) * hop
        stream.push(rand(S, warm // hop + 1, cfg.n_mels), z=rand(S, warm, 1))        # steady state: every session running
        fe = StreamingMel(S)
        fe.push(list(0.5 * rand(S, chunk)))                                           # steady state: every later 800 samples bring 10 frames
        wav = 0.5 * rand(S, chunk)
        chunks, mels, zs = list(wav), [rand(frames, cfg.n_mels) for _ in range(S)], [rand(chunk, 1) for _ in range(S)]
        assert [int(m.shape[0]) for m in fe.push(chunks)] == [frames] * S

        # the live tick as ONE graph launch (graph.GraphedLiveStream), on a stream and a front-end of its own in the same steady state; a
        # slot and a filler's rows to spare, so that the tick of all 8 sessions replays
        from pwv_amd.graph import packed_filler_rows
        stream_g, fe_g = open_stream(model, S + 1), StreamingMel(S + 1)
        stream_g.push(rand(S, warm // hop + 1, cfg.n_mels), slots=list(range(S)), z=rand(S, warm, 1))
        fe_g.push(list(0.5 * rand(S, chunk)), slots=list(range(S)))
        live = stream_g.graphed_live(fe_g, S, S * chunk + packed_filler_rows(hop), sample=False)
        assert [int(o.shape[0]) for o in live.tick(chunks, list(range(S)), z=zs)] == [chunk] * S and live.verify() == 1 and live.eager_calls == 0

        legs = {
            'vocoder': (lambda: stream.push_varlen(mels, z=zs, verify=False), stream.verify),
            'live': (lambda: stream.push_varlen(fe.push(chunks), z=zs, verify=False), stream.verify),
            'live_graph': (lambda: live.tick(chunks, list(range(S)), z=zs), live.verify),
            'frontend': (lambda: fe.push(chunks), torch.cuda.synchronize),
            'one_shot': (lambda: wav_to_mel_device(wav), torch.cuda.synchronize),
        }
        for leg in legs:
            out[leg] = {'ms': [], 'enqueue_ms': []}
        for _ in range(2):
            for leg, (fn, sync) in legs.items():
                ms, host = timed(fn, sync)
                out[leg]['ms'].append(round(ms, 4))
                out[leg]['enqueue_ms'].append(round(host, 4))
        fe.verify()
        out['state_bytes_per_session'] = fe.state_bytes()
        out['spread'] = round(max(abs(out[leg]['ms'][0] - out[leg]['ms'][1]) for leg in legs), 4)
        out['live_over_vocoder'] = [round(a / b, 3) for a, b in zip(out['live']['ms'], out['vocoder']['ms'])]
        out['live_minus_vocoder_ms'] = [round(a - b, 4) for a, b in zip(out['live']['ms'], out['vocoder']['ms'])]
        out['live_graph_over_live'] = [round(a / b, 3) for a, b in zip(out['live_graph']['ms'], out['live']['ms'])]
        out['live_graph_below_live'] = max(out['live_graph']['ms']) < min(out['live']['ms'])          # every median below every median
        out['live_graph_eager_calls'], out['live_graph_captures'] = live.eager_calls, live.captures
        print(json.dumps(out))
        return

    if args.ragged:
        out = {'mode': 'ragged', 'case': args.case, 'precision': args.precision, 'steps': args.steps, 'warmup': args.warmup, 'cells': []}
        cells = [('mixed_%d' % S, [800 * (1 + i % 4) for i in range(S)]) for S in (8, 32)] + [('utterance_ends', [1600] * 31 + [80])]
        for name, lens in cells:
            S = len(lens)
            model = IAFVocoder(batch_size=S, length=hop, store=store, precision=args.precision)
            stream = open_stream(model, S)
            warm = -(-(halo + hop) // hop) * hop
            stream.push(rand(S, warm // hop + 1, cfg.n_mels), z=rand(S, warm, 1))        # steady state: every session running
            mels, zs = [rand(T // hop, cfg.n_mels) for T in lens], [rand(T, 1) for T in lens]
            groups = {}
            for i, T in enumerate(lens):
                groups.setdefault(T, []).append(i)
            grouped = [(members, torch.stack([mels[i] for i in members]), torch.stack([zs[i] for i in members])) for members in groups.values()]
            mean = -(-sum(lens) // (S * hop)) * hop
            mel_u, z_u = rand(S, mean // hop, cfg.n_mels), rand(S, mean, 1)

            def push_grouped():
                for k, (members, mel_g, z_g) in enumerate(grouped):
                    if k:
                        stream.verify()
                    stream.push(mel_g, slots=members, z=z_g, verify=False)

            legs = {
                'ragged': (lambda: stream.push_varlen(mels, z=zs, verify=False), stream.verify),
                'grouped': (push_grouped, stream.verify),
                'uniform': (lambda: stream.push(mel_u, z=z_u, verify=False), stream.verify),
            }
            cell = {'cell': name, 'sessions': S, 'lengths': sorted(groups), 'rows': sum(lens), 'uniform_rows': S * mean, 'groups': len(groups),
                    'launches': {}}
            for leg in legs:        # one untimed tick per leg: what it enqueues
                log, calls = [], []
                engine.EVENT_LOG, _lib.lib = log, (lambda: counting(calls))
                try:
                    legs[leg][0]()
                    legs[leg][1]()
                finally:
                    engine.EVENT_LOG, _lib.lib = None, real_lib
                cell['launches'][leg] = {'calls': len([c for c in calls if c not in NOT_LAUNCHES]),
                                         'flows': [e[0] + ('_' + e[3] if e[0] == 'stream_ragged' else '_stream' if len(e) > 8 and e[8] else '') for e in log],
                                         'short_input': [e[7] for e in log if e[0] == 'persist']}
            for leg in legs:
                cell[leg] = {'ms': [], 'enqueue_ms': []}
            for _ in range(2):
                for leg, (fn, sync) in legs.items():
                    ms, host = timed(fn, sync)
                    cell[leg]['ms'].append(round(ms, 3))
                    cell[leg]['enqueue_ms'].append(round(host, 3))
            cell['spread'] = round(max(abs(cell[leg]['ms'][0] - cell[leg]['ms'][1]) for leg in legs), 3)
            cell['ragged_over_grouped'] = [round(a / b, 3) for a, b in zip(cell['ragged']['ms'], cell['grouped']['ms'])]
            cell['ragged_over_uniform'] = [round(a / b, 3) for a, b in zip(cell['ragged']['ms'], cell['uniform']['ms'])]
            cell['ragged_not_slower_than_grouped'] = all(a <= b + cell['spread'] for a, b in zip(cell['ragged']['ms'], cell['grouped']['ms']))
            out['cells'].append(cell)
            print('# %s' % json.dumps(cell), file=sys.stderr)
        print(json.dumps(out))
        return

    if args.ragged_graph:
        out = {'mode': 'ragged_graph', 'case': args.case, 'precision': args.precision, 'steps': args.steps, 'warmup': args.warmup, 'pipelined_ticks': 8, 'cells': []}
        cells = [('mixed_%d' % S, [800 * (1 + i % 4) for i in range(S)]) for S in (8, 32)] + [('utterance_ends', [1600] * 31 + [80])]
        for name, lens in cells:
            S = len(lens)
            model = IAFVocoder(batch_size=S, length=hop, store=store, precision=args.precision)
            stream = open_stream(model, S)
            warm = -(-(halo + hop) // hop) * hop
            stream.push(rand(S, warm // hop + 1, cfg.n_mels), z=rand(S, warm, 1))        # steady state: every session running
            graphed = stream.graphed_varlen(S, sum(lens), sample=False)
            slots = list(range(S))
            mels, zs = [rand(T // hop, cfg.n_mels) for T in lens], [rand(T, 1) for T in lens]
            z_packed = torch.cat(zs)
            mean = -(-sum(lens) // (S * hop)) * hop
            mel_u, z_u = rand(S, mean // hop, cfg.n_mels), rand(S, mean, 1)

            # the same tick with the first and the last session's counts exchanged: alternating the two, every tick uploads its entries
            lens_b = [lens[-1]] + lens[1:-1] + [lens[0]]
            mels_b, zs_b = [rand(T // hop, cfg.n_mels) for T in lens_b], [rand(T, 1) for T in lens_b]
            flip = [0]

            def pipelined():
                for _ in range(8):
                    graphed.tick(mels, slots, z=z_packed)

            def varying():
                flip[0] ^= 1
                graphed.tick(mels_b if flip[0] else mels, slots, z=zs_b if flip[0] else zs)

            legs = {
                'ragged': (lambda: stream.push_varlen(mels, z=zs, verify=False), stream.verify, 1),
                'ragged_graph': (lambda: graphed.tick(mels, slots, z=z_packed), graphed.verify, 1),
                'ragged_graph_varying': (varying, graphed.verify, 1),
                'ragged_graph_pipelined': (pipelined, graphed.verify, 8),
                'uniform': (lambda: stream.push(mel_u, z=z_u, verify=False), stream.verify, 1),
            }
            cell = {'cell': name, 'sessions': S, 'lengths': sorted(set(lens)), 'rows': sum(lens), 'uniform_rows': S * mean}
            for leg in legs:
                cell[leg] = {'ms': [], 'enqueue_ms': []}
            for _ in range(2):
                for leg, (fn, sync, ticks) in legs.items():
                    ms, host = timed(fn, sync)
                    cell[leg]['ms'].append(round(ms / ticks, 4))
                    cell[leg]['enqueue_ms'].append(round(host / ticks, 4))
            assert graphed.captures == 1 and graphed.eager_calls == 0
            n_ticks = args.warmup + args.steps
            assert stream.emitted(0) == warm + 2 * n_ticks * (10 * lens[0] + mean) + n_ticks * (lens[0] + lens_b[0])       # (varying: 2 n ticks, half of each)
            if name.startswith('mixed_'):
                # CHURN: in every tick one session ends and another starts on its slot (the slots in turn), the tick's rows unchanged
                firsts = [rand(1, cfg.n_mels) for _ in lens]
                began = [[torch.cat([firsts[i], m]) if i == r else m for i, m in enumerate(mels)] for r in range(S)]
                turn, empty = [0], z_packed[:0]

                def churn_sync():          # the protocol without starts: settle, reset, the eager one-frame push, then the tick
                    r = turn[0] = (turn[0] + 1) % S
                    graphed.verify()
                    stream.reset(r)
                    stream.push_varlen([firsts[r]], slots=[r], z=[empty])
                    graphed.tick(mels, slots, z=z_packed)

                def churn_starts():
                    r = turn[0] = (turn[0] + 1) % S
                    graphed.tick(began[r], slots, z=z_packed, starts={r: None})

                churn = {'churn_sync': churn_sync, 'churn_starts': churn_starts}
                for leg in churn:
                    cell[leg] = {'ms': [], 'enqueue_ms': []}
                for _ in range(2):
                    for leg, fn in churn.items():
                        ms, host = timed(fn, graphed.verify)
                        cell[leg]['ms'].append(round(ms, 4))
                        cell[leg]['enqueue_ms'].append(round(host, 4))
                assert graphed.captures == 1 and graphed.eager_calls == 0
                legs = dict(legs, **churn)
            cell['spread'] = round(max(abs(cell[leg]['ms'][0] - cell[leg]['ms'][1]) for leg in legs), 4)
            ratio = lambda a, b: [round(x / y, 3) for x, y in zip(cell[a]['ms'], cell[b]['ms'])]      # noqa: E731
            if 'churn_starts' in cell:
                cell['starts_over_sync'] = ratio('churn_starts', 'churn_sync')
                cell['starts_not_slower_than_sync'] = all(a <= b + cell['spread'] for a, b in zip(cell['churn_starts']['ms'], cell['churn_sync']['ms']))
            cell['graph_over_ragged'] = ratio('ragged_graph', 'ragged')
            cell['graph_pipelined_over_ragged'] = ratio('ragged_graph_pipelined', 'ragged')
            cell['graph_over_uniform'] = ratio('ragged_graph', 'uniform')
            cell['graph_not_slower_than_ragged'] = all(g <= e + cell['spread'] for g, e in zip(cell['ragged_graph']['ms'], cell['ragged']['ms']))
            out['cells'].append(cell)
            print('# %s' % json.dumps(cell), file=sys.stderr)
        print(json.dumps(out))
        return

    if args.graph:
        out = {'mode': 'graph', 'case': args.case, 'precision': args.precision, 'steps': args.steps, 'warmup': args.warmup, 'chain_halo': halo, 'pipelined_ticks': 8,
               'cells': []}
        for S, chunk in ((1, 800), (1, 1600), (2, 800), (8, 800), (32, 1600)):
            model = IAFVocoder(batch_size=S, length=chunk, store=store, precision=args.precision)
            stream = open_stream(model, S)
            warm = -(-(halo + hop) // hop) * hop
            stream.push(rand(S, warm // hop + 1, cfg.n_mels), z=rand(S, warm, 1))        # steady state: emitted > chain_halo
            graphed = stream.graphed(S, chunk // hop, sample=False)
            slots = list(range(S))
            mel_s, z_s = rand(S, chunk // hop, cfg.n_mels), rand(S, chunk, 1)
            over = IAFVocoder(batch_size=S, length=chunk + halo, store=store, precision=args.precision)
            mel_o, z_o = rand(S, (chunk + halo) // hop + 1, cfg.n_mels), rand(S, chunk + halo, 1)

            def pipelined():
                for _ in range(8):
                    graphed.tick(mel_s, slots, z=z_s)

            legs = {
                'stream': (lambda: stream.push(mel_s, z=z_s, verify=False), stream.verify, 1),
                'graph': (lambda: graphed.tick(mel_s, slots, z=z_s), graphed.verify, 1),
                'graph_pipelined': (pipelined, graphed.verify, 8),
                'overlap': (lambda: over(None, mel_o, z=z_o, verify=False)[:, halo:], lambda: engine.verify_enqueued('overlap'), 1),
            }
            cell = {'sessions': S, 'chunk': chunk, 'stream_rows': S * chunk, 'overlap_rows': S * (chunk + halo)}
            for name in legs:
                cell[name] = {'ms': [], 'enqueue_ms': []}
            for _ in range(2):
                for name, (fn, sync, ticks) in legs.items():
                    ms, host = timed(fn, sync)
                    cell[name]['ms'].append(round(ms / ticks, 4))
                    cell[name]['enqueue_ms'].append(round(host / ticks, 4))
            assert graphed.captures == 1 and graphed.eager_calls == 0
            assert stream.emitted(0) == warm + 2 * 10 * (args.warmup + args.steps) * chunk
            cell['spread'] = round(max(abs(cell[name]['ms'][0] - cell[name]['ms'][1]) for name in legs), 4)
            ratio = lambda a, b: [round(x / y, 3) for x, y in zip(cell[a]['ms'], cell[b]['ms'])]      # noqa: E731
            cell['graph_over_stream'] = ratio('graph', 'stream')
            cell['graph_pipelined_over_stream'] = ratio('graph_pipelined', 'stream')
            cell['overlap_over_graph'] = ratio('overlap', 'graph')
            cell['graph_not_slower_than_stream'] = all(g <= e + cell['spread'] for g, e in zip(cell['graph']['ms'], cell['stream']['ms']))
            out['cells'].append(cell)
            print('# %s' % json.dumps(cell), file=sys.stderr)
        print(json.dumps(out))
        return

    out = {'case': args.case, 'precision': args.precision, 'steps': args.steps, 'warmup': args.warmup, 'chain_halo': halo, 'cells': []}
    for S in [int(v) for v in args.sessions.split(',')]:
        for chunk in [int(v) for v in args.chunks.split(',')]:
            model = IAFVocoder(batch_size=S, length=chunk, store=store, precision=args.precision)
            stream = open_stream(model, S)
            warm = -(-(halo + hop) // hop) * hop
            stream.push(rand(S, warm // hop + 1, cfg.n_mels), z=rand(S, warm, 1))        # steady state: emitted > chain_halo
            mel_s, z_s = rand(S, chunk // hop, cfg.n_mels), rand(S, chunk, 1)
            over = IAFVocoder(batch_size=S, length=chunk + halo, store=store, precision=args.precision)
            mel_o, z_o = rand(S, (chunk + halo) // hop + 1, cfg.n_mels), rand(S, chunk + halo, 1)
            mel_r, z_r = rand(S, chunk // hop + 1, cfg.n_mels), rand(S, chunk, 1)
            def push_layers():
                engine.PERSIST = False
                try:
                    return stream.push(mel_s, z=z_s, verify=False)
                finally:
                    engine.PERSIST = persist_default

            legs = {
                'stream': (lambda: stream.push(mel_s, z=z_s, verify=False), stream.verify),
                'stream_layers': (push_layers, stream.verify),
                'overlap': (lambda: over(None, mel_o, z=z_o, verify=False)[:, halo:], lambda: engine.verify_enqueued('overlap')),
                'rows': (lambda: model(None, mel_r, z=z_r, verify=False), lambda: engine.verify_enqueued('rows')),
            }
            if per_sample or skip:          # (one streaming route only: PERSIST plays no part)
                del legs['stream_layers']
            stream_legs = [name for name in ('stream', 'stream_layers') if name in legs]
            cell = {'sessions': S, 'chunk': chunk, 'stream_rows': S * chunk, 'overlap_rows': S * (chunk + halo), 'launches': {}}
            for name in stream_legs:        # one untimed push per streaming leg: what it enqueues
                log, calls = [], []
                engine.EVENT_LOG, _lib.lib = log, (lambda: counting(calls))
                try:
                    legs[name][0]()
                    legs[name][1]()
                finally:
                    engine.EVENT_LOG, _lib.lib = None, real_lib
                cell['launches'][name] = {'calls': len([c for c in calls if c not in NOT_LAUNCHES]),
                                          'flows': [e[0] + ('_stream' if len(e) > 8 and e[8] else '') for e in log],
                                          'short_input': [e[7] for e in log if e[0] == 'persist']}
            for name in legs:
                cell[name] = {'ms': [], 'enqueue_ms': []}
            for _ in range(2):
                for name, (fn, sync) in legs.items():
                    ms, host = timed(fn, sync)
                    cell[name]['ms'].append(round(ms, 3))
                    cell[name]['enqueue_ms'].append(round(host, 3))
            assert stream.emitted(0) == warm + len(stream_legs) * (2 * (args.warmup + args.steps) + 1) * chunk
            cell['overlap_over_stream'] = [round(o / s, 3) for o, s in zip(cell['overlap']['ms'], cell['stream']['ms'])]
            if 'stream_layers' in legs:
                cell['stream_over_stream_layers'] = [round(a / b, 3) for a, b in zip(cell['stream']['ms'], cell['stream_layers']['ms'])]
            cell['stream_over_rows'] = [round(a / b, 3) for a, b in zip(cell['stream']['ms'], cell['rows']['ms'])]
            out['cells'].append(cell)
            print('# %s' % json.dumps(cell), file=sys.stderr)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
