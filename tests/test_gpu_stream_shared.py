"""GPU: streaming the shared-net architecture (model.shared_nets: True -- ONE WaveNet of two outputs per flow, out = x y[..., 0] + y[..., 1])
on every streaming route: the persistent streaming launch with G = 1 and the affine inside its two-output tail, the per-layer streaming
launches with a head of two outputs and the strided affine behind them, the packed ragged launch and its grouped fallback, the three graph
wrappers and the CLI.  The contract is the default model's (tests/test_gpu_stream*.py): the pushes of a session concatenate `torch.equal` to
IAFVocoder(1, L)(None, mel, z=z), a session does not depend on its companions, a push is a transaction.  Every case that claims a route
shows from engine.EVENT_LOG that it ran, with one net."""
import numpy as np
import pytest
import torch

from oracle import iaf_oracle as O
from tests.guarded import Guard
from tests.test_gpu_stream import _Feeder, _inputs, _model, _one_shot
from tests.test_gpu_stream_persist import _Log, _random_state, _short_expected, knobs      # noqa: F401  (knobs: the fixture)
from tests.test_gpu_stream_ragged_graph import hop_80_afterwards      # noqa: F401  (the fixture)
from tests.util import TOL_F32, hop_cfg, small_cfg

pytestmark = pytest.mark.gpu
HOP = 80


def _small():
    return small_cfg(shared_nets=True, dilations=[[1, 2, 4, 8], [1, 2, 4, 8, 16, 32]])


def _wide():
    # most dilations above the 80-sample chunk (the carry launch does most of the work), two that are no multiple of 32
    return small_cfg(shared_nets=True, dilations=[[1, 96, 128, 256], [2, 64, 200, 512, 3, 160]])


def _c2():
    return O.ModelConfig(shared_nets=True)          # the architecture of bench/c2


_CFG = {'small': _small, 'wide': _wide, 'c2': _c2}


def _check_persist(log, cfg, pushes, gpu, min_units=0):
    """Every push (rows N * T each) was ONE streaming persistent launch per flow with one net: layer 0 folded, the tail inside, in the
    instantiation the plan predicts.  Returns the instantiations ([7]: 1 = short-input)."""
    flows = [list(d) for d in cfg.dilations[:cfg.n_iaf]]
    assert not [e for e in log if e[0] != 'persist'], [e[0] for e in log]
    assert len(log) == len(pushes) * len(flows), (len(log), len(pushes))
    k = 0
    for rows in pushes:
        for dil in flows:
            e = log[k]
            k += 1
            assert e[3] == 1 and e[8] == 1 and e[5] == 1 and e[6] == 1 and e[4] == len(dil) - 1, e
            assert e[7] == _short_expected(rows, max(dil), gpu, G=1, min_units=min_units or 4), (rows, e[7])
    return [e[7] for e in log]


def _check_layers(log, cfg, pushes):
    assert [e[0] for e in log] == ['layer_stream'] * (cfg.n_iaf * len(pushes)), [e[0] for e in log]
    assert all(e[3] == 1 for e in log)          # one net per launch


# the routes of a uniform push: (engine.PERSIST, engine.PERSIST_MIN_UNITS)
_ROUTES = {'persist': ('auto', 0), 'persist_general': ('auto', 16), 'layers': (False, 0)}


def _set_route(engine, route):
    engine.PERSIST, engine.PERSIST_MIN_UNITS = _ROUTES[route]


@pytest.fixture()
def routes(knobs):      # noqa: F811
    saved = knobs.PERSIST_MIN_UNITS
    try:
        yield knobs
    finally:
        knobs.PERSIST_MIN_UNITS = saved


# ---- 1 -------------------------------------------------------------------------------------------------------------------------------------
def test_open_stream_returns_a_stream(gpu):
    """A shared-net model has a streaming form: one row history per layer and flow."""
    from pwv_amd.stream import HistoryLayout, StreamingVocoder
    cfg = _small()
    model, _ = _model(gpu, cfg)
    s = model.open_stream(slots=2)
    assert isinstance(s, StreamingVocoder) and s.n_slots == 2
    assert all(len(per_net) == 1 for per_net in s.layout.row_off)
    assert s.layout.block_floats == HistoryLayout(cfg.dilations, nets_per_flow=1).block_floats
    assert tuple(s._hist.shape) == (4, s.layout.block_floats)


# ---- 2 -------------------------------------------------------------------------------------------------------------------------------------
_SCHEDULES = {'one_frame': [80] * 20, 'mixed': [160, 80, 400, 160, 800]}
_WANT = {}          # (config, precision, L) -> the one-shot forward, computed once and never written to


def _case(gpu, config, precision, L, seed=1):
    cfg = _CFG[config]()
    model, w = _model(gpu, cfg, precision)
    mel, z, mel_t, z_t = _inputs(cfg, L, gpu, seed=seed)
    key = (config, precision, L, seed)
    if key not in _WANT:
        _WANT[key] = _one_shot(model, mel_t, z_t).clone()
    return cfg, model, w, mel_t, z_t, _WANT[key]


def _stream_schedule(s, mel_t, z_t, schedule):
    """One session fed `schedule`; 80-sample schedules start with the one-frame push (stored only).  Returns its samples."""
    if set(schedule) == {HOP}:
        assert tuple(s.push(mel_t[None, :1], slots=[0], z=z_t[None, :0]).shape) == (1, 0, 1) and s.emitted(0) == 0
        outs = [s.push(mel_t[None, k:k + 1], slots=[0], z=z_t[None, HOP * (k - 1):HOP * k])[0] for k in range(1, len(schedule) + 1)]
        return torch.cat(outs)
    fd = _Feeder(s)
    fd.start(0, mel_t, z_t)
    for T in schedule:
        fd.adv([0], T)
    return fd.result(0)


@pytest.mark.parametrize('schedule', sorted(_SCHEDULES))
@pytest.mark.parametrize('config', ['small', 'wide'])
@pytest.mark.parametrize('precision', ['f16x3', 'f32'])
def test_chunks_equal_the_one_shot_forward(gpu, routes, precision, config, schedule):
    """L = 1600 in one-frame pushes and in [160, 80, 400, 160, 800], on the persistent route at both settings of PERSIST_MIN_UNITS (the
    800-row push takes the short-input instantiation at 0 and the general one at 16) and on the per-layer launches: the one-shot bits on
    every route, and the same history blocks, byte for byte, at the end."""
    sched = _SCHEDULES[schedule]
    cfg, model, _, mel_t, z_t, want = _case(gpu, config, precision, 1600)
    assert sum(sched) == 1600
    hists, kinds = {}, {}
    for route in _ROUTES:
        _set_route(routes, route)
        s = model.open_stream(slots=1)
        with _Log(routes) as lg:
            got = _stream_schedule(s, mel_t, z_t, sched)
            if route == 'layers':
                _check_layers(lg.log, cfg, sched)
            else:
                kinds[route] = _check_persist(lg.log, cfg, sched, gpu, _ROUTES[route][1])
        assert s.emitted(0) == 1600
        assert torch.equal(got, want), (route, float((got - want).abs().max()))
        hists[route] = (s._hist.clone(), list(s._gen))
    for route in ('persist_general', 'layers'):
        assert hists[route][1] == hists['persist'][1]
        assert torch.equal(hists[route][0], hists['persist'][0]), (route, int((hists[route][0] != hists['persist'][0]).sum()))
    if schedule == 'mixed':          # both persistent instantiations ran (the last push, 800 rows)
        assert kinds['persist'][-1] == 1 and kinds['persist_general'][-1] == 0, kinds


@pytest.mark.parametrize('precision', ['f16x3', 'f32'])
def test_chunks_equal_the_one_shot_forward_c2(gpu, routes, precision):
    """The architecture of bench/c2 (default dilations, largest 512), L = 8000: chunks above and below the largest dilation, so the carry
    launch runs in some pushes and not in others; persistent route and per-layer launches, same bits and same histories."""
    sched = [80, 2400, 560, 160, 4000, 400, 400]
    cfg, model, _, mel_t, z_t, want = _case(gpu, 'c2', precision, 8000)
    assert sum(sched) == 8000
    hists = {}
    for route in ('persist', 'layers'):
        _set_route(routes, route)
        s = model.open_stream(slots=1)
        with _Log(routes) as lg:
            got = _stream_schedule(s, mel_t, z_t, sched)
            if route == 'layers':
                _check_layers(lg.log, cfg, sched)
            else:
                _check_persist(lg.log, cfg, sched, gpu)
        assert torch.equal(got, want), (route, float((got - want).abs().max()))
        hists[route] = s._hist.clone()
    assert torch.equal(hists['persist'], hists['layers']), int((hists['persist'] != hists['layers']).sum())


# ---- 3 -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', ['f16x3', 'f32'])
def test_stream_matches_oracle(gpu, precision):
    """Two sessions against the fp64 oracle at the fp32 bar of every parity test (enqueue-only + verify(): no self-repair)."""
    cfg = _small()
    L = 800
    model, w = _model(gpu, cfg, precision)
    s = model.open_stream(slots=2)
    fd = _Feeder(s)
    ins = [_inputs(cfg, L, gpu, seed=10 + i) for i in range(2)]
    for i in range(2):
        fd.start(i, ins[i][2], ins[i][3])
    for T in [160, 80, 400, 160]:
        fd.adv([0, 1], T, verify=False)
        s.verify()
    for i in range(2):
        want = O.iaf_vocoder_forward(w, ins[i][0][None], ins[i][1][None], cfg)[0]
        err = float(np.abs(fd.result(i).cpu().numpy() - want).max())
        print('shared stream vs oracle, %s, slot %d: %.3g' % (precision, i, err))
        assert err <= TOL_F32, err


# ---- 4 -------------------------------------------------------------------------------------------------------------------------------------
def test_slots_are_independent(gpu):
    """3 slots on different schedules, slot 2 reset midway and restarted on another utterance: every finished utterance equals its own
    one-shot forward, the abandoned one the prefix of its own."""
    cfg = _small()
    model, _ = _model(gpu, cfg)
    s = model.open_stream(slots=3)
    fd = _Feeder(s)
    a, b, c, d = (_inputs(cfg, L, gpu, seed=20 + i) for i, L in enumerate([960, 960, 960, 480]))
    fd.start(0, a[2], a[3]), fd.start(1, b[2], b[3]), fd.start(2, c[2], c[3])
    fd.adv([0, 1, 2], 160)
    fd.adv([2, 0], 80)
    fd.adv([1], 240)
    fd.adv([0, 1], 160)
    part_c = fd.result(2)
    s.reset(2)
    assert s.emitted(2) == 0
    fd.start(2, d[2], d[3])
    fd.adv([2], 240)
    fd.adv([0, 1, 2], 80)
    fd.adv([2, 1], 160)          # d done (480)
    fd.adv([0], 480)             # a done (960)
    fd.adv([1], 160)             # b done (960)
    assert [s.emitted(i) for i in range(3)] == [960, 960, 480]
    for slot, u in ((0, a), (1, b), (2, d)):
        assert torch.equal(fd.result(slot), _one_shot(model, u[2], u[3])), slot
    assert torch.equal(part_c, _one_shot(model, c[2], c[3])[:240])


# ---- 5 -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('route', ['packed', 'grouped'])
@pytest.mark.parametrize('precision', ['f16x3', 'f32'])
def test_ragged_tick(gpu, routes, precision, route):
    """push_varlen of three sessions with 1, 3 and 7 frames -- sessions 0 and 1 running, session 2 fresh -- then with 7, 3 and 1 (the last
    chunk shorter than the others): the bits and the history blocks of the three separate pushes, on the packed launch and (PERSIST off)
    on the grouped fallback; and every session ends on its own one-shot forward."""
    cfg = _small()
    model, _ = _model(gpu, cfg, precision)
    frames = [3 + 1 + 7, 3 + 3 + 3, 7 + 1]          # frames per session over the three calls below
    ins = [_inputs(cfg, (f - 1) * HOP, gpu, seed=30 + i) for i, f in enumerate(frames)]
    a, b = model.open_stream(slots=3), model.open_stream(slots=3)
    for s in (a, b):
        s.push(torch.stack([ins[0][2][:3], ins[1][2][:3]]), slots=[0, 1], z=torch.stack([ins[0][3][:160], ins[1][3][:160]]))
    fpos, outs = [3, 3, 0], [[], [], []]
    routes.PERSIST = False if route == 'grouped' else 'auto'
    for counts in ([1, 3, 7], [7, 3, 1]):
        mels, zs = [], []
        for i, f in enumerate(counts):
            T = (f - (1 if fpos[i] == 0 else 0)) * HOP
            mels.append(ins[i][2][fpos[i]:fpos[i] + f])
            zs.append(ins[i][3][a.emitted(i):a.emitted(i) + T])
        with _Log(routes) as lg:
            got = a.push_varlen(mels, z=zs)
            kinds = [e[3] for e in lg.log if e[0] == 'stream_ragged']
            assert kinds == [route] * cfg.n_iaf, lg.log
            if route == 'packed':
                per = [e for e in lg.log if e[0] == 'persist']
                assert len(per) == cfg.n_iaf and all(e[3] == 1 and e[8] == 1 and e[5] == 1 and e[6] == 1 for e in per), per
                assert not [e for e in lg.log if e[0] not in ('persist', 'stream_ragged')]
            else:
                assert not [e for e in lg.log if e[0] == 'persist'] and all(e[3] == 1 for e in lg.log if e[0] == 'layer_stream')
        routes.PERSIST = 'auto'
        for i in range(3):          # the same chunks as three separate pushes
            want = b.push(mels[i][None], slots=[i], z=zs[i][None])[0]
            assert torch.equal(got[i], want), (i, float((got[i] - want).abs().max()))
            outs[i].append(got[i])
            fpos[i] += counts[i]
        routes.PERSIST = False if route == 'grouped' else 'auto'
        assert a._gen == b._gen
        cur = [2 * i + a._gen[i] for i in range(3)]
        assert torch.equal(a._hist[cur], b._hist[cur]), int((a._hist[cur] != b._hist[cur]).sum())
        assert torch.equal(a._kept, b._kept)
    routes.PERSIST = 'auto'
    for i in range(3):
        head = [_one_shot(model, ins[i][2], ins[i][3])[:160]] if i < 2 else []
        assert a.emitted(i) == (frames[i] - 1) * HOP
        assert torch.equal(torch.cat(head + outs[i]), _one_shot(model, ins[i][2], ins[i][3])), i


# ---- 6 -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', ['f16x3', 'f32'])
def test_graphed_uniform_tick(gpu, routes, precision):
    """graphed(2, 2): three ticks enqueued back to back equal the eager pushes from the same state bit for bit -- outputs, histories, kept
    frames, counters --, one verify() settles them, and the capture's warm-up ran one streaming persistent launch per flow."""
    cfg = _small()
    model, _ = _model(gpu, cfg, precision)
    f, n = 2, 2
    rng = np.random.default_rng(8)
    mels = [torch.from_numpy(rng.uniform(-1, 1, (n, f, cfg.n_mels)).astype(np.float32)).to(gpu) for _ in range(3)]
    zs = [torch.from_numpy(np.clip(rng.logistic(0, 1, (n, f * HOP, 1)), -20, 20).astype(np.float32)).to(gpu) for _ in range(3)]
    res = []
    for graphed in (True, False):
        s = model.open_stream(slots=n)
        g = None
        if graphed:
            with _Log(routes) as lg:
                g = s.graphed(n, f, sample=False)
            _check_persist(lg.log, cfg, [n * f * HOP] * 2, gpu)
            assert g.captures == 1 and g.eager_calls == 0
        for sl in range(n):          # mid-utterance, as load_state leaves a session
            st = s.state(sl)
            st['kept'] = torch.from_numpy(np.random.default_rng(5 + sl).uniform(-1, 1, (s.n_mels,)).astype(np.float32)).to(gpu)
            st['running'], st['emitted'] = True, HOP * (3 + sl)
            s.load_state(sl, st)
        _random_state(s, 104)
        if graphed:
            outs = [g.tick(mels[j], [0, 1], z=zs[j]).clone() for j in range(3)]
            assert s._pending is not None and s.emitted(0) == 3 * HOP          # nothing has come back to the host yet
            assert g.verify() == 3 and s._pending is None and g.eager_calls == 0 and g.captures == 1
        else:
            outs = [s.push(mels[j], z=zs[j]) for j in range(3)]
        res.append((torch.cat(outs, dim=1), s._hist.clone(), s._kept.clone(), [s.emitted(sl) for sl in range(n)], list(s._gen)))
    (out_g, hist_g, kept_g, em_g, gen_g), (out_p, hist_p, kept_p, em_p, gen_p) = res
    assert bool(torch.isfinite(out_g).all()) and torch.equal(out_g, out_p), float((out_g - out_p).abs().max())
    assert torch.equal(hist_g, hist_p), int((hist_g != hist_p).sum())
    assert torch.equal(kept_g, kept_p) and em_g == em_p == [HOP * (3 + sl) + 3 * f * HOP for sl in range(n)] and gen_g == gen_p


@pytest.mark.parametrize('sample', [False, True], ids=['own_noise', 'sampler'])
def test_graphed_ragged_tick_with_a_start_on_a_running_slot(gpu, routes, sample):
    """graphed_varlen(3, 1600) on a 3-slot stream (slot 2 serves the filler entries): a plain tick of two running sessions; a tick in which
    slot 1, running, is cut off and STARTS another utterance (starts=); a plain tick in the other order.  Enqueued back to back, every
    piece equals the piece of a second stream driven by reset + push_varlen, one verify() settles them with nothing run eagerly, and the
    sessions end on their own one-shot forwards."""
    from tests.test_gpu_stream_starts import _Utterance, _drive
    cfg = _small()
    model, _ = _model(gpu, cfg)
    u = [_Utterance(cfg, f, gpu, 60 + i) for i, f in enumerate((9, 8, 7))]
    seeds = [3, 4, (1 << 63) + 5]
    s, ref = model.open_stream(slots=3), model.open_stream(slots=3)
    for st in (s, ref):
        st.push_varlen([u[0].mel[:1], u[1].mel[:1]], slots=[0, 1], **({'seeds': seeds[:2]} if sample else {'z': [u[0].z[:0], u[1].z[:0]]}))
    with _Log(routes) as lg:
        g = s.graphed_varlen(3, 1600, sample=sample)
    assert [e[3] for e in lg.log if e[0] == 'stream_ragged'] == ['packed'] * (2 * cfg.n_iaf), lg.log
    per = [e for e in lg.log if e[0] == 'persist']
    assert len(per) == 2 * cfg.n_iaf and all(e[3] == 1 and e[8] == 1 and e[5] == 1 and e[6] == 1 for e in per), per
    assert g.captures == 1 and g.eager_calls == 0
    ticks = [[(0, u[0], 3, None), (1, u[1], 2, None)],
             [(0, u[0], 2, None), (1, u[2], 4, ('start', seeds[2], True))],
             [(1, u[2], 3, None), (0, u[0], 4, None)]]
    pieces = {0: [], 2: []}
    owner = [{0: 0, 1: 1}, {0: 0, 1: 2}, {1: 2, 0: 0}]
    for tick, who in zip(ticks, owner):
        assert g.fits([t[2] for t in tick])
        got, want = _drive(g, ref, tick, sample)
        for t, a, b in zip(tick, got, want):
            assert a.shape == b.shape == (t[2] * HOP, 1) and torch.equal(a, b), (t[0], float((a - b).abs().max()))
            if who[t[0]] in pieces:
                pieces[who[t[0]]].append(a)
    assert g.verify() == 3 and g.eager_calls == 0 and g.captures == 1
    assert [s.emitted(i) for i in range(3)] == [ref.emitted(i) for i in range(3)] == [9 * HOP, 7 * HOP, 0]
    for sl in range(3):
        a, b = s.state(sl), ref.state(sl)
        assert torch.equal(a['hist'], b['hist']) and torch.equal(a['kept'], b['kept']) and a['running'] == b['running'], sl
    for i in (0, 2):
        want = _one_shot(model, u[i].mel, None if sample else u[i].z, seed=seeds[i] if sample else None)
        assert torch.equal(torch.cat(pieces[i]), want), i


def test_graphed_live_tick_at_hop_16(gpu, routes, hop_80_afterwards):      # noqa: F811
    """graphed_live at n_fft 64 / win_length 40 / hop 16 (min_frames 2), sized as tests/test_gpu_live_tick.py sizes it: chunks of 96 samples,
    all ticks graphed; the pieces equal the one-shot pair and the eager fe.push / fe.finish / push_varlen sequence bit for bit."""
    from pwv_amd.audio_frontend import StreamingMel
    from tests.test_gpu_live_tick import HOP16, _eager_sequence, _Feed, _want, _wavs
    cfg = hop_cfg(16, shared_nets=True)
    model, _ = _model(gpu, cfg)
    lengths, seeds = (400, 290), (21, 22)
    wavs = _wavs(gpu, lengths, first=1)
    fe, s = StreamingMel(3, signal=HOP16), model.open_stream(slots=3)
    live = s.graphed_live(fe, 2, 320)
    assert live.min_frames == 2 and live.wav_cap == 320 + 2 * (32 + 16)
    feed = _Feed(HOP16, wavs, [96, 96], seeds)
    log, n = [], 0
    while feed.left():
        before = feed.state()
        log.append(feed.args())
        feed.rewind(before)
        feed.tick(live)
        n += 1
    assert live.verify() == n and live.eager_calls == 0 and live.captures == 1
    eager = _eager_sequence(model, HOP16, log, 3, True)
    for i, L in enumerate(lengths):
        want = _want(model, HOP16, wavs[i], seeds[i])
        assert feed.result(i).shape == (L // 16 * 16, 1) and torch.equal(feed.result(i), want), i
        assert torch.equal(feed.result(i), eager[i]), i


# ---- 7 -------------------------------------------------------------------------------------------------------------------------------------
def test_pack_time_demotion_is_the_same_on_every_route(gpu, routes):
    """The last-layer `skip` of flow 1's shared net scaled by 2e4 fails the pack-time bound of the split-fp16 arithmetic (as
    tests/test_gpu_stream_varlen.py does it for the default model): that flow -- and only it -- runs in exact fp32 on the one-shot forward,
    on uniform pushes (persistent and per layer) and on a ragged schedule; same bits everywhere, one warning for the net."""
    import warnings
    from pwv_amd import _lib
    from pwv_amd.variables import variable_scope
    from tests.test_gpu_stream_varlen import _run_schedule
    engine = routes
    cfg = _small()
    model, w = _model(gpu, cfg, 'f16x3')
    name = 'iaf_vocoder/iaf1/shared/dilated_stack/layer%d/skip' % (len(cfg.dilations[1]) - 1)
    model.store.assign(name, w[name] * 2.0e4)
    with variable_scope('iaf_vocoder'):
        flows = model._flows(model.store, False, 'f16x3')
    ok = [[engine.get_plan(net, 'frames', _lib.PREC_F16X3).f16x3_ok for net in iaf.nets()] for iaf in flows]
    assert ok == [[True], [False]], ok
    key = tuple(net.full_scope for net in flows[1].nets())
    engine._range_warned.discard(key)
    layers = [len(d) - 1 for d in cfg.dilations[:cfg.n_iaf]]
    seen = []
    schedule = {0: [4, 1, 5], 1: [None, 9, 7], 2: [None, None, 6]}
    engine.PERSIST_ARGS_HOOK = lambda pa: seen.append((int(pa.G), int(pa.n_layers), int(pa.precision)))
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter('always')
            s, fd, ins, rows = _run_schedule(model, cfg, gpu, schedule, 80)
            ragged, seen[:] = list(seen), []
            want = [_one_shot(model, ins[sl][2], ins[sl][3]) for sl in schedule]
            one_shot, seen[:] = list(seen), []
            res = {}
            for route in ('persist', 'layers'):
                _set_route(engine, route)
                u = model.open_stream(slots=3)
                uf = _Feeder(u)
                for sl, chunks in ((0, [240, 80, 400]), (1, [640, 560]), (2, [400])):
                    uf.start(sl, ins[sl][2], ins[sl][3])
                    for T in chunks:
                        uf.adv([sl], T)
                res[route] = [uf.result(sl) for sl in schedule]
                if route == 'persist':
                    uniform, seen[:] = list(seen), []
            assert not seen          # the per-layer route makes no persistent launch
    finally:
        engine.PERSIST_ARGS_HOOK = None
    assert rows == [240, 80 + 640, 400 + 560 + 400]
    for sl in schedule:
        for route, got in (('push', res['persist'][sl]), ('push per layer', res['layers'][sl]), ('push_varlen', fd.result(sl))):
            assert torch.equal(got, want[sl]), (route, sl, float((got - want[sl]).abs().max()))
    for route, launches in (('one-shot', one_shot), ('push', uniform), ('push_varlen', ragged)):
        assert launches and all(g == 1 for g, _, _ in launches), (route, launches)
        demoted = [p for _, n, p in launches if n == layers[1]]
        assert demoted and all(p == _lib.PREC_F32 for p in demoted), (route, launches)
        assert [p for _, n, p in launches if n == layers[0]] == [_lib.PREC_F16X3] * len(demoted), (route, launches)
    told = [str(c.message) for c in caught if 'exceed the range' in str(c.message)]
    assert len(told) == 1 and key[0] in told[0], told


def test_a_push_refused_at_verify_leaves_the_session_where_it_was(gpu):
    """A chunk whose mel leaves the range of the split-fp16 arithmetic, only enqueued: verify() raises PwvRangeError and commits nothing
    -- generation, counter, kept frame and the block the session stands on are as before.  The same chunk pushed as a verified call is rerun
    in exact fp32 from that generation (it warns) and equals the push of a precision='f32' stream brought to the same state; the stream
    goes on from there."""
    from pwv_amd._lib import PwvRangeError
    from pwv_amd.models import IAFVocoder
    cfg = _small()
    model, _ = _model(gpu, cfg)
    m32 = IAFVocoder(batch_size=1, length=80, store=model.store, precision='f32')
    L = 720
    _, _, mel_t, z_t = _inputs(cfg, L, gpu, seed=40)
    mel_t = mel_t.clone()
    mel_t[4:6] *= 1e5                      # frames 4, 5 of the chunk that brings frames 4, 5, 6
    s = model.open_stream(slots=1)
    first = s.push(mel_t[None, :4], z=z_t[None, :240])
    assert torch.equal(first[0], _one_shot(model, mel_t[:4], z_t[:240]))
    before = s.state(0)
    gen = list(s._gen)
    s.push(mel_t[None, 4:7], z=z_t[None, 240:480], verify=False)
    with pytest.raises(PwvRangeError):
        s.verify()
    after = s.state(0)
    assert s._gen == gen and s._pending is None and s.emitted(0) == 240 and after['running']
    assert torch.equal(after['hist'], before['hist']) and torch.equal(after['kept'], before['kept'])
    with pytest.warns(UserWarning, match='rerun in exact fp32'):
        tripped = s.push(mel_t[None, 4:7], z=z_t[None, 240:480])
    assert s.emitted(0) == 480 and bool(torch.isfinite(tripped).all())
    s32 = m32.open_stream(slots=1)
    s32.load_state(0, before)
    assert torch.equal(tripped, s32.push(mel_t[None, 4:7], z=z_t[None, 240:480]))
    s2 = model.open_stream(slots=1)
    s2.load_state(0, s32.state(0))
    last = s.push(mel_t[None, 7:], z=z_t[None, 480:])
    assert torch.equal(last, s2.push(mel_t[None, 7:], z=z_t[None, 480:])) and s.emitted(0) == L


# ---- 8 -------------------------------------------------------------------------------------------------------------------------------------
def test_state_moves_a_session_to_another_slot(gpu):
    """state -> load_state into another slot continues to the same bits; state_bytes follows the layout; a state of the default
    architecture (another block size) is turned away."""
    cfg, model, _, mel_t, z_t, want = _case(gpu, 'small', None, 1600)
    s = model.open_stream(slots=3)
    a = s.push(mel_t[None, :9], slots=[0], z=z_t[None, :640])
    s.load_state(2, s.state(0))
    assert s.emitted(2) == 640
    b = s.push(mel_t[None, 9:], slots=[2], z=z_t[None, 640:])
    assert torch.equal(torch.cat([a[0], b[0]]), want)
    assert s.state_bytes(0) == 2 * s.layout.block_floats * 4 + cfg.n_mels * 4
    two = small_cfg(dilations=[list(d) for d in cfg.dilations])
    other, _ = _model(gpu, two)
    st_two = other.open_stream(slots=1).state(0)
    assert st_two['block_floats'] > s.layout.block_floats
    with pytest.raises(ValueError, match='another shape'):
        s.load_state(1, st_two)


def test_state_bytes_of_the_c2_model(gpu):
    model, _ = _model(gpu, _c2())
    s = model.open_stream(slots=1)
    assert s.state_bytes(0) == 2 * s.layout.block_floats * 4 + 80 * 4 == 3475776


# ---- 9 -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('schedule', sorted(_SCHEDULES))
@pytest.mark.parametrize('precision', ['f16x3', 'f32'])
def test_guard_bands_around_the_histories(gpu, routes, precision, schedule):
    """The small model's two schedules on the persistent route once more, the history blocks (hist_alloc) inside a 0xFF-filled buffer
    (tests/guarded.py): the one-shot bits, no NaN left in a block, no band touched, and the blocks of a slot that was never pushed still
    zero."""
    sched = _SCHEDULES[schedule]
    cfg, model, _, mel_t, z_t, want = _case(gpu, 'small', precision, 1600)
    _set_route(routes, 'persist')
    bands = Guard(band_bytes=1 << 18)
    s = model.open_stream(slots=2, hist_alloc=lambda floats: bands.allocate((floats,), torch.float32, gpu, 0.0))
    with _Log(routes) as lg:
        got = _stream_schedule(s, mel_t, z_t, sched)
        _check_persist(lg.log, cfg, sched, gpu)
    torch.cuda.synchronize()
    bands.check()
    blocks = bands.allocations[0].payload().view(4, -1)
    assert not bool(torch.isnan(blocks).any()) and not bool(blocks[2:4].any())
    assert torch.equal(got, want), float((got - want).abs().max())


# ---- 10 ------------------------------------------------------------------------------------------------------------------------------------
def test_generate_cli_stream(gpu, tmp_path, monkeypatch):
    """`generate default --stream=5` on a case with shared_nets: True and three .npy mels of 3, 21 and 9 frames writes the sample counts
    `--varlen` writes, and `--stream=5 --graph` writes the same samples (the OS seeds the CLI draws are made the same for the runs)."""
    from pwv_amd import engine
    from pwv_amd.generate import _fire, generate
    from pwv_amd.hparam import hparam as hp
    rng = np.random.default_rng(4)
    frames = [3, 21, 9]
    for i, f in enumerate(frames):
        np.save(str(tmp_path / ('m%d.npy' % i)), rng.uniform(-1, 1, (f, 80)).astype(np.float32))
    orig = type(hp).set_hparam_yaml

    def patched(self, case, *a, **k):          # what a user's hparams.yaml case would override
        r = orig(self, case, *a, **k)
        self.data_path = str(tmp_path / '*.npy')
        self.train.dataset_ratio, self.generate.batch_size = 0.0, 3
        self.model.n_iaf, self.model.dilations, self.model.shared_nets = 1, [[1, 2, 4, 8]], True
        return r

    monkeypatch.setattr(type(hp), 'set_hparam_yaml', patched)
    files, shapes = {}, {}
    for how, argv in (('varlen', ['default', '--varlen']), ('stream', ['default', '--stream=5']), ('graph', ['default', '--stream=5', '--graph'])):
        drawn = iter(range(1000, 2000))
        monkeypatch.setattr(engine, 'os_seed', lambda: next(drawn))
        logdir = tmp_path / how
        monkeypatch.setenv('PWV_LOGDIR', str(logdir))
        pred = _fire(generate, argv)
        shapes[how] = [p.shape for p in pred]
        files[how] = [(logdir / ('pred_%d.wav' % i)).read_bytes() for i in range(3)]
        with np.load(str(logdir / 'pred_wav_varlen.npz')) as npz:
            files[how] += [npz['pred_%d' % i].tobytes() for i in range(3)]
    assert shapes['varlen'] == shapes['stream'] == shapes['graph'] == [((f - 1) * 80, 1) for f in frames]
    assert files['graph'] == files['stream']
