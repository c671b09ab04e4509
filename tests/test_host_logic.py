"""CPU: hparam semantics (hparam.py:7-68), the variable store / TF naming, the fire-style CLI
parser, and that the product path refuses CPU tensors instead of falling back."""
import os

import numpy as np
import pytest
import torch

from oracle import iaf_oracle as O


def test_hparam_cases_and_merge():
    from pwv_amd.hparam import hparam as hp, merge_dict
    hp.set_hparam_yaml('default')                      # unknown case name -> plain defaults (hparam.py:59)
    assert hp.case == 'default' and hp.logdir == hp.logdir_path + '/default'
    assert hp.signal.hop_length == 80 and hp.model.n_iaf == 4 and hp['model']['filter_width'] == 2
    assert [len(d) for d in hp.model.dilations] == [10, 10, 10, 30]
    assert hp.model.use_skip_connection is False and hp.model.cond_upsample_method == 'repeat'
    assert hp.generate.length == 64000 and hp.generate.batch_size == 3
    hp.set_hparam_yaml('test/tran')                    # user wins, defaults fill recursively
    assert hp.model.cond_upsample_method == 'transposed_conv' and hp.model.n_iaf == 4
    assert hp.train.batch_size == 1 and hp.train.lr == 0.0002
    assert hp.data_path.endswith('slt/*.wav')          # case-level data_path under train:/generate: is inert
    hp.set_hparam_yaml('bench/c1')                     # lists are replaced whole, not merged (hparam.py:17-24)
    assert hp.model.dilations == [[1, 2, 4, 8, 16, 32, 64, 128]] and hp.model.n_iaf == 1
    assert hp.data_path == 'synthetic'
    hp.set_hparam_yaml('ema/len4000')                  # second YAML document
    assert hp.train.num_gpu == 8 and hp.train.batch_size == 8
    assert merge_dict({'a': {'x': 1}, 'l': [1]}, {'a': {'x': 2, 'y': 3}, 'l': [1, 2], 'b': 4}) == \
        {'a': {'x': 1, 'y': 3}, 'l': [1], 'b': 4}
    cfg = O.ModelConfig.from_hparam(hp.set_hparam_yaml('bench/c2'))
    assert cfg.shared_nets and cfg.n_iaf == 4
    hp.set_hparam_yaml('default')


def test_variable_names_match_tf_graph():
    """WaveNet creates exactly the TF variable names / shapes of SURVEY.md section 8 f-1."""
    from pwv_amd.modules import WaveNet
    from pwv_amd.variables import VariableStore, variable_scope
    store = VariableStore(device='cpu')
    cfg = O.ModelConfig(dilations=[[1, 2, 4]], n_iaf=1)
    with variable_scope('iaf_vocoder'), variable_scope('iaf0'):
        nets = [WaveNet(1, [1, 2, 4], 2, 64, 64, 128, quantization_channels=1, use_biases=True,
                        condition_channels=80, use_skip_connection=False, name=n, store=store)
                for n in ('scalar', 'shifter')]
    for net in nets:
        net.causal_filter()
        for j in range(3):
            net.layer_variables(j, with_cond=True)
        net.head_variables()
    want = {k: v for k, v in O.variable_shapes(cfg).items() if '/iaf0/' in k}
    got = {k: tuple(v.shape) for k, v in store.vars.items()}
    assert got == want
    # biases follow the reference's zeros_initializer, matrices are glorot-uniform bounded
    assert float(store.vars['iaf_vocoder/iaf0/scalar/dilated_stack/layer0/filter_bias'].abs().max()) == 0.0
    w = store.vars['iaf_vocoder/iaf0/scalar/dilated_stack/layer0/filter']
    assert float(w.abs().max()) <= np.sqrt(6.0 / (2 * 64 + 2 * 64)) + 1e-7 and float(w.std()) > 0.05


def test_store_ema_preference_and_shape_checks():
    from pwv_amd.variables import EMA_SUFFIX, VariableStore
    store = VariableStore(device='cpu')
    ck = {'a/w': np.ones((2, 3), np.float32), 'a/w' + EMA_SUFFIX: np.full((2, 3), 5, np.float32),
          'a/b': np.zeros(3, np.float32)}
    assert store.load_dict(ck, use_ema=True) == 2          # generate.py:59-63: EMA shadow wins
    assert float(store.vars['a/w'][0, 0]) == 5.0
    store.load_dict(ck, use_ema=False)
    assert float(store.vars['a/w'][0, 0]) == 1.0
    v0 = store.version
    assert store.get_variable('a/w', [2, 3]) is store.vars['a/w'] and store.version == v0
    with pytest.raises(ValueError):
        store.get_variable('a/w', [3, 2])
    with pytest.raises(ValueError):
        store.assign('a/w', np.zeros((4, 4)))


def test_fire_style_cli():
    from pwv_amd.generate import _fire
    got = {}
    def fn(case='default', ckpt=None, debug=False):
        got.update(case=case, ckpt=ckpt, debug=debug)
    _fire(fn, ['bench/c1'])
    assert got == dict(case='bench/c1', ckpt=None, debug=False)
    _fire(fn, ['test/tran', '--ckpt=model-100', '--debug'])
    assert got == dict(case='test/tran', ckpt='model-100', debug=True)
    _fire(fn, ['--case', 'ema/lj', '--ckpt', 'x'])
    assert got == dict(case='ema/lj', ckpt='x', debug=False)


def test_cpu_tensors_are_refused(built_lib):
    """The product path has no CPU implementation: it raises instead of silently computing elsewhere."""
    from pwv_amd import _lib
    from pwv_amd.modules import causal_conv
    with pytest.raises(_lib.PwvError, match='no CPU path'):
        causal_conv(torch.zeros(1, 8, 4), torch.zeros(2, 4, 4), 1)


def test_repeated_condition_validation():
    from pwv_amd.engine import RepeatedCondition
    frames = torch.zeros(2, 5, 80)
    rc = RepeatedCondition(frames, 80, 40, 320)
    assert rc.shape == (2, 320, 80)
    with pytest.raises(ValueError):
        RepeatedCondition(frames, 80, 40, 400)          # needs 6 frames


@pytest.mark.parametrize('knob', ['PERSIST', '_persist_cooldown', 'TWO_STREAMS', 'FOLD_FIRST', 'FUSE_FIRST', 'FUSE_HEAD', 'FUSE_TAIL',
                                  'HOIST_P', 'PERSIST_MAX_LAYERS', 'PERSIST_MIN_UNITS', 'DEFAULT_PRECISION', 'FUSE_PROLOGUE',
                                  'FUSE_PROLOGUE_MAX_OUTPUTS', 'PERSIST_AUTO_MAX_ROWS'])
def test_every_launch_knob_outdates_a_captured_graph(monkeypatch, knob):
    """A graph captured under one value of a knob that decides which launches a forward enqueues is stale under another
    (_persist_cooldown: a suspension of the persistent launches) -- for each of the three wrappers, through the one _stale() they
    share; new weights and a dropped graph make it stale too."""
    from pwv_amd import engine
    saved = getattr(engine, knob)
    other = {'PERSIST': False if saved is not False else 'auto', 'DEFAULT_PRECISION': 'f32' if saved != 'f32' else 'f16x3'}.get(knob)
    if other is None:
        other = (not saved) if isinstance(saved, bool) else saved + 1
    for cls in _graph_classes():
        g = _captured_stand_in(cls)
        assert not g._stale(), cls.__name__
        monkeypatch.setattr(engine, knob, other)
        assert g._stale(), cls.__name__
        monkeypatch.setattr(engine, knob, saved)
        assert not g._stale(), cls.__name__
        g.store.version += 1
        assert g._stale(), cls.__name__
        g.store.version -= 1
        assert not g._stale(), cls.__name__
        g.graph = None
        assert g._stale(), cls.__name__


def _graph_classes():
    from pwv_amd.graph import GraphedPackedVocoder, GraphedStream, GraphedVocoder
    return GraphedVocoder, GraphedPackedVocoder, GraphedStream


def _captured_stand_in(cls):
    """A wrapper as it stands after a capture made now, without a device: a store with a version, a sentinel for the graph."""
    import types
    from pwv_amd import engine
    g = cls.__new__(cls)
    g.store = types.SimpleNamespace(version=3)
    g.graph, g._version, g._mode = object(), g.store.version, engine.launch_knobs()
    return g


def test_ready_policy_under_a_suspension():
    """_ready(): under a suspension the two wrappers whose forward exists on the persistent route only drop their graph, answer False
    and capture nothing, GraphedVocoder captures once (the knobs changed: the per-layer path); after the suspension every one of them
    captures once more; _settle runs ahead of every capture and at no other time."""
    from pwv_amd import engine
    for cls in _graph_classes():
        g, events = _captured_stand_in(cls), []

        def capture(g=g, events=events):
            events.append('capture')
            g.graph, g._version, g._mode = object(), g.store.version, engine.launch_knobs()
        g._capture, g._settle = capture, lambda events=events: events.append('settle')
        assert g._ready() is True and events == [], cls.__name__
        engine.suspend_persist()
        try:
            for _ in range(2):
                if cls.PERSIST_ONLY:
                    assert g._ready() is False and g.graph is None and events == [], cls.__name__
                else:
                    assert g._ready() is True and g.graph is not None and events == ['settle', 'capture'], cls.__name__
        finally:
            engine.resume_persist()
        del events[:]
        for _ in range(2):
            assert g._ready() is True and g.graph is not None and events == ['settle', 'capture'], cls.__name__
    assert [cls.PERSIST_ONLY for cls in _graph_classes()] == [False, True, True]


def test_u64_helpers():
    from pwv_amd import engine
    for bad in (True, -1, 2 ** 64, 1.0):
        with pytest.raises(ValueError, match=r'a seed must be an integer in \[0, 2\*\*64\), got'):
            engine.check_u64(bad, 'a seed')
    for good in (0, 2 ** 64 - 1, np.int64(5)):
        got = engine.check_u64(good, 'a seed')
        assert type(got) is int and got == int(good)
    v = (1 << 63) + 12345
    assert engine.as_int64_bits(v) == v - (1 << 64) and engine.from_int64_bits(engine.as_int64_bits(v)) == v
    assert all(engine.from_int64_bits(engine.as_int64_bits(u)) == u for u in (0, 7, (1 << 63) - 1, 1 << 63, (1 << 64) - 1))
    assert 0 <= engine.os_seed() < 1 << 56


def test_fused_supported_matrix():
    from pwv_amd.engine import RepeatedCondition
    from pwv_amd.modules import WaveNet
    from pwv_amd.variables import VariableStore
    st = VariableStore(device='cpu')
    mk = lambda **kw: WaveNet(1, [1, 2], kw.pop('W', 2), kw.pop('R', 64), 64, 128, quantization_channels=1,
                              condition_channels=kw.pop('C', 80), store=st, **kw)
    rc = RepeatedCondition(torch.zeros(1, 3, 80), 80, 40, 160)
    assert mk().fused_supported(None) and mk().fused_supported(rc) and mk().fused_supported(torch.zeros(1, 160, 80))
    assert not mk(W=3).fused_supported(None) and not mk(R=32).fused_supported(None)
    assert not mk(normalize='in').fused_supported(None)
    assert not mk(C=40).fused_supported(torch.zeros(1, 160, 40))     # per-sample conditioning kernel is 80-channel
    assert mk(C=40).fused_supported(RepeatedCondition(torch.zeros(1, 3, 40), 80, 40, 160))


def test_time_shard_plan():
    from pwv_amd.timeshard import chain_halo, shard_plan
    d10 = [1, 2, 4, 8, 16, 32, 64, 128, 256, 512]
    assert chain_halo([d10, d10, d10, d10 * 3], 2, 4, 1) == 6142
    assert chain_halo([d10, d10, d10, d10 * 3], 2, 4, 80) == 6160
    plan = shard_plan(960000, 8, 6160, 80)
    assert plan[0] == (0, 0, 120000) and plan[-1][2] == 960000
    assert all(a % 80 == 0 and b % 80 == 0 and c % 80 == 0 for c, a, b in plan)
    assert all(plan[i][2] == plan[i + 1][1] for i in range(7))             # outputs tile [0, L)
    assert all(a - c == min(a, 6160) for c, a, b in plan)
    assert len(shard_plan(160, 8, 6160, 80)) == 2                            # never more shards than frames
    with pytest.raises(ValueError):
        shard_plan(100, 2, 0, 80)


def test_fire_style_cli_parsing():
    """python-fire accepts `generate c --debug --ckpt foo` (a bare flag followed by a spaced option): ADVICE r1."""
    from pwv_amd.generate import _fire
    seen = {}

    def fn(case='default', ckpt=None, debug=False):
        seen.update(case=case, ckpt=ckpt, debug=debug)

    _fire(fn, ['c', '--debug', '--ckpt', 'foo'])
    assert seen == dict(case='c', ckpt='foo', debug=True)
    _fire(fn, ['--ckpt=model-1', '--debug=False', 'x'])
    assert seen == dict(case='x', ckpt='model-1', debug=False)
    _fire(fn, ['y', '--debug'])
    assert seen == dict(case='y', ckpt=None, debug=True)
    _fire(fn, ['--some-flag'.replace('some-flag', 'debug'), '--ckpt', 'a-b'])
    assert seen == dict(case='default', ckpt='a-b', debug=True)


def test_bench_spawns_its_own_ranks_when_started_without_a_launcher():
    """`python bench.py --gpus 2` (the driver's command shape, no torch.distributed.run in front) must start 2 ranks
    itself, rendezvous, take the max over ranks and print ONE JSON line with n_gpus == 2.  PWV_BENCH_DRYRUN=control
    swaps the GPU step for a no-op (gloo on CPU) -- the launcher / collective control flow is what is under test."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PWV_BENCH_DRYRUN='control')
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT'):
        env.pop(k, None)
    res = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '2', '--steps', '2', '--warmup', '1', '--full'],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, res.stdout
    out = json.loads(lines[0])
    assert out['n_gpus'] == 2 and out['steps'] == 2 and out['warmup'] == 1
    assert 'scattered over 2 ranks' in out['sharded_generate'] and 'dryrun' in out
    # the job-level number (rank 0's mels -> scatter -> forward -> gather): median of 5 calls, max over ranks per call
    job = out['job']
    assert job['calls'] == 5 and len(job['job_ms_all']) == 5 and job['samples'] == 2 * 160000
    assert abs(job['job_samples_per_s'] * job['job_ms_median'] * 1e-3 - job['samples']) < 1.0


def test_bench_time_sharded_mode_is_strong_scaling():
    """`python bench.py --case bench/c5 --gpus 2 --shard time`: the 60 s utterance of BASELINE config 5 cut along the time axis
    over the ranks (pwv_amd/timeshard.py); one job of fixed size, so the line says "strong" and `value` counts the job's
    samples once.  Control-flow dry run (no kernels) over gloo."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PWV_BENCH_DRYRUN='control')
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT'):
        env.pop(k, None)
    res = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--case', 'bench/c5', '--gpus', '2', '--shard', 'time',
                          '--steps', '2', '--warmup', '1', '--full'], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    out = json.loads([l for l in res.stdout.splitlines() if l.startswith('{')][0])
    assert out['n_gpus'] == 2 and out['scaling'] == 'strong'
    assert 'time-sharded x2' in out['config']['parallelism'] and '6160 samples' in out['config']['parallelism']
    assert 'cut into 2 time shards' in out['sharded_generate']
    assert out['job']['samples'] == 960000 and 'generate_time_sharded_ranks' in out['job']['what'] and out['job']['job_samples_per_s'] > 0
    assert abs(out['value'] * out['ms_per_step'] * 1e-3 - 960000) < 1.0          # the job's samples, counted once per step


def test_bench_plain_run_times_only_the_steps_and_dumps_the_last_one(tmp_path):
    """`python bench.py --gpus 1 --steps N --warmup W --dump-outputs DIR` without --full: the contract fields, N timed steps,
    none of the extra legs, and the last timed step's waveform as DIR/waveform.npy.  Control-flow dry run (no kernels)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PWV_BENCH_DRYRUN='control')
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT', 'PWV_BENCH_FORCE_DIST'):
        env.pop(k, None)
    res = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1',
                          '--dump-outputs', str(tmp_path / 'out')], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, res.stdout
    out = json.loads(lines[0])
    for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
        assert k in out, k
    assert out['steps'] == 3 and out['warmup'] == 1 and out['unit'] == 'samples/s' and out['higher_is_better'] is True
    assert abs(out['value'] * out['ms_per_step'] * 1e-3 - 160000) < 1.0
    for k in ('f32_exact', 'roofline', 'range_guard', 'short_input', 'cpu_baseline', 'job'):
        assert k not in out, k
    assert sorted(os.listdir(tmp_path / 'out')) == ['waveform.npy']
    w = np.load(tmp_path / 'out' / 'waveform.npy')
    assert w.shape == (1, 160000, 1) and w.dtype == np.float32


def test_bench_dump_outputs_samples_what_exceeds_the_budget(tmp_path):
    """An output larger than its share of the --dump-outputs budget is written as a fixed, seeded sample of its elements."""
    import bench
    a = np.arange(3000, dtype=np.float64).reshape(3, 1000)
    small = np.ones((2, 5), dtype=np.float32)
    bench.dump_outputs(str(tmp_path / 'x'), {'big': a, 'small': small}, budget=2 * 4 * 500)
    bench.dump_outputs(str(tmp_path / 'y'), {'big': a, 'small': small}, budget=2 * 4 * 500)
    assert sorted(os.listdir(tmp_path / 'x')) == ['big_sample.npy', 'small.npy']
    s = np.load(tmp_path / 'x' / 'big_sample.npy')
    assert s.dtype == np.float32 and s.shape == (500,) and np.all(np.diff(s) > 0) and np.isin(s, a).all()
    assert np.array_equal(s, np.load(tmp_path / 'y' / 'big_sample.npy'))
    assert np.array_equal(np.load(tmp_path / 'x' / 'small.npy'), small)


@pytest.mark.parametrize('case,precision,name', [('bench/c3', 'f16x3', 'c3'), ('bench/c4', 'f16x3', 'c4'), ('bench/c5', 'f16x3', 'c5'), ('bench/c5', 'f16', 'c5_f16')])
def test_roofline_reproduces_from_the_committed_profiles(case, precision, name):
    """bench.py's `roofline.traffic` / `committed_profile.frac_rocprof` come from profiles/rNN_x_<case>_hbm_traffic.json of the SAME configuration; that
    file in turn follows from raw counter totals, the rocprofv3 average and the bench line of the same set by plain arithmetic
    (tools/profile_round4_summarize.py) -- checked here, so a hand edit or a stale file cannot go unnoticed."""
    import glob
    import json
    import types
    import bench
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tpath = sorted(glob.glob(os.path.join(root, 'profiles', 'r[0-9][0-9]_*_%s_hbm_traffic.json' % name)))[-1]
    tj = json.load(open(tpath))
    bline = [l for l in open(tpath.replace('_hbm_traffic.json', '_bench.json')) if l.startswith('{')][-1]
    b = json.loads(bline)
    roof_b = b['roofline']
    rows = b['config']['utterances_per_gpu'] * b['config']['samples_per_utterance']
    assert tj['rows'] == rows and b['config']['case'] == case and b['precision'] == precision
    # raw counters -> traffic (gfx950: FETCH_SIZE counts 128-byte requests at 64 B)
    assert abs(tj['traffic_bytes_total'] - (2 * tj['FETCH_SIZE_KB_total'] + tj['WRITE_SIZE_KB_total']) * 1024.0) < 1.0
    # the bench line's own per-forward / per-launch figures -> algorithmic bytes of the same launches
    if 'alg_bytes_per_forward' in roof_b:
        layer_bytes = roof_b['alg_bytes_per_net_layer'] // rows
        tail = roof_b.get('tail_net_layers_per_forward', 0) * roof_b.get('alg_bytes_per_tail_net_layer', 0)      # (round 5: last layer + head inside the launch)
        assert roof_b['alg_bytes_per_forward'] == rows * (roof_b['net_layers_per_forward'] * layer_bytes
                                                            - roof_b['first_net_layers_per_forward'] * (layer_bytes // 2 - 4)) + tail
        assert tj['algorithmic_bytes_total'] == tj['forwards'] * roof_b['alg_bytes_per_forward']
        assert tj['launches'] == tj['forwards'] * roof_b['launches_per_forward']
    else:
        assert tj['algorithmic_bytes_total'] == tj['launches'] * roof_b['alg_bytes_per_launch']
    assert abs(tj['ratio'] - tj['traffic_bytes_total'] / tj['algorithmic_bytes_total']) < 1e-12
    assert abs(tj['traffic_bytes_per_launch'] - tj['traffic_bytes_total'] / tj['launches']) < 1e-3
    frac = tj['concurrent_launches'] * tj['algorithmic_bytes_per_launch'] / (tj['rocprof_kernel_us'] * 1e-6) / 8.0e12
    assert abs(tj['frac_rocprof'] - frac) < 1e-12
    # ... and the kernel-stats table of the set holds that average
    stats = open(tpath.replace('_hbm_traffic.json', '_kernel_stats.md')).read()
    assert ('| %.2f |' % tj['rocprof_kernel_us']) in stats
    # what bench.py attaches for this --case
    roof = {'kernel': roof_b['kernel']}
    bench.attach_profile(roof, types.SimpleNamespace(case=case, precision=precision), rows)
    cp = roof['committed_profile']
    assert roof['traffic'] == tj['traffic_bytes_per_launch'] and cp['frac_rocprof'] == tj['frac_rocprof']
    assert roof['traffic_measured_in_run'] is False and cp['measured_in_run'] is False      # (provenance: canned, and labelled so)
    assert cp['source'].startswith('profiles/') and not any(k in roof for k in ('frac_rocprof', 'rocprof_kernel_us', 'traffic_source'))
    assert abs(cp['frac_rocprof'] - roof_b['frac']) < 0.08 * roof_b['frac']      # the profiler costs a few per cent, not more


def test_variable_scopes_are_per_thread():
    """tf.variable_scope is thread-local; so is the restatement's (variables.variable_scope).  Two threads that build models side by
    side must not see each other's prefixes -- with one process-wide stack they read and created each other's variables (a GPU
    test with two serving threads found it: results off by O(1), round 5)."""
    import threading
    from pwv_amd.variables import current_scope, scoped, variable_scope
    seen, go = {}, threading.Barrier(2)

    def work(tag):
        with variable_scope('iaf_vocoder'):
            with variable_scope(tag):
                go.wait()                      # both threads are inside their scopes now
                seen[tag] = (current_scope(), scoped('filter'))
                go.wait()
            with variable_scope('abs_' + tag, absolute=True):
                go.wait()
                seen[tag + '_abs'] = current_scope()
                go.wait()
    ts = [threading.Thread(target=work, args=(t,)) for t in ('a', 'b')]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert seen == {'a': ('iaf_vocoder/a', 'iaf_vocoder/a/filter'), 'b': ('iaf_vocoder/b', 'iaf_vocoder/b/filter'),
                    'a_abs': 'abs_a', 'b_abs': 'abs_b'} and current_scope() == ''


def test_no_vgpr_spills_in_the_layer_kernels():
    """`use_skip_connection: True` (modules.py:147) used to run kernels with 19-37 VGPRs spilled to scratch
    (layer_f16x3_kernel<SKIP = true, ...>: all four variants; layer_f32_kernel<SKIP, COND>: 27-35).  The compiler's own resource
    remarks (`-Rpass-analysis=kernel-resource-usage`, gfx950 device code, no GPU needed) must show no spilled VGPR in any kernel of the
    layer / persistent sources -- except the two variants pinned below, which no default or benchmarked configuration reaches."""
    from tests.util import kernel_resources
    allowed = {      # demangled-name fragment -> most spilled VGPRs tolerated
        'layer_f16x3_kernel<true, true, false, false, false, false>': 3,      # skip sums AND a per-sample condition (transposed conv), residual output
        'layer_f16x3_kernel<false, true, false, true, false, false>': 14,     # per-sample condition, layer 0 NOT folded (PWV_FOLD_FIRST=0 only)
    }
    for src in ('pwv_layer_f16.hip', 'pwv_layer.hip', 'pwv_layer_h16.hip', 'pwv_stack_persist.hip'):
        for name, n in ((k, r['vgpr_spills']) for k, r in kernel_resources(src).items()):
            limit = max([v for k, v in allowed.items() if k in name] or [0])
            assert n <= limit, '%s: %d VGPRs spilled (%s)' % (name, n, src)
