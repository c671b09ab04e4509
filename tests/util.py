"""Shared helpers for the parity tests (oracle = checker, HIP path = thing under test)."""
import functools

import numpy as np

from oracle import iaf_oracle as O

# fp32 parity bar (SURVEY.md section 8c / BASELINE.md section 4): max |y - y_fp64| on O(1) outputs
TOL_F32 = 2e-5


def set_hparams(cfg: O.ModelConfig, length=None, batch=None):
    """Point the global hparam singleton at ``cfg`` (what hp.set_hparam_yaml(case) would do)."""
    from pwv_amd.hparam import hparam as hp
    hp.set_hparam_yaml('default')
    m = hp.model
    m.dilations = [list(d) for d in cfg.dilations]
    m.filter_width = cfg.filter_width
    m.residual_channels = cfg.residual_channels
    m.dilation_channels = cfg.dilation_channels
    m.skip_channels = cfg.skip_channels
    m.condition_channels = cfg.condition_channels
    m.use_biases = cfg.use_biases
    m.use_skip_connection = cfg.use_skip_connection
    m.n_iaf = cfg.n_iaf
    m.normalize = cfg.normalize
    m.normalize_cond = cfg.normalize_cond
    m.normalize_wavenet = cfg.normalize_wavenet
    m.cond_upsample_method = cfg.cond_upsample_method
    m.shared_nets = cfg.shared_nets
    hp.signal.n_mels = cfg.n_mels
    hp.signal.hop_length = cfg.hop_length
    if length is not None:
        hp.generate.length = length
    if batch is not None:
        hp.generate.batch_size = batch
    return hp


def run_vocoder_hip(cfg, weights, mel, z, device, precision=None):
    """The HIP path through the reference-shaped host API: IAFVocoder(batch, length)(wav, mel, ...)."""
    import torch
    from pwv_amd.models import IAFVocoder
    from pwv_amd.variables import VariableStore
    set_hparams(cfg)
    store = VariableStore(device=device)
    store.load_dict(weights)
    n, length = z.shape[0], z.shape[1]
    model = IAFVocoder(batch_size=n, length=length, store=store, precision=precision)
    # enqueue-only + verify(): the parity tests must see the REQUESTED arithmetic or an exception -- not the call's own repair
    # (a rerun in exact fp32 would pass any parity bar); tests/test_safe_call.py covers the default, verified form
    out = model(None, torch.from_numpy(mel).to(device), is_training=False, z=torch.from_numpy(z).to(device), verify=False)
    model.verify()          # synchronises; raises PwvRangeError if the split-fp16 range guard fired
    return out.cpu().numpy()


def small_cfg(**kw):
    base = dict(dilations=[[1, 2, 4], [1, 2, 4, 8]], n_iaf=2)
    base.update(kw)
    return O.ModelConfig(**base)


# Conditioning geometry at hops other than 80 (tests/test_gpu_hop_geometry.py, tests/test_hop_geometry_host.py).  2: offset 1, up to 17
# P rows per 32-row unit; 16: below the unit; 32: a frame boundary at row 16 of every unit, power-of-two magic; 48: neither a power of two
# nor a multiple of 32; 96: a multiple of 32 that is no power of two; 256: a power of two above every dilation of the small models.
HOPS = (2, 16, 32, 48, 96, 256)
# hop -> (utterances, samples each) of the one-shot cases: at least 3 frames per utterance, and a total row count that is no multiple of
# 32 wherever the hop allows one (140, 144, 432 rows); 5 to 48 units of 32 rows, so both persistent instantiations can be asked for
HOP_CASES = {2: (2, 70), 16: (3, 48), 32: (3, 96), 48: (3, 144), 96: (2, 288), 256: (2, 768)}


def hop_cfg(hop, **kw):
    """The small two-flow model of the streaming / packed tests (every flow at least 4 layers: shorter stacks have no persistent form)
    at another hop."""
    return small_cfg(dilations=[[1, 2, 4, 8], [1, 2, 4, 8, 16, 32]], hop_length=hop, **kw)


def f16_storage_model(weights, cfg):
    """What the PWV_PREC_F16 build extension computes, restated for the fp64 oracle: the weights as its kernels
    hold them (fp16 after the exp2 scale folding of csrc/pwv_layer_common.h; dense / skip / postprocess1 plain
    fp16; everything at frame rate, biases and postprocess2 stay fp32) and the hook that rounds every activation
    the mode stores as fp16 (oracle.wavenet_forward(act_round=...)).  Returns (weights, act_round)."""
    k_f, k_g = np.float32(-2.8853900817779268), np.float32(-1.4426950408889634)

    def r16(a):
        return np.asarray(a).astype(np.float16).astype(np.float64)

    per_sample_cond = cfg.cond_upsample_method == 'transposed_conv'
    out = {}
    for name, v in weights.items():
        leaf = name.rsplit('/', 1)[1]
        in_stack = '/dilated_stack/' in name
        if in_stack and (leaf in ('filter', 'gate') or (per_sample_cond and leaf in ('gc_filter', 'gc_gate'))):
            k = k_f if leaf in ('filter', 'gc_filter') else k_g
            out[name] = r16(k * v.astype(np.float32)) / np.float64(k)
        elif (in_stack and leaf in ('dense', 'skip')) or leaf == 'postprocess1':
            out[name] = r16(v)
        else:
            out[name] = v
    return out, r16


def untile_f16(buf, rows):
    """fp16 tile32 (64 channels) -> [rows, 64] float64 in channel order (include/pwv_hip.h)."""
    blocks = buf.numel() // 2048
    perm = np.array([16 * s + 8 * (q >> 2) + 4 * h + (q & 3) for s in range(4) for h in range(2) for q in range(8)])
    v = buf.cpu().numpy().astype(np.float64).reshape(blocks, 8, 32, 8).transpose(0, 2, 1, 3).reshape(blocks * 32, 64)[:rows]
    out = np.zeros_like(v)
    out[:, perm] = v
    return out


# ---- the fused gate, tanh(F) * sigmoid(G), over the whole (F, G) plane (tests/test_gate_formula_host.py, tests/test_gpu_gate_plane.py) ----
K_F, K_G = np.float32(-2.8853900817779268), np.float32(-1.4426950408889634)      # kFScale, kGScale of csrc/pwv_layer_common.h
GATE_MUTANTS = ('no_clamp', 'clamp_g_only', 'clamp_at_128', 'scales_swapped', 'one_plus_e1')


def _push_ulp(v, ulps):
    """`v` (fp32, finite and positive where it is moved) pushed by `ulps` units in the last place: the stated accuracy of v_exp_f32 / v_rcp_f32."""
    out = v.copy()
    move = np.isfinite(v) & (v > 0)
    for _ in range(abs(int(ulps))):
        out[move] = np.nextafter(out[move], np.float32(np.inf if ulps > 0 else 0))
    return out


def gate_emulated(F, G, exp_ulp=0, rcp_ulp=0, mutant=None):
    """gate_act of csrc/pwv_layer_common.h restated in numpy, operation by operation in fp32: Fs = fp32(F * kF), Gs = fp32(G * kG) (what the
    packers fold into the weights and P), the one-sided med3 clamp against (-3.0e38, 57.7), two correctly rounded exp2, t = 1 + e2, ONE fused
    e1 * t + t, a correctly rounded reciprocal and the final product.  `exp_ulp` / `rcp_ulp` push both exp2 / the reciprocal by that many
    units in the last place.  `mutant` (one of GATE_MUTANTS) restates a wrong gate instead -- what assert_gate_plane must reject."""
    assert mutant is None or mutant in GATE_MUTANTS, mutant
    f32 = np.float32
    kf, kg = (K_G, K_F) if mutant == 'scales_swapped' else (K_F, K_G)
    hi = f32(128.0) if mutant == 'clamp_at_128' else f32(57.7)
    with np.errstate(all='ignore'):
        fs = np.asarray(F, dtype=f32) * kf
        gs = np.asarray(G, dtype=f32) * kg
        if mutant not in ('no_clamp', 'clamp_g_only'):
            fs = np.clip(fs, f32(-3.0e38), hi)
        if mutant != 'no_clamp':
            gs = np.clip(gs, f32(-3.0e38), hi)
        e1 = _push_ulp(np.exp2(fs.astype(np.float64)).astype(f32), exp_ulp)
        e2 = _push_ulp(np.exp2(gs.astype(np.float64)).astype(f32), exp_ulp)
        t = f32(1) + e2
        den = (e1.astype(np.float64) * t.astype(np.float64) + t.astype(np.float64)).astype(f32)      # (the product is exact in fp64: one rounding)
        rcp = _push_ulp((1.0 / den.astype(np.float64)).astype(f32), rcp_ulp)
        num = (f32(1) + e1) if mutant == 'one_plus_e1' else (f32(1) - e1)
        return num * rcp


_PLANE_FIXED = (2.0 ** -20, 1e-3, 0.1, 0.5, 1, 2, 3, 5, 8, 12, 16, 19, 19.99, 20, 20.01, 22.17, 22.2, 30, 39.99, 40, 40.01, 44.3, 44.4,
                60, 88, 100, 1e4, 1e30)


@functools.lru_cache(maxsize=None)
def gate_plane():
    """(F, G, perm): the fixed grid of 128 F values x 128 G values as two flat fp32 arrays of 16384 pairs, in the order of a fixed seeded
    permutation `perm` of the row-major grid (so that every lane and register position of a kernel sees every regime).  Each axis: 0 and
    both signs of _PLANE_FIXED -- the small arguments, both sides of Fs = 57.7 (|F| = 20), of Fs = 64 (22.18: e1 * t overflows without the
    clamp), of Gs = 57.7 (|G| = 40), of Fs = 128 (44.36: e1 itself overflows), and far beyond --, the rest seeded uniform in (-25, 25)."""
    rng = np.random.RandomState(20)
    fixed = [0.0] + [s * v for v in _PLANE_FIXED for s in (1.0, -1.0)]
    axes = [np.array(fixed + list(rng.uniform(-25, 25, 128 - len(fixed))), dtype=np.float32) for _ in range(2)]
    f2, g2 = np.meshgrid(axes[0], axes[1], indexing='ij')
    perm = rng.permutation(128 * 128)
    F, G = f2.ravel()[perm], g2.ravel()[perm]
    for a in (F, G, perm):
        a.setflags(write=False)
    return F, G, perm


def gate_exact(F, G):
    """tanh(F) / (1 + exp(-G)) in fp64."""
    with np.errstate(over='ignore'):
        return np.tanh(np.asarray(F, dtype=np.float64)) / (1.0 + np.exp(-np.asarray(G, dtype=np.float64)))


def gate_errors(got, F, G):
    """(max absolute error, max relative error where 0.5 <= |F| <= 19.5 and G >= -39.5) of `got` against gate_exact; inf if not finite."""
    got, F, G = (np.asarray(a, dtype=np.float64).ravel() for a in (got, F, G))
    if not np.isfinite(got).all():
        return np.inf, np.inf
    want = gate_exact(F, G)
    err = np.abs(got - want)
    rel = (np.abs(F) >= 0.5) & (np.abs(F) <= 19.5) & (G >= -39.5)
    return float(err.max()), float((err[rel] / np.abs(want[rel])).max()) if rel.any() else 0.0


@functools.lru_cache(maxsize=None)
def gate_bounds():
    """(A, R, worst absolute, worst relative): the bars of assert_gate_plane.  The worst errors of gate_emulated over gate_plane() for the
    nine (exp_ulp, rcp_ulp) in {-1, 0, 1}^2 -- every answer a gate built from v_exp_f32 / v_rcp_f32 at their stated accuracy can give --
    times 4: the factor covers the hardware's argument reduction and the compiler's freedom outside the contract(off) block.  They come
    from the emulation, never from a kernel."""
    F, G, _ = gate_plane()
    errs = [gate_errors(gate_emulated(F, G, e, r), F, G) for e in (-1, 0, 1) for r in (-1, 0, 1)]
    worst_abs, worst_rel = max(a for a, _ in errs), max(r for _, r in errs)
    return 4 * worst_abs, 4 * worst_rel, worst_abs, worst_rel


def assert_gate_plane(got, F, G, extra_abs=0):
    """`got` = tanh(F) * sigmoid(G) as a kernel (or gate_emulated) computed it, against fp64, with A, R = gate_bounds(): everything finite;
    absolute error <= A everywhere; relative error <= R where 0.5 <= |F| <= 19.5 and G >= -39.5; where G <= -40.01 (the gate's clamp holds
    sigmoid at 2^-57.7): |got| <= 4.3e-18 and got is zero or has the sign of F; where |F| >= 20.01 and G >= -39.5 (tanh is +-1 in fp32): got =
    +-sigmoid(G) to R.  `extra_abs` (a scalar or one value per point) is added to every bar: the rounding of an output stored as fp16.
    Returns (max absolute error, max relative error) for the record."""
    A, R = gate_bounds()[:2]
    got, F, G = (np.asarray(a, dtype=np.float64).ravel() for a in (got, F, G))
    extra = np.broadcast_to(np.asarray(extra_abs, dtype=np.float64).ravel(), got.shape)
    assert got.shape == F.shape == G.shape
    bad = ~np.isfinite(got)
    assert not bad.any(), ('not finite', int(bad.sum()), F[bad][:8], G[bad][:8], got[bad][:8])
    want = gate_exact(F, G)
    err = np.abs(got - want)
    bad = err > A + extra
    assert not bad.any(), ('absolute error', int(bad.sum()), float(err.max()), A, F[bad][:8], G[bad][:8], got[bad][:8])
    rel = (np.abs(F) >= 0.5) & (np.abs(F) <= 19.5) & (G >= -39.5)
    bad = rel & (err > R * np.abs(want) + extra)
    assert not bad.any(), ('relative error', int(bad.sum()), float((err[bad] / np.abs(want[bad])).max()), R, F[bad][:8], G[bad][:8], got[bad][:8])
    low = G <= -40.01
    bad = low & ((np.abs(got) > 4.3e-18 + extra) | ((got != 0) & (F != 0) & (np.sign(got) != np.sign(F))))      # (F = 0 has no sign: the bound alone)
    assert not bad.any(), ('below the sigmoid clamp', int(bad.sum()), F[bad][:8], G[bad][:8], got[bad][:8])
    sat = (np.abs(F) >= 20.01) & (G >= -39.5)
    sig = np.sign(F) * gate_exact(np.full_like(G, 1e3), G)
    bad = sat & (np.abs(got - sig) > R * np.abs(sig) + extra)
    assert not bad.any(), ('saturated tanh', int(bad.sum()), F[bad][:8], G[bad][:8], got[bad][:8])
    return float(err.max()), float((err[rel] / np.abs(want[rel])).max())


def saturating_weights(cfg, seed):
    """O.init_weights(cfg, seed) with every filter_bias and gate_bias of the dilated stacks redrawn per channel: with probability 1/2 from
    U(-70, 70), else from N(0, 1), independently for filter and gate.  Nothing else is scaled: biases enter the projection P exactly, so
    the model stays well conditioned while a third of its gates run beyond |F| = 20 and a tenth below G = -40 (where gate_act's clamp
    works), next to gates in the ordinary range."""
    w = O.init_weights(cfg, seed=seed)
    rng = np.random.RandomState(7919 + seed)
    for name in w:
        if '/dilated_stack/' in name and name.rsplit('/', 1)[1] in ('filter_bias', 'gate_bias'):
            n = w[name].shape[0]
            wide = rng.uniform(size=n) < 0.5
            w[name] = np.where(wide, rng.uniform(-70, 70, n), rng.randn(n)).astype(np.float32)
    return w


def gate_statistics(weights, mel, z, cfg):
    """The fp64 oracle's forward with every gate pre-activation recorded: (y, share with |F| > 20, share with G < -40, share with |F| < 3 and
    |G| < 3, largest |F|)."""
    seen = []
    O.GATE_PROBE = lambda f, g: seen.append((np.abs(f).ravel(), g.ravel()))
    try:
        y = O.iaf_vocoder_forward(weights, mel, z, cfg)
    finally:
        O.GATE_PROBE = None
    af, g = np.concatenate([a for a, _ in seen]), np.concatenate([b for _, b in seen])
    return y, float((af > 20).mean()), float((g < -40).mean()), float(((af < 3) & (np.abs(g) < 3)).mean()), float(af.max())


DIL7 = [1, 2, 32, 64, 48, 512, 4]      # tests/test_gpu_persist_prefetch.py: every look-back path of the general persistent loop
SATURATED_SEED = 6


@functools.lru_cache(maxsize=None)
def saturated_case(kind):
    """The models of the saturated-gate route tests (tests/test_gpu_gate_plane.py; their shares of saturated gates are asserted in
    tests/test_gate_formula_host.py): (cfg, weights, mel, z).  Shared between the tests, never written to."""
    if kind == 'small':             # the two-flow model of the streaming / packed tests
        cfg, n, length = hop_cfg(80), 2, 480
    elif kind == 'dil7':            # one flow whose persistent launch is the general instantiation at PERSIST_MIN_UNITS = 16
        cfg, n, length = small_cfg(dilations=[DIL7], n_iaf=1), 1, 2080
    elif kind == 'shared':          # one two-output net per flow: the affine in place
        cfg, n, length = hop_cfg(80, shared_nets=True), 2, 160
    elif kind == 'transposed':      # the per-sample condition GEMM inside the layer kernels
        cfg, n, length = hop_cfg(80, cond_upsample_method='transposed_conv'), 2, 240
    else:
        raise KeyError(kind)
    w = saturating_weights(cfg, SATURATED_SEED)
    mel, z = O.synthetic_inputs(n, length, cfg)
    return cfg, w, mel, z


SATURATED_KINDS = ('small', 'dil7', 'shared', 'transposed')


def build_c_abi_smoke(out_path):
    """Compile examples/c_abi_smoke.c (a plain C99 client of the C ABI: raw hipMalloc pointers, no Python / torch)
    with gcc against the in-tree library.  Returns the command's CompletedProcess."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib_dir = os.path.join(root, 'parallel-wavenet-vocoder_amd')
    cmd = ['gcc', '-std=c99', '-Wall', '-D__HIP_PLATFORM_AMD__', os.path.join(root, 'examples', 'c_abi_smoke.c'),
           '-I' + os.path.join(root, 'include'), '-I/opt/rocm/include', '-L' + lib_dir, '-lpwv_hip', '-L/opt/rocm/lib',
           '-lamdhip64', '-lm', '-Wl,-rpath,' + lib_dir, '-Wl,-rpath,/opt/rocm/lib', '-o', out_path]
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def c_struct_probe(struct, fields, tmp_path, extra=()):
    """What the C compiler makes of a struct of include/pwv_hip.h (gcc -std=c99 -pedantic -Werror on a probe program): [sizeof(struct),
    offsetof(struct, f) for f in fields, *extra (further size_t expressions), PWV_HIP_VERSION]."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    probe = ['sizeof(%s)' % struct] + ['offsetof(%s, %s)' % (struct, f) for f in fields] + list(extra)
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "pwv_hip.h"\nint main(void){ printf("%s %%d\\n", %s, PWV_HIP_VERSION); return 0; }\n'
           % (' '.join(['%zu'] * len(probe)), ', '.join(probe)))
    c, exe = str(tmp_path / 't.c'), str(tmp_path / 't')
    with open(c, 'w') as f:
        f.write(src)
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Wextra', '-pedantic', '-Werror', '-I' + os.path.join(root, 'include'), c, '-o', exe])
    return [int(x) for x in subprocess.check_output([exe]).decode().split()]


def _device_compile(source_name, mode):
    """Run the shipped compile command (_lib.device_compile_command) of csrc/<source_name> for the device side alone; returns the
    CompletedProcess (text)."""
    import os
    import subprocess
    from pwv_amd import _lib
    src = os.path.join(os.path.dirname(_lib.__file__), 'csrc', source_name)
    res = subprocess.run(_lib.device_compile_command(src) + ['--cuda-device-only'] + mode + [src], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    return res


_REMARK_FIELDS = (('vgprs', 'VGPRs'), ('agprs', 'AGPRs'), ('sgprs', 'TotalSGPRs'), ('scratch', 'ScratchSize [bytes/lane]'),
                  ('vgpr_spills', 'VGPRs Spill'), ('sgpr_spills', 'SGPRs Spill'), ('lds', 'LDS Size [bytes/block]'))


@functools.lru_cache(maxsize=None)
def kernel_resources(source_name):
    """The compiler's resource remarks (`-Rpass-analysis=kernel-resource-usage`, gfx950 device code, no GPU needed) for every kernel of
    csrc/<source_name> as the library is built: {demangled kernel name: {vgprs, agprs, sgprs, scratch, vgpr_spills, sgpr_spills, lds,
    dynamic_stack}}.  One compile per process and source."""
    import re
    import subprocess
    out = _device_compile(source_name, ['-c', '-Rpass-analysis=kernel-resource-usage', '-o', '/dev/null']).stderr
    blocks = out.split('Function Name: ')[1:]
    assert blocks, out[-2000:]
    names = [b.split()[0] for b in blocks]
    demangled = subprocess.run(['c++filt'] + names, stdout=subprocess.PIPE, text=True).stdout.split('\n')
    res = {}
    for name, block in zip(demangled, blocks):
        vals = {key: int(re.search(r' %s: (\d+)' % re.escape(label), block).group(1)) for key, label in _REMARK_FIELDS}
        vals['dynamic_stack'] = re.search(r'Dynamic Stack: (\w+)', block).group(1) != 'False'
        assert name not in res, name
        res[name] = vals
    return res


@functools.lru_cache(maxsize=None)
def kernel_assembly(source_name):
    """The assembly listing (`-S`) of the device code of csrc/<source_name> as the library is built.  One compile per process and source."""
    return _device_compile(source_name, ['-S', '-o', '-']).stdout


def persist_plan_restated(cus, G, rows, dmax, min_units=0, max_workgroups=0, tail_q=0, tail_dil=0):
    """How a persistent launch deals its rows to workgroups and lays out its workspace, restated from the design (DESIGN.md section 4,
    K1p) and not from csrc/pwv_persist_plan.h: units of 32 rows; one workgroup per CU and net, fewer if that leaves a workgroup
    under `min_units` units (default 4) or `max_workgroups` caps the grid; the look-back reach in units and in workgroups; the
    short-input instantiation (unit_mode 2) iff the reach stays within 32 units, there is more than one workgroup and none has more than
    7 units; the workspace = a 128-byte progress word per workgroup and net + one 256-byte line, an arrival counter per range and, in
    unit mode, a 128-byte word per unit and net, each part rounded up to 256 bytes.  Returns a dict -- or None where the library
    refuses the launch: more than 832 units per workgroup, or a reach of more than 60 workgroups."""
    def cdiv(a, b):
        return -(-a // b)

    def align256(v):
        return cdiv(v, 256) * 256
    units = cdiv(rows, 32)
    wgs = cus // G
    if max_workgroups > 0:
        wgs = min(wgs, max_workgroups // G)
    if min_units <= 0:
        min_units = 4
    nwg = min(wgs, max(1, cdiv(units, min_units)))
    per_wg = cdiv(units, nwg)
    reach = cdiv(dmax, 32)
    plan = dict(units=units, nwg=nwg, per_wg=per_wg, last_wg=(units - 1) // per_wg, reach_wgs=cdiv(reach, per_wg),
                xcd_map=int(nwg % 8 == 0 and (G * nwg) % 8 == 0),
                tail_reach_wgs=cdiv(cdiv(tail_dil, 32), per_wg) if tail_q > 0 else 0,
                unit_mode=2 if (reach <= 32 and nwg > 1 and per_wg <= 7) else 0)
    if per_wg > 832 or plan['reach_wgs'] > 60 or plan['tail_reach_wgs'] > 60:
        return None
    plan['prog_bytes'] = G * nwg * 128
    plan['pair_off'] = align256(plan['prog_bytes'] + 256)
    plan['uprog_off'] = plan['pair_off'] + align256(4 * nwg)
    plan['total'] = plan['uprog_off'] + (align256(G * units * 128) if plan['unit_mode'] else 0)
    return plan
