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
