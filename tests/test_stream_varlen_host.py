"""CPU: the host side of RAGGED streaming pushes (StreamingVocoder.push_varlen; pwv_stream_args.cu_rows; stack_persist_ragged_kernel) --
the bookkeeping function, the field the C ABI gained and its ctypes mirror, the refusals that need no device, and the compiler's
resource remarks for the new kernels.  No GPU needed."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ragged_plan_mixed_fresh_and_running():
    """T_i, the launch list and the prefix sums for fresh / running sessions, a fresh session with one frame included (T = 0: committed,
    left out of the launch), against push_samples per session; per session and history length, history_sources(length, T_i) says which
    rows the carry moves and which the launch stores -- with T_i the session's OWN, which is what the packed carry and kernel use."""
    from pwv_amd.stream import HistoryLayout, history_sources, push_samples, ragged_plan
    hop = 80
    frames = [10, 1, 1, 40, 2, 7]
    fresh = [False, True, False, True, True, False]
    plan = ragged_plan(frames, fresh, hop)
    assert plan.samples == [push_samples(f, fr, hop) for f, fr in zip(frames, fresh)] == [800, 0, 80, 3120, 80, 560]
    assert plan.launch == [0, 2, 3, 4, 5]                       # session 1: fresh, one frame, T = 0
    assert plan.cu_rows == [0, 800, 880, 4000, 4080, 4640]
    # T / hop + 1 frames each: a running session's kept frame + its f, a fresh one's f
    per = [frames[i] + (0 if fresh[i] else 1) for i in plan.launch]
    assert per == [plan.samples[i] // hop + 1 for i in plan.launch] == [11, 2, 40, 2, 8]
    assert plan.cu_frames == [0, 11, 13, 53, 55, 63]
    lay = HistoryLayout([[1, 2, 4, 512], [1, 96, 200]])
    for k, i in enumerate(plan.launch):
        T = plan.cu_rows[k + 1] - plan.cu_rows[k]
        assert T == plan.samples[i]
        for _, length, _ in lay.carry:
            src = history_sources(length, T)
            moved = [s for s in src if s[0] == 'carry']
            stored = [s for s in src if s[0] == 'chunk']
            assert len(moved) == max(length - T, 0) and len(stored) == min(length, T)
            # the stored rows are the chunk's LAST rows of this session: row t goes to k = t + length - T_i
            assert stored == [('chunk', t) for t in range(max(T - length, 0), T)]
            assert moved == [('carry', kk + T) for kk in range(max(length - T, 0))]
    # all fresh with one frame: nothing launches
    empty = ragged_plan([1, 1], [True, True], hop)
    assert empty.samples == [0, 0] and empty.launch == [] and empty.cu_rows == [0] and empty.cu_frames == [0]
    with pytest.raises(ValueError):
        ragged_plan([0, 3], [True, False], hop)
    with pytest.raises(ValueError):
        ragged_plan([2], [True, False], hop)


def test_stream_args_gained_cu_rows_at_its_end(tmp_path):
    """pwv_stream_args ends with `cu_rows`; the C compiler's sizeof / offsetof equal the ctypes mirror's; the struct grew under
    struct_size, so the version is still 301."""
    from pwv_amd import _lib
    names = [f[0] for f in _lib.StreamArgs._fields_]
    assert names[-1] == 'cu_rows' and names[-2] == 'n_carry'
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "pwv_hip.h"\nint main(void){ printf("%zu %zu %zu %d\\n", '
           'sizeof(pwv_stream_args), offsetof(pwv_stream_args, cu_rows), offsetof(pwv_stream_args, n_carry), PWV_HIP_VERSION); return 0; }\n')
    c, exe = str(tmp_path / 't.c'), str(tmp_path / 't')
    with open(c, 'w') as f:
        f.write(src)
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Wextra', '-pedantic', '-Werror', '-I' + os.path.join(ROOT, 'include'), c, '-o', exe])
    got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    S = _lib.StreamArgs
    assert got == [ctypes.sizeof(S), S.cu_rows.offset, S.n_carry.offset, 301]
    assert S.cu_rows.offset + S.cu_rows.size == ctypes.sizeof(S)      # the last field
    assert _lib.HEADER_VERSION == 301 and S().struct_size == ctypes.sizeof(S)


def test_refusals_name_hist_cu_rows(built_lib):
    """hist->cu_rows on a launch that is not packed, hist->cu_rows != pwv_persist_args.cu_rows, and pwv_wavenet_layer_stream_f32 with
    hist->cu_rows: each returns PWV_EINVAL (-1) and names the field, before a device is needed (the pointers are made up: every call
    here FAILS validation, nothing may be launched or dereferenced)."""
    from pwv_amd import _lib
    lib = built_lib
    dil = (ctypes.c_int * 4)(1, 2, 4, 8)
    offs = [(ctypes.c_size_t * 5)(0, 64, 2112, 4160, 6208) for _ in range(2)]
    sa = _lib.StreamArgs()
    sa.hist_rd = sa.hist_wr = 0x20000
    sa.block_stride, sa.slot_tab = 1 << 16, 0x30000

    def launch(**kw):
        pa = _lib.PersistArgs()
        pa.G, pa.n_layers, pa.dilations, pa.N, pa.T = 2, 4, dil, 3, 800
        pa.precision, pa.workspace = _lib.PREC_F16X3, 0x10000
        pa.hist = ctypes.addressof(sa)
        for g in range(2):
            pa.hist_row_off[g] = offs[g]
        for k, v in kw.items():
            setattr(pa, k, v)
        rc = lib.pwv_wavenet_stack_persist_f32(ctypes.byref(pa), None)
        return rc, lib.pwv_last_error()

    sa.cu_rows = 0x1000
    rc, err = launch()                                                        # a uniform [N, T] launch
    assert rc == -1 and b'hist->cu_rows' in err and b'not packed' in err, err
    rc, err = launch(cu_rows=0x5000, unit_map=0x2000, varlen_rows=4800)       # packed, another table
    assert rc == -1 and b'hist->cu_rows' in err and b'differs' in err, err
    # (packed with hist->cu_rows == NULL keeps the refusal tests/test_stream_persist_host.py asserts)
    sa.cu_rows = None
    rc, err = launch(cu_rows=0x1000, unit_map=0x2000, varlen_rows=4800)
    assert rc == -1 and b'hist together with cu_rows' in err, err
    # a caller's shorter struct cannot ask for the ragged launch: what lies behind it is not read
    sa.cu_rows = 0x1000
    sa.struct_size = _lib.StreamArgs.cu_rows.offset
    rc, err = launch(cu_rows=0x1000, unit_map=0x2000, varlen_rows=4800)
    assert rc == -1 and b'hist together with cu_rows' in err, err
    sa.struct_size = ctypes.sizeof(_lib.StreamArgs)
    # the per-layer kernels have no packed form
    la = _lib.LayerArgs()
    la.G, la.N, la.T, la.dilation, la.precision = 1, 1, 80, 4, _lib.PREC_F16X3
    sa.block_stride = 32 * 64
    rc = lib.pwv_wavenet_layer_stream_f32(ctypes.byref(la), ctypes.byref(sa), None)
    assert rc == -1 and b'hist->cu_rows' in lib.pwv_last_error(), lib.pwv_last_error()


def _remarks(source):
    from tests.util import kernel_resources
    return [(name, r['scratch'], r['vgpr_spills'], r['vgprs']) for name, r in kernel_resources(source).items()]


def test_the_ragged_kernels_spill_nothing():
    """The compiler's resource remarks (gfx950 device code, no GPU needed) list stack_persist_ragged_kernel<false|true, 0|2> -- both
    arithmetics: the fp32 escape of the issue was not needed (engine.RAGGED_F32) -- and the packed carry kernel, each with 0 bytes of
    scratch, 0 spilled VGPRs and at most 256 VGPRs."""
    from pwv_amd import engine
    seen = {}
    for name, sc, sp, vg in _remarks('pwv_stack_persist.hip'):
        if 'ragged' in name:
            seen[name.split('(')[0].replace('void ', '')] = (sc, sp, vg)
    print('ragged kernels (scratch, spilled VGPRs, VGPRs):', seen)
    assert engine.RAGGED_F32 is True
    assert sorted(k for k in seen if 'stack_persist' in k) == ['pwv::stack_persist_ragged_kernel<%s, %d>' % (a, m)
                                                              for a in ('false', 'true') for m in (0, 2)], seen
    assert 'pwv::stream_carry_ragged_kernel' in seen, seen
    for key, (sc, sp, vg) in seen.items():
        assert sc == 0 and sp == 0 and vg <= 256, (key, sc, sp, vg)


def test_grouped_route_bookkeeping_on_the_cpu():
    """engine.stream_groups: the sessions of a ragged tick grouped by chunk length -- each group's rows and frames of the packed tensors,
    its rows of the slot table, and its share of the packed condition with the projection bank's rows (CPU tensors: no launch)."""
    import torch
    from pwv_amd import engine
    geom = engine.VarlenGeometry([800, 80, 800, 240, 80], 80, 'cpu')
    tab = torch.arange(10, dtype=torch.int32).view(5, 2)
    groups = engine.stream_groups(geom, tab)
    assert [(g.t, g.n, g.frames, g.tab.tolist()) for g in groups] == [(800, 2, 11, [[0, 1], [4, 5]]), (80, 2, 2, [[2, 3], [8, 9]]), (240, 1, 4, [[6, 7]])]
    assert engine.stream_groups(geom, tab) is groups
    F, C = geom.total_frames, 8
    frames = torch.arange(F * C, dtype=torch.float32).view(1, F, C)
    cond = engine.RepeatedCondition(frames, 80, 40, geom.rows)
    p_all = torch.arange(F * 6, dtype=torch.float32).view(F, 6)
    cond.proj_bank = {1: p_all[:, 0:2], 2: p_all[:, 2:6]}
    x = torch.arange(geom.rows, dtype=torch.float32).view(-1, 1)
    out = torch.full_like(x, -1.0)
    for g in groups:
        gc = g.condition(cond, geom)
        assert tuple(gc.frames.shape) == (g.n, g.t // 80 + 1, C) and gc.length == g.t and g.condition(cond, geom) is gc
        assert torch.equal(gc.frames.reshape(-1, C), frames[0][g.frames_idx])
        assert torch.equal(gc.proj_bank[1], p_all[g.frames_idx][:, 0:2]) and torch.equal(gc.proj_bank[2], p_all[g.frames_idx][:, 2:6])
        assert gc.proj_bank[1].stride(0) == gc.proj_bank[2].stride(0) == 6           # one row stride for all nets' columns
        xg = x.index_select(0, g.rows_idx).reshape(g.n, g.t, 1)
        for k in range(g.n):
            assert float(xg[k, 0, 0]) == geom.cu_rows_host[[i for i, t in enumerate(geom.lengths) if t == g.t][k]]
        out.index_copy_(0, g.rows_idx, xg.reshape(-1, 1))
    assert torch.equal(out, x)                                                         # every packed row belongs to exactly one group
