"""CPU: the host side of the persistent STREAMING launch (pwv_persist_args.hist, stack_persist_kernel<F32, MODE, false, STREAM = true>):
the new fields of the C ABI and their ctypes mirror, the launcher's refusals (each names its field, none needs a device), a caller
compiled against the shorter struct, and the compiler's resource remarks for the four new instantiations."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_binding_agree_on_the_new_fields(tmp_path):
    """pwv_persist_args ends with `hist` and `hist_row_off[PWV_MAX_NETS]`; the C compiler's sizeof / offsetof equal the ctypes
    mirror's; the struct grew under struct_size, so the version is still 301."""
    from pwv_amd import _lib
    names = [f[0] for f in _lib.PersistArgs._fields_]
    assert names[-2:] == ['hist', 'hist_row_off'] and names[-3] == 'varlen_rows'
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "pwv_hip.h"\nint main(void){ printf("%zu %zu %zu %zu %zu %d\\n", '
           'sizeof(pwv_persist_args), offsetof(pwv_persist_args, hist), offsetof(pwv_persist_args, hist_row_off), '
           'sizeof(((pwv_persist_args*)0)->hist_row_off), sizeof(pwv_stream_args), PWV_HIP_VERSION); return 0; }\n')
    c, exe = str(tmp_path / 't.c'), str(tmp_path / 't')
    with open(c, 'w') as f:
        f.write(src)
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Wextra', '-pedantic', '-Werror', '-I' + os.path.join(ROOT, 'include'), c, '-o', exe])
    got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    P = _lib.PersistArgs
    assert got == [ctypes.sizeof(P), P.hist.offset, P.hist_row_off.offset, P.hist_row_off.size, ctypes.sizeof(_lib.StreamArgs), 301]
    assert P.hist_row_off.size == _lib.PWV_MAX_NETS * ctypes.sizeof(ctypes.c_void_p)
    assert _lib.HEADER_VERSION == 301


def _args(dil, **kw):
    from pwv_amd import _lib
    pa = _lib.PersistArgs()
    pa.G, pa.n_layers, pa.dilations, pa.N, pa.T = 2, len(dil), dil, 3, 800
    pa.precision, pa.workspace = _lib.PREC_F16X3, 0x10000      # (past the NULL-workspace check; nothing is dereferenced on these paths)
    for k, v in kw.items():
        setattr(pa, k, v)
    return pa


def test_launcher_refusals_name_the_field(built_lib):
    """Every refusal of include/pwv_hip.h's list returns PWV_EINVAL (-1) with the field in pwv_last_error(), before a device is
    needed: the pointers here are made up, nothing may be launched or dereferenced."""
    from pwv_amd import _lib
    lib = built_lib
    dil = (ctypes.c_int * 4)(1, 2, 4, 8)
    offs = [(ctypes.c_size_t * 5)(0, 64, 2112, 4160, 6208) for _ in range(2)]
    sa = _lib.StreamArgs()
    sa.hist_rd = sa.hist_wr = 0x20000
    sa.block_stride, sa.slot_tab = 1 << 16, 0x30000

    def launch(pa, with_offs=(0, 1)):
        for g in with_offs:
            pa.hist_row_off[g] = offs[g]
        rc = lib.pwv_wavenet_stack_persist_f32(ctypes.byref(pa), None)
        return rc, lib.pwv_last_error()

    hist = ctypes.addressof(sa)
    # hist with cu_rows: a packed batch has no streaming form
    rc, err = launch(_args(dil, hist=hist, cu_rows=0x1000, unit_map=0x2000, varlen_rows=4800))
    assert rc == -1 and b'hist together with cu_rows' in err, err
    # hist with a precision other than F16X3 / F32
    rc, err = launch(_args(dil, hist=hist, precision=_lib.PREC_F16))
    assert rc == -1 and b'hist needs precision' in err, err
    # hist with a run that starts at x_first without first_fold
    rc, err = launch(_args(dil, hist=hist, x_first=0x4000))
    assert rc == -1 and b'first_fold' in err and b'hist' in err, err
    # hist with a missing hist_row_off[g]
    rc, err = launch(_args(dil, hist=hist), with_offs=(0,))
    assert rc == -1 and b'hist_row_off[1]' in err, err
    # hist->struct_size == 0
    sa.struct_size = 0
    rc, err = launch(_args(dil, hist=hist))
    assert rc == -1 and b'hist->struct_size' in err, err
    sa.struct_size = ctypes.sizeof(_lib.StreamArgs)
    # slot_tab == NULL
    sa.slot_tab = None
    rc, err = launch(_args(dil, hist=hist))
    assert rc == -1 and b'hist->slot_tab' in err, err


def test_a_shorter_callers_struct_is_the_one_shot_launch(built_lib):
    """A caller compiled against the header before `hist` passes struct_size = offsetof(hist); what lies behind it in its memory is
    not read: with garbage there, pwv_persist_workspace_bytes / pwv_persist_short_input say nothing about `hist`.  (The launch itself
    is not called here: where a device is present it would run.  tests/test_gpu_persist.py launches shorter structs.)"""
    from pwv_amd import _lib
    lib = built_lib
    dil = (ctypes.c_int * 4)(1, 2, 4, 8)
    pa = _args(dil)
    pa.struct_size = _lib.PersistArgs.hist.offset
    pa.hist = 0xdeadbeef00                    # garbage behind the caller's struct
    for g in range(_lib.PWV_MAX_NETS):
        ctypes.cast(ctypes.byref(pa, _lib.PersistArgs.hist_row_off.offset + 8 * g), ctypes.POINTER(ctypes.c_uint64))[0] = 0xbad0000 + g
    lib.pwv_persist_workspace_bytes(ctypes.byref(pa))
    assert b'hist' not in lib.pwv_last_error() and b'struct_size' not in lib.pwv_last_error(), lib.pwv_last_error()
    lib.pwv_persist_short_input(ctypes.byref(pa))
    assert b'hist' not in lib.pwv_last_error(), lib.pwv_last_error()
    # the full struct reads nothing new in the two planning calls either: the plan is on rows
    full = _args(dil, hist=0xdeadbeef00)
    lib.pwv_persist_workspace_bytes(ctypes.byref(full))
    assert b'hist' not in lib.pwv_last_error()


def test_the_four_stream_instantiations_spill_nothing():
    """The compiler's resource remarks for pwv_stack_persist.hip (gfx950 device code, no GPU needed) list
    stack_persist_kernel<false|true, 0|2, false, true> -- both arithmetics: the fp32 escape of the issue was not needed -- each with
    0 bytes of scratch and 0 spilled VGPRs."""
    from tests.util import kernel_resources
    res = kernel_resources('pwv_stack_persist.hip')
    demangled = list(res)
    seen = {}
    for name, sc, sp, vg in ((k, r['scratch'], r['vgpr_spills'], r['vgprs']) for k, r in res.items()):
        m = re.search(r'stack_persist_kernel<(true|false), (\d), false, true>', name)
        if m:
            seen[(m.group(1), int(m.group(2)))] = (sc, sp, vg)
    print('STREAM instantiations (scratch, spilled VGPRs, VGPRs):', seen)
    assert sorted(seen) == [('false', 0), ('false', 2), ('true', 0), ('true', 2)], demangled
    for key, (sc, sp, vg) in seen.items():
        assert sc == 0 and sp == 0 and vg <= 256, (key, sc, sp, vg)
    assert not any('stack_persist_kernel<' in n and ', true, true>' in n for n in demangled)      # VARLEN && STREAM is not built
