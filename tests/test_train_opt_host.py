"""CPU: the gradient arena and the fused optimiser (include/pwv_hip_train_opt.h, csrc/pwv_train_opt.hip, train.Trainer(fused=True),
train.DataParallelTrainer) -- the C structs against their ctypes mirrors, the header's symbols, every host-side refusal of the three
entry points, the kernels' resources, the arena layout, the noise schedule of the ranks, the all-reduce helper over gloo at world size 2
and the train/small_dp case.  Nothing here needs a GPU."""
import ctypes
import os
import re
import socket
import subprocess

import numpy as np
import pytest
import torch

from tests.util import kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACK_FIELDS = ['struct_size', 'table', 'block_map', 'table_host', 'block_map_host', 'arena', 'arena_floats', 'n', 'blocks']
ADAM_FIELDS = ['struct_size', 'table', 'block_map', 'table_host', 'block_map_host', 'grad', 'm', 'v', 'shadow', 'arena_floats', 'n', 'blocks',
               'lr_t', 'beta1', 'beta2', 'eps', 'decay', 'grad_scale']


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def test_opt_args_layouts_match_ctypes(tmp_path):
    """The C compiler's sizes and offsets of both structs (gcc -std=c99 -pedantic -Werror) against the ctypes mirrors, and the header's
    constants against _lib's."""
    from pwv_amd import _lib
    assert [n for n, _ in _lib.TrainOptPackArgs._fields_] == PACK_FIELDS and [n for n, _ in _lib.TrainOptAdamArgs._fields_] == ADAM_FIELDS
    probe = (['sizeof(pwv_train_opt_pack_args)'] + ['offsetof(pwv_train_opt_pack_args, %s)' % f for f in PACK_FIELDS]
             + ['sizeof(pwv_train_opt_adam_args)'] + ['offsetof(pwv_train_opt_adam_args, %s)' % f for f in ADAM_FIELDS]
             + ['(size_t)PWV_TRAIN_OPT_REC', '(size_t)PWV_TRAIN_OPT_CHUNK', '(size_t)PWV_TRAIN_OPT_MAX_GRID', '(size_t)PWV_HIP_VERSION'])
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "pwv_hip_train_opt.h"\nint main(void){ printf("%s\\n", %s); return 0; }\n'
           % (' '.join(['%zu'] * len(probe)), ', '.join(probe)))
    c, exe = str(tmp_path / 't.c'), str(tmp_path / 't')
    with open(c, 'w') as f:
        f.write(src)
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Wextra', '-pedantic', '-Werror', '-I' + os.path.join(ROOT, 'include'), c, '-o', exe])
    got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    P, A = _lib.TrainOptPackArgs, _lib.TrainOptAdamArgs
    assert got == ([ctypes.sizeof(P)] + [getattr(P, f).offset for f in PACK_FIELDS] + [ctypes.sizeof(A)] + [getattr(A, f).offset for f in ADAM_FIELDS]
                   + [_lib.TRAIN_OPT_REC, _lib.TRAIN_OPT_CHUNK, _lib.TRAIN_OPT_MAX_GRID, 301])
    assert P().struct_size == ctypes.sizeof(P) and A().struct_size == ctypes.sizeof(A) and _lib.HEADER_VERSION == 301
    assert _lib.TRAIN_OPT_CHUNK == 4 * 256


def test_header_declares_exactly_the_new_symbols():
    """The header declares exactly _lib.TRAIN_OPT_SYMBOLS, disjoint from every older list; the built library exports them; pwv_hip.h and
    its list are what they were."""
    from pwv_amd import _lib
    _lib.build_library()
    code = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'pwv_hip_train_opt.h')).read(), flags=re.S)
    assert sorted(set(re.findall(r'\b(pwv_[a-z0-9_]+)\s*\(', code))) == sorted(_lib.TRAIN_OPT_SYMBOLS) \
        == ['pwv_train_opt_adam_ema_f32', 'pwv_train_opt_pack_f32', 'pwv_train_opt_unpack_f32']
    taken = (set(_lib.EXPORTED_SYMBOLS) | set(_lib.EXTENSION_SYMBOLS) | set(_lib.LIVE_TICK_SYMBOLS) | set(_lib.SCORE_SYMBOLS) | set(_lib.TRAIN_SYMBOLS)
             | set(_lib.TRAIN_LOSS_SYMBOLS) | set(_lib.TRAIN_VARLEN_SYMBOLS) | set(_lib.TRAIN_COND_SYMBOLS))
    assert not set(_lib.TRAIN_OPT_SYMBOLS) & taken and len(_lib.EXPORTED_SYMBOLS) == 52
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(raw, name) for name in _lib.TRAIN_OPT_SYMBOLS)
    raw.pwv_version.restype = ctypes.c_int
    assert raw.pwv_version() == 301
    assert os.path.join(os.path.dirname(_lib.__file__), 'csrc', 'pwv_train_opt.hip') in _lib.CSRC
    assert '#define PWV_HIP_VERSION 301' in open(os.path.join(ROOT, 'include', 'pwv_hip.h')).read()


class _Case(object):
    """Arguments the library accepts up to its launch: host tables that are real, device pointers that are numbers never dereferenced on
    the host.  Three tensors of 5, 1024 and 2049 floats in an arena of 8 + 1024 + 2052 floats."""

    def __init__(self):
        self.table = np.array([[4096, 0, 5], [8192, 8, 1024], [16384, 1032, 2049]], dtype=np.int64)
        self.map = np.array([[0, 0], [1, 0], [2, 0], [2, 1], [2, 2]], dtype=np.int32)
        self.total = 8 + 1024 + 2052

    def common(self):
        return dict(table=4096, block_map=4096, table_host=self.table.ctypes.data, block_map_host=self.map.ctypes.data, arena_floats=self.total,
                    n=3, blocks=5)

    def pack(self):
        from pwv_amd import _lib
        return _lib.TrainOptPackArgs(arena=4096, **self.common())

    def adam(self, **kw):
        from pwv_amd import _lib
        base = dict(grad=4096, m=4096, v=4096, shadow=4096, lr_t=2e-4, beta1=0.9, beta2=0.999, eps=1e-8, decay=0.998, grad_scale=1.0)
        base.update(kw)
        return _lib.TrainOptAdamArgs(**base, **self.common())


ENTRIES = ('pwv_train_opt_pack_f32', 'pwv_train_opt_unpack_f32', 'pwv_train_opt_adam_ema_f32')


def _refused(lib, entry, a, *words):
    code = getattr(lib, entry)(ctypes.byref(a), None)
    msg = lib.pwv_last_error()
    assert code == -1 and entry.encode() in msg, (entry, code, msg)
    for w in words:
        assert w in msg, (entry, w, msg)


def test_opt_refusals_no_gpu(built_lib):
    """Every refusal of the three entry points returns -1 (PWV_EINVAL) with its field named, before anything touches a device (this
    process has none)."""
    for entry in ENTRIES:
        make = (lambda c: c.adam()) if 'adam' in entry else (lambda c: c.pack())
        assert getattr(built_lib, entry)(None, None) == -1 and b'NULL' in built_lib.pwv_last_error()
        for size in (0, -8, 8):
            c = _Case()
            a = make(c)
            a.struct_size = size if size == 0 else ctypes.sizeof(a) + size
            _refused(built_lib, entry, a, b'struct_size')
        fields = ['table', 'block_map', 'table_host', 'block_map_host'] + (['grad', 'm', 'v', 'shadow'] if 'adam' in entry else ['arena'])
        for field in fields:
            c = _Case()
            a = make(c)
            setattr(a, field, None)
            _refused(built_lib, entry, a, b'NULL pointer', (': %s ' % field).encode())
        for field in (['grad', 'm', 'v', 'shadow'] if 'adam' in entry else ['arena']):       # an arena begins on a 16-byte line
            c = _Case()
            a = make(c)
            setattr(a, field, 4096 + 4)
            _refused(built_lib, entry, a, b'16-byte', (': %s ' % field).encode())
        for n in (0, -1):
            c = _Case()
            a = make(c)
            a.n = n
            _refused(built_lib, entry, a, b': n ')
        for blocks in (0, -3):
            c = _Case()
            a = make(c)
            a.blocks = blocks
            _refused(built_lib, entry, a, b': blocks ')
        c = _Case()
        a = make(c)
        a.arena_floats = 0
        _refused(built_lib, entry, a, b'arena_floats')
        for off in (2, 1030, -4):                    # an offset that is no multiple of 4, or negative
            c = _Case()
            c.table[1, 1] = off
            _refused(built_lib, entry, make(c), b'offset', b'record 1', b'multiple of 4')
        for rec, col, val in ((2, 2, 2053), (2, 1, 1040), (0, 1, 1 << 40), (1, 2, 1 << 62)):       # a tensor that overruns the arena
            c = _Case()
            c.table[rec, col] = val
            _refused(built_lib, entry, make(c), b'overruns the arena', ('record %d' % rec).encode())
        for count in (0, -5):
            c = _Case()
            c.table[0, 2] = count
            _refused(built_lib, entry, make(c), b'count', b'record 0')
        c = _Case()
        c.table[1, 0] = 0
        _refused(built_lib, entry, make(c), b'record 1', b'NULL pointer')
        c = _Case()
        c.table[1, 0] = 8194
        _refused(built_lib, entry, make(c), b'record 1', b'4-byte aligned')
        for rec, tensor in ((3, 3), (0, -1)):        # a map record that names no tensor
            c = _Case()
            c.map[rec, 0] = tensor
            _refused(built_lib, entry, make(c), b'block_map record %d' % rec, b'tensor')
        for rec, chunk in ((0, 1), (1, 1), (4, 3), (2, -1)):     # a chunk behind its tensor's end would overrun the arena
            c = _Case()
            c.map[rec, 1] = chunk
            _refused(built_lib, entry, make(c), b'block_map record %d' % rec, b'chunk')


def test_adam_refusals_of_the_scalars_no_gpu(built_lib):
    """Non-finite lr_t / grad_scale / eps, betas and decay outside [0, 1): refused by name.  A negative decay is no EMA, and then shadow
    may be NULL."""
    entry = 'pwv_train_opt_adam_ema_f32'
    c = _Case()
    for bad in (float('nan'), float('inf'), float('-inf')):
        _refused(built_lib, entry, c.adam(lr_t=bad), b'lr_t')
        _refused(built_lib, entry, c.adam(grad_scale=bad), b'grad_scale')
        _refused(built_lib, entry, c.adam(eps=bad), b'eps')
    _refused(built_lib, entry, c.adam(eps=-1e-8), b'eps')
    for bad in (1.0, 1.5, -0.1, float('nan'), float('inf')):
        _refused(built_lib, entry, c.adam(beta1=bad), b'beta1')
        _refused(built_lib, entry, c.adam(beta2=bad), b'beta2')
    for bad in (1.0, 2.0, float('nan'), float('inf')):
        _refused(built_lib, entry, c.adam(decay=bad), b'decay')
    a = c.adam(decay=-1.0)              # (no call here is complete: one that passed every check would launch on a machine with a GPU)
    a.shadow = None
    a.n = 0
    _refused(built_lib, entry, a, b': n ')          # the tables are looked at after the arenas: a NULL shadow was let through
    a = c.adam(decay=0.0)
    a.shadow = None
    _refused(built_lib, entry, a, b': shadow ', b'NULL pointer')


def test_opt_kernel_resources():
    """The compiler's resource remarks (gfx950 device code) for the three kernels: no scratch, no spilled register, no LDS."""
    res = kernel_resources('pwv_train_opt.hip')
    assert len(res) == 3, sorted(res)
    for k in ('opt_pack_kernel', 'opt_unpack_kernel', 'opt_adam_ema_kernel'):
        assert any(k in n for n in res), (k, sorted(res))
    for name, r in res.items():
        assert r['scratch'] == 0 and r['vgpr_spills'] == 0 and r['sgpr_spills'] == 0 and not r['dynamic_stack'] and r['lds'] == 0, (name, r)


# ---- the layout and the schedule ---------------------------------------------------------------------------------------------------------
def test_arena_layout():
    """Sorted names, offsets multiples of 4, no overlap, total = sum of round4(count), the same for any order of the input; the block
    map names every chunk once."""
    from pwv_amd import _lib
    from pwv_amd import train as TR
    shapes = {'iaf/b': (1,), 'iaf/a': (3,), 'cond/dense': (1, 80, 64), 'iaf/z': (2, 64, 64), 'iaf/c': (5,), 'iaf/d': (4,), 'iaf/s': ()}
    names = list(shapes)
    lay = TR.arena_layout(names, shapes)
    assert lay.names == sorted(names)
    assert lay.counts == [int(np.prod(shapes[n])) for n in lay.names]
    assert all(o % 4 == 0 for o in lay.offsets) and lay.offsets[0] == 0
    spans = sorted(zip(lay.offsets, lay.counts))
    assert all(o + c <= o2 for (o, c), (o2, _) in zip(spans, spans[1:]))
    assert all(o2 - (o + c) < 4 for (o, c), (o2, _) in zip(spans, spans[1:]))
    assert lay.total == sum((c + 3) // 4 * 4 for c in lay.counts) and lay.total >= spans[-1][0] + spans[-1][1]
    for order in (list(reversed(names)), sorted(names), names[3:] + names[:3]):
        for form in (dict((n, shapes[n]) for n in order), [shapes[n] for n in order]):
            other = TR.arena_layout(order, form)
            assert (other.names, other.offsets, other.counts, other.total) == (lay.names, lay.offsets, lay.counts, lay.total)
    with pytest.raises(ValueError):
        TR.arena_layout(['a', 'a'], [(1,), (1,)])
    views = lay.views(torch.arange(lay.total, dtype=torch.float32))
    assert [tuple(v.shape) for v in views] == lay.shapes and all(float(v.reshape(-1)[0]) == o for v, o in zip(views, lay.offsets))
    bm = TR.arena_block_map(lay.counts)
    assert bm.dtype == np.int32 and bm.shape == (sum((c + _lib.TRAIN_OPT_CHUNK - 1) // _lib.TRAIN_OPT_CHUNK for c in lay.counts), 2)
    covered = np.zeros(lay.total, dtype=np.int32)
    for i, c in bm:
        lo = c * _lib.TRAIN_OPT_CHUNK
        hi = min(lay.counts[i], lo + _lib.TRAIN_OPT_CHUNK)
        assert lo < hi
        covered[lay.offsets[i] + lo:lay.offsets[i] + hi] += 1
    want = np.zeros(lay.total, dtype=np.int32)
    for o, c in zip(lay.offsets, lay.counts):
        want[o:o + c] = 1
    assert np.array_equal(covered, want)


@pytest.mark.parametrize('world', [1, 2, 3])
def test_noise_schedule_tiles_the_counters(world):
    """Over 3 steps the ranks' counter ranges [offset, offset + N T) tile [0, steps world N T) without gap or overlap, and at every
    step rank r's range is rows r N .. (r + 1) N - 1 of the concatenated [world N, T] batch one process would draw."""
    from pwv_amd import train as TR
    N, T, steps = 2, 208, 3
    ranges = sorted((TR.noise_offset(s, world, r, N, T), TR.noise_offset(s, world, r, N, T) + N * T) for s in range(steps) for r in range(world))
    assert ranges[0][0] == 0 and ranges[-1][1] == steps * world * N * T
    assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
    for s in range(steps):
        for r in range(world):
            assert TR.noise_offset(s, world, r, N, T) == s * (world * N * T) + r * N * T


# ---- the collective ----------------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _inputs(rank):
    rng = np.random.RandomState(40 + rank)
    a = (rng.randn(4099) * np.exp(rng.uniform(-20, 5, 4099))).astype(np.float32)
    a[:3] = (0.0, 1e-30, -3.0)
    return a


def _allreduce_worker(rank, world, port, ret):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from pwv_amd import train as TR
        flat = torch.from_numpy(_inputs(rank).copy())
        out = TR.allreduce_sum_(flat)
        assert out is flat
        flat.mul_(1.0 / world)
        ret[rank] = flat.numpy().tobytes()
        src = torch.from_numpy(_inputs(rank).copy())
        TR.broadcast_(src, 0)
        ret['b%d' % rank] = src.numpy().tobytes()
    finally:
        dist.destroy_process_group()


def test_allreduce_helper_gloo_world2():
    """train.allreduce_sum_ on CPU tensors over gloo, two spawned processes: both ranks end with the same bits, (a + b) / 2 in float32;
    broadcast_ leaves rank 0's tensor on both."""
    import torch.multiprocessing as mp
    ret = mp.Manager().dict()
    mp.spawn(_allreduce_worker, args=(2, _free_port(), ret), nprocs=2, join=True)
    want = ((_inputs(0) + _inputs(1)) * np.float32(0.5)).astype(np.float32)
    assert ret[0] == ret[1] == want.tobytes()
    assert ret['b0'] == ret['b1'] == _inputs(0).tobytes()


# ---- hparams and the refusal ---------------------------------------------------------------------------------------------------------------
def test_small_dp_case_and_the_refusal_of_too_many_gpus():
    """train/small_dp = train/small with num_gpu 2; nothing about it is refused structurally; more ranks than visible devices is refused
    by name before anything else happens (this machine shows fewer than 99)."""
    from pwv_amd import train as TR
    from pwv_amd._lib import PwvError
    from pwv_amd.hparam import hparam as hp

    def plain(d):
        return {k: plain(v) for k, v in d.items()} if isinstance(d, dict) else d

    hp.set_hparam_yaml('train/small')
    small = plain(dict(hp))
    hp.set_hparam_yaml('train/small_dp')
    dp = plain(dict(hp))
    assert TR.refusal() is None
    assert dp['train']['num_gpu'] == 2 and small['train']['num_gpu'] == 1
    for d in (small, dp):
        d['train'] = {k: v for k, v in d['train'].items() if k != 'num_gpu'}
        for k in [k for k in d if 'logdir' in k or k == 'case']:
            del d[k]
    assert small == dp
    assert torch.cuda.device_count() < 99
    env = {k: os.environ.pop(k) for k in ('WORLD_SIZE', 'PWV_TRAIN_DRYRUN_ONE_GPU') if k in os.environ}
    try:
        with pytest.raises(PwvError, match='training refused.*num_gpu 99 exceeds the %d visible' % torch.cuda.device_count()):
            TR.train('train/small_dp', steps=1, gpus=99)
        with pytest.raises(PwvError, match='training refused.*num_gpu 99'):
            TR.train('train/small', steps=1, gpus='99')
        os.environ['PWV_TRAIN_DRYRUN_ONE_GPU'] = '1'
        with pytest.raises(PwvError, match='num_gpu 9 exceeds the 8 ranks'):
            TR.train('train/small', steps=1, gpus=9)
    finally:
        os.environ.pop('PWV_TRAIN_DRYRUN_ONE_GPU', None)
        os.environ.update(env)
        hp.set_hparam_yaml('default')
    assert TR.Trainer.__init__.__defaults__[-1] is False            # the default path is the unfused one
