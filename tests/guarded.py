"""A test-side allocator: every device buffer the package allocates lies inside a larger, poisoned buffer with guard bands.

    with guarded(engine, stream, graph) as g:
        ...build the store and the model, run the route...
        torch.cuda.synchronize()
        g.check()

Inside the context the name `torch` of every given module is a proxy of the real module that intercepts `empty`, `empty_like`, `zeros`,
`zeros_like` and `full` for device tensors.  An intercepted call allocates ONE uint8 backing tensor of band + nbytes + band bytes, all
0xFF, and returns the middle viewed as the dtype and shape that were asked for:

  * the payload of a floating `empty*` stays as filled: 0xFF.. is a NaN in fp16, fp32 and fp64, so a store that never lands leaves a
    NaN behind instead of whatever the caching allocator's block held before (often: the previous run's correct value);
  * the payload of an INTEGER `empty*` is zeroed, not poisoned: integers here are indices, counts and offsets, and a poisoned one would
    turn a latent uninitialised read into a wild access on a machine that others share.  Such a read is not found by this harness;
  * `zeros*` and `full` payloads hold what was asked for;
  * the bands stay 0xFF unless something stores into them: check() compares them byte for byte (not with isnan: a stray NaN store
    has to show too) and names the allocation, the side and the offset.

What goes to the real torch: CPU and pinned tensors, calls with keyword arguments the proxy does not know, `*_like` of a non-contiguous
tensor, and every other attribute.  Tensor METHODS (`x.new_empty`) never pass through a module's `torch` name: the package does not
use them (tests/test_guarded_host.py asserts that by source search).

The band, 256 KiB by default, is a condition and no measurement: twice the farthest a misplaced row store of these kernels can land,
512 rows (the largest dilation) x 256 B per row of a 64-channel tile32 buffer.  It is a multiple of 4096 bytes, so the payload keeps the
alignment the allocator gave the backing tensor.

What a guarded run does NOT see: a load outside a buffer (a descriptor-bounded one returns zero silently, a plain one reads 0xFF bytes
of a band, which only shows if the value reaches a result), and a stray store that lands farther away than the band."""
import contextlib
import operator
import os
import sys

import torch as _torch

FILL = 0xFF
INTERCEPTED = ('empty', 'empty_like', 'zeros', 'zeros_like', 'full')


class Allocation(object):
    __slots__ = ('backing', 'band', 'nbytes', 'site', 'shape', 'dtype')

    def __init__(self, backing, band, nbytes, site, shape, dtype):
        self.backing, self.band, self.nbytes, self.site, self.shape, self.dtype = backing, band, nbytes, site, shape, dtype

    def payload(self):
        return self.backing[self.band:self.band + self.nbytes].view(self.dtype).view(self.shape)

    def bands(self):
        """(('front', bytes, offset of its first byte relative to the payload), ('behind', ...))"""
        return (('front', self.backing[:self.band], -self.band), ('behind', self.backing[self.band + self.nbytes:], self.nbytes))


def _default_want_device(device) -> bool:
    return device.type == 'cuda'


class Guard(object):
    """The proxy's state: the registry of guarded allocations (strong references, so no block goes back to the allocator -- and to an
    unguarded owner -- before check() has looked at its bands) and the check."""

    def __init__(self, band_bytes=256 * 1024, want_device=_default_want_device):
        assert band_bytes > 0 and band_bytes % 4096 == 0, 'band_bytes must be a positive multiple of 4096'
        self.band_bytes = int(band_bytes)
        self.want_device = want_device
        self.allocations = []
        self._files = set()

    # -- the registry ------------------------------------------------------------------------------------------------------
    def find(self, tensor):
        """The Allocation that holds `tensor`'s first byte in its payload, or None."""
        if tensor is None:
            return None
        p = tensor.data_ptr()
        for a in self.allocations:
            lo = a.backing.data_ptr() + a.band
            if a.backing.device == tensor.device and (lo <= p < lo + a.nbytes or (a.nbytes == 0 and p == lo)):
                return a
        return None

    def holds(self, tensor) -> bool:
        return self.find(tensor) is not None

    def sites(self):
        return sorted({a.site for a in self.allocations})

    # -- an intercepted call ------------------------------------------------------------------------------------------------
    def _site(self):
        """file:line of the nearest caller that is code of a guarded module (else of the nearest caller outside this file)."""
        f = sys._getframe(1)
        first = None
        while f is not None:
            name = f.f_code.co_filename
            if name != __file__ and first is None:
                first = f
            if name in self._files:
                return '%s:%d' % (os.path.basename(name), f.f_lineno)
            f = f.f_back
        return '%s:%d' % (os.path.basename(first.f_code.co_filename), first.f_lineno) if first is not None else '?'

    def allocate(self, shape, dtype, device, fill):
        """`fill`: None (empty: poison floats, zero integers), or the value every element holds."""
        shape = tuple(int(v) for v in shape)
        numel = 1
        for v in shape:
            numel *= v
        itemsize = _torch.empty((), dtype=dtype).element_size()
        nbytes, band = numel * itemsize, self.band_bytes
        backing = _torch.full((band + nbytes + band,), FILL, dtype=_torch.uint8, device=device)
        if backing.is_cuda:
            assert (backing.data_ptr() + band) % 256 == 0, 'the payload lost the allocator\'s alignment'
        a = Allocation(backing, band, nbytes, self._site(), shape, dtype)
        self.allocations.append(a)
        out = a.payload()
        if fill is not None:
            out.fill_(fill)
        elif not (dtype.is_floating_point or dtype.is_complex):
            out.zero_()
        return out

    # -- the check ----------------------------------------------------------------------------------------------------------
    def touched(self):
        """[(call site, shape, dtype, 'front' | 'behind', byte offset of the first touched byte relative to the payload, number of
        touched bytes)] over every registered allocation.  Synchronises; not for use under stream capture."""
        flags, keys = [], []
        for a in self.allocations:
            for side, band, off in a.bands():
                flags.append((band != FILL).any())
                keys.append((a, side, band, off))
        if not flags:
            return []
        hits = _torch.stack([f.to(flags[0].device) for f in flags]).cpu().tolist()      # (one device -> host copy for all of them)
        found = []
        for hit, (a, side, band, off) in zip(hits, keys):
            if hit:
                idx = (band != FILL).nonzero().reshape(-1)
                found.append((a.site, a.shape, a.dtype, side, off + int(idx[0]), int(idx.numel())))
        return found

    def check(self):
        found = self.touched()
        assert not found, 'stores outside %d guarded allocation(s) -- (call site, shape, dtype, side, first byte relative to the ' \
                          'payload, bytes touched): %r' % (len(found), found)


class _TorchProxy(object):
    """Stands in for the module `torch` in a guarded module's namespace."""

    def __init__(self, guard):
        object.__setattr__(self, '_guard', guard)

    def __getattr__(self, name):
        return getattr(_torch, name)

    def __setattr__(self, name, value):
        setattr(_torch, name, value)

    # -- which calls are taken ------------------------------------------------------------------------------------------------
    def _device(self, device):
        """The torch.device of a `device=` argument if the guard wants it, else None."""
        dev = _torch.device(device) if device is not None else _torch.empty(0).device
        return dev if self._guard.want_device(dev) else None

    @staticmethod
    def _size(args):
        """The size of torch.empty(*size) / torch.zeros(*size): integers, or one sequence of integers; None where it is neither."""
        if len(args) == 1 and isinstance(args[0], (tuple, list, _torch.Size)):
            args = tuple(args[0])
        try:
            return None if any(isinstance(v, (bool, float)) for v in args) else tuple(operator.index(v) for v in args)
        except TypeError:
            return None

    def _new(self, name, args, kwargs, fill):
        if set(kwargs) - {'dtype', 'device'}:
            return getattr(_torch, name)(*args, **kwargs)
        size, dev = self._size(args), self._device(kwargs.get('device'))
        if size is None or dev is None or (len(args) == 0):
            return getattr(_torch, name)(*args, **kwargs)
        dtype = kwargs.get('dtype') or _torch.get_default_dtype()
        return self._guard.allocate(size, dtype, dev, fill)

    def _like(self, name, args, kwargs, fill):
        if len(args) != 1 or set(kwargs) - {'dtype', 'device'} or not isinstance(args[0], _torch.Tensor) or not args[0].is_contiguous():
            return getattr(_torch, name)(*args, **kwargs)
        t = args[0]
        dev = self._device(kwargs.get('device') if kwargs.get('device') is not None else t.device)
        if dev is None:
            return getattr(_torch, name)(*args, **kwargs)
        return self._guard.allocate(t.shape, kwargs.get('dtype') or t.dtype, dev, fill)

    def empty(self, *args, **kwargs):
        return self._new('empty', args, kwargs, None)

    def zeros(self, *args, **kwargs):
        return self._new('zeros', args, kwargs, 0)

    def empty_like(self, *args, **kwargs):
        return self._like('empty_like', args, kwargs, None)

    def zeros_like(self, *args, **kwargs):
        return self._like('zeros_like', args, kwargs, 0)

    def full(self, *args, **kwargs):
        # full(size, fill_value, *, dtype, device): without a dtype the real torch infers it from the value; leave that to it
        if len(args) != 2 or set(kwargs) - {'dtype', 'device'} or kwargs.get('dtype') is None or isinstance(args[1], _torch.Tensor):
            return _torch.full(*args, **kwargs)
        size, dev = self._size(args[:1]), self._device(kwargs.get('device'))
        if size is None or dev is None:
            return _torch.full(*args, **kwargs)
        return self._guard.allocate(size, kwargs['dtype'], dev, args[1])


def clear_caches():
    """Drop what the package keeps across calls and would otherwise hand back unguarded (or guarded, to an ordinary run): the persistent
    launches' workspaces, the packed plans, the converted condition, the projection banks, the mel front-end's constants.  Only modules
    that have been imported are touched."""
    engine = sys.modules.get('pwv_amd.engine')
    if engine is not None:
        engine._persist_ws.clear()
        engine._plan_cache.clear()
        engine._cond_cache = None
        engine._bank_cache.clear()
    frontend = sys.modules.get('pwv_amd.audio_frontend')
    if frontend is not None:
        frontend._device_consts.clear()


@contextlib.contextmanager
def guarded(*modules, band_bytes=256 * 1024, want_device=_default_want_device):
    """Replace the name `torch` in each of `modules` (the package's own: engine, stream, graph, modules, audio_frontend, generate, as
    the test needs them) by the proxy; the real module is back on exit, also on an exception.  Yields the Guard.  A guarded test builds
    its VariableStore and model INSIDE the context (clear_caches() runs on entry and on exit), so that the packed weights and the
    projection banks the pack kernels write are banded too."""
    guard = Guard(band_bytes, want_device)
    proxy = _TorchProxy(guard)
    for m in modules:
        assert m.__dict__.get('torch') is _torch, '%s has no module-level name `torch` (or is guarded already)' % m.__name__
        guard._files.add(m.__file__)
    clear_caches()
    done = []
    try:
        for m in modules:
            m.torch = proxy
            done.append(m)
        yield guard
    finally:
        for m in done:
            m.torch = _torch
        clear_caches()
