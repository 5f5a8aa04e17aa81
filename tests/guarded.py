"""Guard bands and poisoned allocations for the tests of the HIP library (tests/test_hip_guarded.py, tests/encoder_gpu.py).

PyTorch's caching allocator rounds every request up to 512 bytes or more and hands the last block of a size straight back, so a kernel
that writes a few bytes past its buffer faults nothing, and a region a kernel forgot to write often already holds the right answer.  A
:class:`Guard` takes both covers away.  Every tensor it hands out is a view into a larger uint8 allocation of its own:

    [ front band: GUARD bytes of SENTINEL | the tensor: exactly the bytes asked for | rear band: GUARD bytes of SENTINEL ]

GUARD is a multiple of 512, so the tensor starts at the alignment the allocator gives anyway; the rear band starts at the tensor's last
byte, whatever its size.  ``empty`` tensors are filled with the guard's poison byte (0xFF: NaN as a float, -1 as an int, every bit of a
mask word or z key set), ``zeros`` and ``full`` keep their values.  :meth:`Guard.check` synchronises and asserts that every band of every
allocation made so far still holds the sentinel; a failure names the allocation's call site and the first touched offset.  The guard
keeps every allocation alive until :meth:`Guard.release`, so what a cloud's ``state`` caches is checked too.

How the library's own allocations get there: ``with Guard(poison) as g:`` replaces the name ``torch`` inside
``ken_burns_effect_amd._native`` with a proxy for the time of the block.  The proxy answers ``empty``, ``empty_like``, ``zeros`` and
``full`` with guarded tensors (device and pinned host memory alike) and passes every other attribute through to torch, so the wrappers
run unchanged.  It also empties the kernel set's cached scratch of the tiled render_pointcloud, which would otherwise be one from outside
the block, and puts it back afterwards.  Leaving the block without an exception runs :meth:`Guard.check`.  Tests that call the C entries
through ctypes take their buffers from the same guard: ``g.empty(shape, dtype, shift=k)`` (``shift``: the tensor starts k bytes behind
the front band's end; those k bytes belong to the band).  Without ``with`` a guard intercepts nothing and only allocates and checks.

Out of scope: what the library obtains for itself (csrc/kbe_handoff.hip: the SDMA hand-off's HSA signals and one 64-byte mapped host word) is not guarded.
"""
import sys

import torch

SENTINEL, GUARD = 0xA5, 4096           # the byte of the bands; the size of one band (a multiple of 512)
assert GUARD % 512 == 0

_HERE = __file__[:-1] if __file__.endswith('.pyc') else __file__


def _shape_of(size):
    if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
        size = tuple(size[0])
    return tuple(int(v) for v in size)


def _call_site():
    """file:line (function) of the nearest caller outside this module."""
    f = sys._getframe(1)
    while f is not None and f.f_code.co_filename == _HERE:
        f = f.f_back
    return '?' if f is None else '%s:%d (%s)' % (f.f_code.co_filename, f.f_lineno, f.f_code.co_name)


class _Allocation:
    def __init__(self, whole, front, nbytes, site, what):
        self.whole, self.front, self.nbytes, self.site, self.what = whole, front, nbytes, site, what

    def touched(self):
        """None, or (band, offset): the first byte that no longer holds the sentinel -- as an offset from the tensor's first byte for
        the front band (negative), from the byte behind its last for the rear band."""
        for band, lo, hi, origin in (('front', 0, self.front, self.front), ('rear', self.front + self.nbytes, self.whole.numel(), self.front + self.nbytes)):
            bad = torch.nonzero(self.whole[lo:hi] != SENTINEL)
            if bad.numel():
                return band, lo + int(bad[0]) - origin
        return None


class _TorchProxy:
    """``torch`` as ken_burns_effect_amd._native sees it inside a guard's block: the allocating functions are the guard's."""

    def __init__(self, guard):
        self._guard = guard

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *size, dtype=None, device=None, pin_memory=False):
        return self._guard.empty(_shape_of(size), dtype, device, pin_memory)

    def empty_like(self, t):
        assert t.is_contiguous(), 'the wrappers only ask for tensors like contiguous ones'
        return self._guard.empty(tuple(t.shape), t.dtype, t.device)

    def zeros(self, *size, dtype=None, device=None, pin_memory=False):
        return self._guard.full(_shape_of(size), 0, torch.get_default_dtype() if dtype is None else dtype, device, pin_memory)

    def full(self, size, fill_value, dtype=None, device=None, pin_memory=False):
        return self._guard.full(_shape_of((size,)), fill_value, dtype, device, pin_memory)


class Guard:
    def __init__(self, poison=0xFF):
        assert 0 <= int(poison) <= 255
        self.poison = int(poison)
        self.allocations = []
        self._saved = None

    # -- allocation ---------------------------------------------------------------------
    def _allocate(self, shape, dtype, device, pin_memory, shift, what):
        dtype = torch.get_default_dtype() if dtype is None else dtype
        device = torch.device('cpu' if device is None else device)
        item = torch.empty(0, dtype=dtype).element_size()
        numel = 1
        for v in shape:
            numel *= v
        nbytes, front = numel * item, GUARD + int(shift)
        assert shift >= 0 and (shift % item == 0 or item == 1), 'a shifted tensor must still be aligned to its element size'
        whole = torch.empty(front + nbytes + GUARD, dtype=torch.uint8, device=device, pin_memory=bool(pin_memory))
        whole.fill_(SENTINEL)
        alloc = _Allocation(whole, front, nbytes, _call_site(), '%s %s %s%s' % (what, tuple(shape), str(dtype).replace('torch.', ''), ', pinned' if pin_memory else ''))
        self.allocations.append(alloc)
        return whole[front:front + nbytes]

    def empty(self, shape, dtype=None, device=None, pin_memory=False, shift=0):
        """torch.empty(shape, ...) between two bands, every byte of it the poison; `shift`: that many bytes behind the front band's end."""
        shape = _shape_of((shape,))
        raw = self._allocate(shape, dtype, device, pin_memory, shift, 'empty')
        raw.fill_(self.poison)
        return raw.view(torch.get_default_dtype() if dtype is None else dtype).view(shape)

    def full(self, shape, value, dtype=None, device=None, pin_memory=False, shift=0):
        """torch.full(shape, value, ...) between two bands."""
        shape = _shape_of((shape,))
        if dtype is None:
            dtype = torch.tensor(value).dtype           # (what torch.full infers: int64 from an int, the default float type from a float)
        t = self._allocate(shape, dtype, device, pin_memory, shift, 'full').view(dtype).view(shape)
        t.fill_(value)
        return t

    # -- the check ------------------------------------------------------------------------
    def problems(self):
        if torch.cuda.is_available() and any(a.whole.is_cuda or a.whole.is_pinned() for a in self.allocations):
            torch.cuda.synchronize()
        found = []
        for a in self.allocations:
            hit = a.touched()
            if hit is not None:
                found.append('%s band of %s allocated at %s: first byte touched at offset %d (%d bytes asked for)' % (hit[0], a.what, a.site, hit[1], a.nbytes))
        return found

    def check(self):
        """Every band of every allocation made so far still holds the sentinel."""
        found = self.problems()
        assert not found, 'written outside a buffer:\n  ' + '\n  '.join(found)

    def release(self):
        self.allocations = []

    # -- interception of ken_burns_effect_amd._native ---------------------------------------
    def __enter__(self):
        from ken_burns_effect_amd import _native
        assert self._saved is None and _native.torch is torch, 'guards do not nest'
        kernels = _native._kernels
        self._saved = (kernels, None if kernels is None else kernels._tiled_scratch)
        if kernels is not None:
            kernels._tiled_scratch = {}
        _native.torch = _TorchProxy(self)
        return self

    def __exit__(self, exc_type, exc, tb):
        from ken_burns_effect_amd import _native
        _native.torch = torch
        kernels, scratch = self._saved
        self._saved = None
        if kernels is not None:
            kernels._tiled_scratch = scratch
        elif _native._kernels is not None:
            _native._kernels._tiled_scratch = {}
        if exc_type is None:
            self.check()
        return False
