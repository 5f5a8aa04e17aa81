"""Frames that lie in HBM, reduced on the GPU by an exact area average (include/kbe_area.h: kbe_area_reduce_u8; the arithmetic is defined in
csrc/kbe_area_block.h).  It only reduces: gif.write_gif(size=...) uses it to write a GIF smaller than the render.

Integer arithmetic throughout: per axis, target cell o of n covers [o N, (o + 1) N) and source cell s of N covers [s n, (s + 1) n) of an
axis of N n units; a source pixel weighs in with the overlap of its cell and the target's, per axis; the weighted sum S over the source
becomes (2 S + W H) // (2 W H), the mean rounded half up.  The same size copies.  The project's own definition, not Pillow's: Pillow's BOX
filter rounds between its two passes and differs by a count here and there (tests/test_area_stream.py).

This is the only module that names the entries of kbe_area.h: they are exported by libkbe_hip.so beside those of kbe.h and kbe_gif.h and typed
from their own header, the way gif.py types its own.  No fallback: without the HIP library every call here raises.
"""
import ctypes
import os

from . import _cabi, _native

HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'kbe_area.h')
ABI_VERSION = 1
MAX_SIDE = 65535
_lib = None
_protos = None


def prototypes():
    """{entry: (restype, [argtypes])} of every entry include/kbe_area.h declares, in its order, read once."""
    global _protos
    if _protos is None:
        if not os.path.exists(HEADER_PATH):
            raise _native.KbeError('%s is missing: the binding takes the types of the area entries of libkbe_hip.so from it' % HEADER_PATH)
        with open(HEADER_PATH) as f:
            _protos = _cabi.prototypes(f.read(), 'KBE_AREA_API')
    return _protos


def load():
    """libkbe_hip.so once more, through a handle of this module's own, its area entries typed from include/kbe_area.h."""
    global _lib
    if _lib is None:
        _native.load()                                                     # (says what to do when the library has not been built)
        lib = ctypes.CDLL(_native.LIB_PATH)
        for name in prototypes():
            if not hasattr(lib, name):
                raise _native.KbeError('libkbe_hip.so does not export %s (stale build?)' % name)
        _cabi.bind(lib, prototypes())
        if lib.kbe_area_abi_version() != ABI_VERSION:
            raise _native.KbeError('libkbe_hip.so area ABI %d != expected %d' % (lib.kbe_area_abi_version(), ABI_VERSION))
        _lib = lib
    return _lib


def _raw(name, *args):
    """The entry `name` of include/kbe_area.h with plain Python values -> what it returns; a surplus argument, which cdecl lets through, is refused here."""
    proto = prototypes().get(name)
    if proto is None:
        raise _native.KbeError('%s is not an entry of include/kbe_area.h' % name)
    if len(args) != len(proto[1]):
        raise _native.KbeError('%s takes %d arguments, got %d' % (name, len(proto[1]), len(args)))
    return getattr(load(), name)(*args)


def _call(name, *args):
    """An entry that returns a status: KbeError with the library's text unless KBE_OK."""
    rc = _raw(name, *args)
    if rc != 0:
        raise _native.KbeError('%s failed (%d): %s' % (name, rc, _native.load().kbe_last_error().decode()))


def size_for(W, H, width=None, height=None):
    """(w, h) of a reduction of W x H frames to `width`, to `height` or to both.  A side that is not given keeps the aspect ratio, rounded
    half up in integers and never below one pixel: height = max(1, (H * width + W // 2) // W), and the same with the sides exchanged.
    Neither: (W, H).  A target larger than the source is refused: the reduction only reduces."""
    W, H = int(W), int(H)
    if not (1 <= W <= MAX_SIDE and 1 <= H <= MAX_SIDE):
        raise ValueError('size_for takes a source of 1..%d pixels a side, not %dx%d' % (MAX_SIDE, W, H))
    w = None if width is None else int(width)
    h = None if height is None else int(height)
    if w is None and h is None:
        return W, H
    if (w is not None and not 1 <= w <= W) or (h is not None and not 1 <= h <= H):
        raise ValueError('a size of %sx%s from %dx%d frames: the sides are 1..%d and 1..%d, frames are only reduced'
                         % ('?' if w is None else w, '?' if h is None else h, W, H, W, H))
    if h is None:
        h = max(1, (H * w + W // 2) // W)
    elif w is None:
        w = max(1, (W * h + H // 2) // H)
    return w, h


def reduce(frames_in_hbm, w, h):
    """uint8 [n,H,W,3] frames in HBM -> uint8 [n,h,w,3] on the same device, w <= W and h <= H: the exact area average (kbe_area_reduce_u8).
    Asynchronous on the current stream."""
    import torch
    frames = frames_in_hbm
    if not (torch.is_tensor(frames) and frames.dim() == 4 and frames.size(3) == 3 and frames.size(0) >= 1):
        raise _native.KbeError('area.reduce takes a uint8 [n,H,W,3] tensor on the GPU')
    n, H, W, _ = frames.shape
    w, h = int(w), int(h)
    if not (1 <= w <= W and 1 <= h <= H):
        raise _native.KbeError('area.reduce: %dx%d from %dx%d frames: the sides are 1..%d and 1..%d, frames are only reduced' % (w, h, W, H, W, H))
    base = _native._ptr(frames, torch.uint8).value
    out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=frames.device)
    sources = (ctypes.c_void_p * n)(*[base + i * H * W * 3 for i in range(n)])
    targets = (ctypes.c_void_p * n)(*[out.data_ptr() + i * h * w * 3 for i in range(n)])
    _call('kbe_area_reduce_u8', sources, n, W, H, 3 * W, targets, w, h, 3 * w, _native._stream())
    return out
