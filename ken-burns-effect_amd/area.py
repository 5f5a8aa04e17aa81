"""Frames that lie in HBM, reduced on the GPU by an exact area average (include/kbe_area.h: kbe_area_reduce_u8; the arithmetic is defined in
csrc/kbe_area_block.h).  It only reduces: gif.write_gif(size=...) uses it to write a GIF smaller than the render.

Integer arithmetic throughout: per axis, target cell o of n covers [o N, (o + 1) N) and source cell s of N covers [s n, (s + 1) n) of an
axis of N n units; a source pixel weighs in with the overlap of its cell and the target's, per axis; the weighted sum S over the source
becomes (2 S + W H) // (2 W H), the mean rounded half up.  The same size copies.  The project's own definition, not Pillow's: Pillow's BOX
filter rounds between its two passes and differs by a count here and there (tests/test_area_stream.py).

This is the only module that names the entries of kbe_area.h: they are exported by libkbe_hip.so beside those of kbe.h and kbe_gif.h and typed
from their own header on the package's one handle of that library, the way gif.py types its own.  No fallback: without the HIP library every
call here raises.
"""
import os

from . import _cabi, _native

HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'kbe_area.h')
ABI_VERSION = 1
MAX_SIDE = 65535
HEADER = _cabi.Header(HEADER_PATH, 'KBE_AREA_API', 'include/kbe_area.h', abi=('kbe_area_abi_version', ABI_VERSION, 'area '))
prototypes = HEADER.prototypes     # {entry: (restype, [argtypes])} of every entry include/kbe_area.h declares, in its order, read once


def load():
    """The package's one handle of libkbe_hip.so (_native.load), its area entries typed from include/kbe_area.h the first time it is seen."""
    return HEADER.bind(_native.load())


def _raw(name, *args):
    """The entry `name` of include/kbe_area.h with plain Python values -> what it returns; a surplus argument, which cdecl lets through, is refused."""
    return HEADER.raw(load(), name, *args)


def _call(name, *args):
    """An entry that returns a status: KbeError with the library's text unless KBE_OK."""
    HEADER.call(load(), name, *args)


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
    n, H, W, _, sources = _native.frame_pointers(frames_in_hbm, 'area.reduce')
    w, h = int(w), int(h)
    if not (1 <= w <= W and 1 <= h <= H):
        raise _native.KbeError('area.reduce: %dx%d from %dx%d frames: the sides are 1..%d and 1..%d, frames are only reduced' % (w, h, W, H, W, H))
    out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=frames_in_hbm.device)
    targets = _native.frame_pointers(out, 'area.reduce')[4]
    _call('kbe_area_reduce_u8', sources, n, W, H, 3 * W, targets, w, h, 3 * w, _native._stream())
    return out
