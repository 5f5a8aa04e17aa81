"""Raw frames that lie in HBM, their centred crop enlarged on the GPU by an exact integer bicubic, in one pass (include/kbe_enlarge.h:
kbe_enlarge_u8; the arithmetic is defined in csrc/kbe_enlarge_block.h).  It only enlarges:
common.render_frames(out_size=..., enlarge=True) uses it to deliver a video wider than the crop it was rendered from, up to 16384 pixels a side.

The crop is the patch cv2.getRectSubPix takes from the frame's centre, the first step of the crop + resize that frames of the photo's own
size go through, as bytes.  The patch is resampled once, straight to the target: a separable Catmull-Rom bicubic (a = -1/2) on half-pixel
centres, the border pixel repeated, its weights 14-bit integers that add up to 16384, first along the rows into bytes, then down the
columns.  Integers throughout, three roundings: the patch, the rows, the columns.  The crop's own size gives the patch itself.

This is the only module that names the entries of kbe_enlarge.h: they are exported by libkbe_hip.so beside those of the other headers and
typed from their own header on the package's one handle of that library.  No fallback: without the HIP library every call here raises.
"""
import os

from . import _cabi, _native, area

HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'kbe_enlarge.h')
ABI_VERSION = 1
MAX_SIDE = 16384                   # csrc/kbe_enlarge_block.h, kMaxOut: the longest side of a target, where the coefficients' products still fit 64 bits
HEADER = _cabi.Header(HEADER_PATH, 'KBE_ENLARGE_API', 'include/kbe_enlarge.h', abi=('kbe_enlarge_abi_version', ABI_VERSION, 'enlarge '))
prototypes = HEADER.prototypes     # {entry: (restype, [argtypes])} of every entry include/kbe_enlarge.h declares, in its order, read once


def size_for(W, H, width):
    """(w, h) of frames `width` wide from a W x H image: the height follows the IMAGE's aspect ratio, as the frames written at full size
    do -- area.size_for's answer up to the image's width, and its rounding beyond it: max(1, (H * width + W // 2) // W)."""
    W, H, width = int(W), int(H), int(width)
    if width <= W:
        return area.size_for(W, H, width=width)
    return width, max(1, (H * width + W // 2) // W)


def load():
    """The package's one handle of libkbe_hip.so (_native.load), its enlarge entries typed from include/kbe_enlarge.h the first time it is seen."""
    return HEADER.bind(_native.load())


def _raw(name, *args):
    """The entry `name` of include/kbe_enlarge.h with plain Python values -> what it returns; a surplus argument, which cdecl lets through, is refused."""
    return HEADER.raw(load(), name, *args)


def _call(name, *args):
    """An entry that returns a status: KbeError with the library's text unless KBE_OK."""
    HEADER.call(load(), name, *args)


def enlarge(frames_in_hbm, crop, size):
    """uint8 [n,H,W,3] raw frames in HBM, crop = (cw, ch) with cw <= W and ch <= H, size = (w, h) with cw <= w <= 16384 and ch <= h <= 16384
    -> uint8 [n,h,w,3] on the same device: the centred crop's exact bicubic enlargement (kbe_enlarge_u8).  Asynchronous on the current stream."""
    import torch
    n, H, W, _, sources = _native.frame_pointers(frames_in_hbm, 'enlarge.enlarge')
    (cw, ch), (w, h) = (int(v) for v in crop), (int(v) for v in size)
    if not (1 <= cw <= W and 1 <= ch <= H):
        raise _native.KbeError('enlarge.enlarge: a crop of %dx%d from %dx%d frames: the sides are 1..%d and 1..%d' % (cw, ch, W, H, W, H))
    if not (cw <= w <= MAX_SIDE and ch <= h <= MAX_SIDE):
        raise _native.KbeError('enlarge.enlarge: %dx%d from a crop of %dx%d: the sides are %d..%d and %d..%d, frames are only enlarged' % (w, h, cw, ch, cw, MAX_SIDE, ch, MAX_SIDE))
    out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=frames_in_hbm.device)
    targets = _native.frame_pointers(out, 'enlarge.enlarge')[4]
    _call('kbe_enlarge_u8', sources, n, W, H, 3 * W, cw, ch, targets, w, h, 3 * w, _native._stream())
    return out
