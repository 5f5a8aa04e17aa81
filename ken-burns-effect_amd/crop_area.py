"""Raw frames that lie in HBM, their centred crop reduced on the GPU by an exact area average, in one pass (include/kbe_crop_area.h:
kbe_crop_area_u8; the arithmetic is defined in csrc/kbe_crop_area_block.h on top of csrc/kbe_area_block.h).  It only reduces:
common.render_frames(out_size=...) uses it to deliver a video narrower than the photo it was rendered from.

The crop is the patch cv2.getRectSubPix takes from the frame's centre, the first step of the crop + resize that frames of the photo's own
size go through: per axis it starts on a whole pixel when the frame's side minus the crop's is odd, and half a pixel further when it is
even; a patch pixel is then the raw pixel, (a + b + 1) >> 1 of two raw neighbours or (a + b + c + d + 2) >> 2 of 2 x 2.  The patch is
reduced as area.reduce reduces a frame of the crop's size.  Integers throughout, two roundings: the patch to a byte, then the mean, half up.

This is the only module that names the entries of kbe_crop_area.h: they are exported by libkbe_hip.so beside those of the other headers and
typed from their own header on the package's one handle of that library, the way area.py types its own.  No fallback: without the HIP
library every call here raises.
"""
import os

from . import _cabi, _native, area

HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'kbe_crop_area.h')
ABI_VERSION = 1
HEADER = _cabi.Header(HEADER_PATH, 'KBE_CROP_AREA_API', 'include/kbe_crop_area.h', abi=('kbe_crop_area_abi_version', ABI_VERSION, 'crop-area '))
prototypes = HEADER.prototypes     # {entry: (restype, [argtypes])} of every entry include/kbe_crop_area.h declares, in its order, read once
size_for = area.size_for           # (w, h) of frames `width` wide: the height follows the IMAGE's aspect ratio, as the frames written at full size do


def load():
    """The package's one handle of libkbe_hip.so (_native.load), its crop-area entries typed from include/kbe_crop_area.h the first time it is seen."""
    return HEADER.bind(_native.load())


def _raw(name, *args):
    """The entry `name` of include/kbe_crop_area.h with plain Python values -> what it returns; a surplus argument, which cdecl lets through, is refused."""
    return HEADER.raw(load(), name, *args)


def _call(name, *args):
    """An entry that returns a status: KbeError with the library's text unless KBE_OK."""
    HEADER.call(load(), name, *args)


def reduce(frames_in_hbm, crop, size):
    """uint8 [n,H,W,3] raw frames in HBM, crop = (cw, ch) with cw <= W and ch <= H, size = (w, h) with w <= cw and h <= ch -> uint8 [n,h,w,3]
    on the same device: the centred crop's exact area average (kbe_crop_area_u8).  Asynchronous on the current stream."""
    import torch
    n, H, W, _, sources = _native.frame_pointers(frames_in_hbm, 'crop_area.reduce')
    (cw, ch), (w, h) = (int(v) for v in crop), (int(v) for v in size)
    if not (1 <= cw <= W and 1 <= ch <= H):
        raise _native.KbeError('crop_area.reduce: a crop of %dx%d from %dx%d frames: the sides are 1..%d and 1..%d' % (cw, ch, W, H, W, H))
    if not (1 <= w <= cw and 1 <= h <= ch):
        raise _native.KbeError('crop_area.reduce: %dx%d from a crop of %dx%d: the sides are 1..%d and 1..%d, frames are only reduced' % (w, h, cw, ch, cw, ch))
    out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=frames_in_hbm.device)
    targets = _native.frame_pointers(out, 'crop_area.reduce')[4]
    _call('kbe_crop_area_u8', sources, n, W, H, 3 * W, cw, ch, targets, w, h, 3 * w, _native._stream())
    return out
