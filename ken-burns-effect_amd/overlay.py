"""Overlays: an RGBA picture -- a watermark, a caption -- composited onto frames that lie in HBM, in place (include/kbe_overlay.h:
kbe_overlay_u8; the arithmetic is defined in csrc/kbe_overlay_block.h), and what the products need of it: where a layer goes (place), how a
caption fades in and out (opacity_table), the picture of a file (read_rgba) or of a text (caption_image), and the two layers of kbe.py,
Pipeline and slideshow.py (layers_request, layers_for, apply_layers).  Exact and byte-defined, in integers: with the pixel's alpha a and the
frame's opacity in 0..256, e = (a opacity + 128) >> 8 and out = (c (255 - e) + o e + 127) / 255.

This is the only module that names the entries of kbe_overlay.h: they are exported by libkbe_hip.so beside those of the other headers and
typed from their own header on the package's one handle of that library, the way the other frame filters' modules type their own.  No
fallback: without the HIP library every call here raises.
"""
import ctypes
import os

from . import _cabi, _native

HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'kbe_overlay.h')
ABI_VERSION = 1
FRAMES_PER_LAUNCH = 12             # KBE_OVERLAY_FRAMES_PER_LAUNCH: the entry cuts a call's frames into launches of this many
MAX_SIDE = 65535
MAX_OPACITY = 256
ANCHORS = ('top-left', 'top', 'top-right', 'left', 'centre', 'right', 'bottom-left', 'bottom', 'bottom-right')
HEADER = _cabi.Header(HEADER_PATH, 'KBE_OVERLAY_API', 'include/kbe_overlay.h', abi=('kbe_overlay_abi_version', ABI_VERSION, 'overlay '))
prototypes = HEADER.prototypes     # {entry: (restype, [argtypes])} of every entry include/kbe_overlay.h declares, in its order, read once


def load():
    """The package's one handle of libkbe_hip.so (_native.load), its overlay entries typed from include/kbe_overlay.h the first time it is seen."""
    return HEADER.bind(_native.load())


def _raw(name, *args):
    """The entry `name` of include/kbe_overlay.h with plain Python values -> what it returns; a surplus argument, which cdecl lets through, is refused."""
    return HEADER.raw(load(), name, *args)


def _call(name, *args):
    """An entry that returns a status: KbeError with the library's text unless KBE_OK."""
    HEADER.call(load(), name, *args)


# -- the entry on tensors ------------------------------------------------------------------------
def _per_frame(value, n, what, name, low, high):
    """`value`, a whole number or n of them, as a list of n numbers in low..high, or KbeError."""
    try:
        values = [value] * n if isinstance(value, int) and not isinstance(value, bool) else list(value)
        good = len(values) == n and all(isinstance(v, int) and not isinstance(v, bool) and low <= v <= high for v in values)
    except TypeError:
        good = False
    if not good:
        raise _native.KbeError('%s: %s: a whole number or %d of them, one per frame, %d..%d' % (what, name, n, low, high))
    return values


def apply(frames, overlay, x, y, opacity=256):
    """frames: a contiguous uint8 [n,H,W,3] tensor in HBM, changed in place and returned; overlay: a uint8 [h,w,4] tensor on the same device,
    its colour bytes in the frames' channel order, byte 3 a straight alpha; x, y: where its top-left pixel lies in a frame, clipped at the
    frame's edges; opacity: 0..256.  x, y and opacity are each a number, for every frame, or n numbers.  Asynchronous on the current stream."""
    import torch
    what = 'overlay.apply'
    if not (torch.is_tensor(frames) and frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() == 4 and frames.size(3) == 3 and frames.size(0) >= 1 and frames.is_contiguous()):
        raise _native.KbeError('%s takes a contiguous uint8 [n,H,W,3] tensor on the GPU (frames: %s)' % (
            what, '%s %s on %s' % (tuple(frames.shape), frames.dtype, frames.device) if torch.is_tensor(frames) else type(frames).__name__))
    if not (torch.is_tensor(overlay) and overlay.dtype == torch.uint8 and overlay.dim() == 3 and overlay.size(2) == 4 and overlay.size(0) >= 1 and overlay.size(1) >= 1
            and overlay.is_contiguous() and overlay.device == frames.device):
        raise _native.KbeError('%s takes a contiguous uint8 [h,w,4] tensor on the frames\' device, %s (overlay: %s)' % (
            what, frames.device, '%s %s on %s' % (tuple(overlay.shape), overlay.dtype, overlay.device) if torch.is_tensor(overlay) else type(overlay).__name__))
    n, H, W, _, pointers = _native.frame_pointers(frames, what)
    h, w = int(overlay.shape[0]), int(overlay.shape[1])
    if not (1 <= W <= MAX_SIDE and 1 <= H <= MAX_SIDE and w <= MAX_SIDE and h <= MAX_SIDE):
        raise _native.KbeError('%s: frames of %d x %d and an overlay of %d x %d: 1..%d either way' % (what, W, H, w, h, MAX_SIDE))
    table = [(ctypes.c_int32 * n)(*_per_frame(v, n, what, name, low, high))
             for v, name, low, high in ((x, 'x', -MAX_SIDE, MAX_SIDE), (y, 'y', -MAX_SIDE, MAX_SIDE), (opacity, 'opacity', 0, MAX_OPACITY))]
    _call('kbe_overlay_u8', pointers, n, W, H, 3 * W, _native._ptr(overlay, torch.uint8), w, h, 4 * w, table[0], table[1], table[2], _native._stream())
    return frames


# -- where and when ------------------------------------------------------------------------------
def explicit(anchor):
    """(X, Y) of an explicit position "X,Y", or None for anything else."""
    if isinstance(anchor, str) and anchor.count(',') == 1:
        parts = [p.strip() for p in anchor.split(',')]
        if all(p.lstrip('-').isdigit() and p.count('-') <= 1 for p in parts):
            return int(parts[0]), int(parts[1])
    return None


def place(anchor, W, H, w, h, margin):
    """(x, y) of the top-left pixel of a w x h layer in a W x H frame: at one of ANCHORS, `margin` pixels off the edges the anchor names and
    centred along the others, or at an explicit "X,Y".  ValueError for anything else."""
    at = explicit(anchor)
    if at is not None:
        return at
    if anchor not in ANCHORS:
        raise ValueError('%s: %s, or X,Y' % (anchor, ', '.join(ANCHORS)))
    W, H, w, h, margin = int(W), int(H), int(w), int(h), int(margin)
    x = margin if anchor.endswith('left') else W - w - margin if anchor.endswith('right') else (W - w) // 2
    y = margin if anchor.startswith('top') else H - h - margin if anchor.startswith('bottom') else (H - h) // 2
    return x, y


def opacity_table(n, first, last, fade, peak=256):
    """The opacities of a layer over n frames: 0 outside the window [first, last); inside it they rise over the first `fade` frames by
    transition.progress_table(fade) scaled to `peak` (rounded to nearest), hold `peak`, and fall mirrored over the last `fade` frames.
    2 fade <= last - first, otherwise ValueError."""
    from .transition import progress_table
    n, first, last, fade, peak = int(n), int(first), int(last), int(fade), int(peak)
    if not (0 <= first <= last <= n and 0 <= peak <= MAX_OPACITY):
        raise ValueError('overlay.opacity_table: a window [%d, %d) of %d frames and a peak of %d: 0 <= first <= last <= n, the peak 0..%d' % (first, last, n, peak, MAX_OPACITY))
    if fade < 0 or 2 * fade > last - first:
        raise ValueError('overlay.opacity_table: fade = %d: 0..%d, half of the window\'s %d frames' % (fade, (last - first) // 2, last - first))
    ramp = [(p * peak + 128) >> 8 for p in progress_table(fade)]
    return [0] * first + ramp + [peak] * (last - first - 2 * fade) + ramp[::-1] + [0] * (n - last)


# -- the pictures --------------------------------------------------------------------------------
def read_rgba(path, bgr):
    """A picture file as a uint8 [h,w,4] array with a straight alpha (255 where the file has none), read with Pillow; bgr: the colour bytes
    B, G, R, the order of the frames unless --pretrained-estim.  OSError (Pillow's) for a file that cannot be read."""
    import numpy as np
    from PIL import Image
    with Image.open(path) as picture:
        rgba = np.asarray(picture.convert('RGBA'), dtype=np.uint8)
    return np.ascontiguousarray(rgba[:, :, [2, 1, 0, 3]] if bgr else rgba)


def caption_mask(text, size, font=None):
    """(the glyph mask of `text` as a uint8 [th,tw] array: Pillow's, 0..255; nothing else of Pillow enters a caption).  The text may hold
    line breaks; size: the font's, in pixels; font: the path of a TrueType file, or None for Pillow's built-in scalable face."""
    import numpy as np
    from PIL import Image, ImageDraw, ImageFont
    face = ImageFont.truetype(font, int(size)) if font else ImageFont.load_default(int(size))
    left, top, right, bottom = ImageDraw.Draw(Image.new('L', (1, 1), 0)).multiline_textbbox((0, 0), text, font=face)
    mask = Image.new('L', (max(1, right - left), max(1, bottom - top)), 0)
    ImageDraw.Draw(mask).multiline_text((-left, -top), text, fill=255, font=face)
    return np.asarray(mask, dtype=np.uint8)


def over_plate(mask, colour, plate):
    """A text of one colour (R, G, B) whose alpha is `mask`, composited with `over` onto a plate of one (R, G, B, A), both straight: uint8
    [h,w,4], R, G, B, A.  In whole numbers, rounded to nearest: with A = 255 m + pa (255 - m) (the alpha, times 255^2) the alpha is
    A / 255 and a colour byte (255 m text + pa (255 - m) plate) / A, 0 where A = 0."""
    import numpy as np
    m = np.asarray(mask, dtype=np.int64)
    pa = int(plate[3])
    A = 255 * m + pa * (255 - m)
    out = np.zeros(m.shape + (4,), np.uint8)
    for k in range(3):
        num = 255 * m * int(colour[k]) + pa * (255 - m) * int(plate[k])
        out[:, :, k] = np.where(A > 0, (2 * num + A) // np.maximum(2 * A, 1), 0)
    out[:, :, 3] = (A + 127) // 255
    return out


def caption_image(text, size, colour=(255, 255, 255), plate=(0, 0, 0, 128), font=None, bgr=True):
    """The picture of a caption: uint8 [h,w,4] with a straight alpha -- the text in `colour` (R, G, B), its glyph mask Pillow's
    (caption_mask), composited with `over` onto a plate (R, G, B, A) that is the text's box plus size // 2 on every side (over_plate);
    bgr: the colour bytes in the frames' order B, G, R."""
    import numpy as np
    size = int(size)
    if not isinstance(text, str) or not text.strip():
        raise ValueError('an empty caption')
    if size < 4:
        raise ValueError('a caption of size %d: 4 pixels or more' % size)
    for value, count in ((colour, 3), (plate, 4)):
        if len(value) != count or not all(isinstance(v, int) and 0 <= v <= 255 for v in value):
            raise ValueError('a caption\'s colour %r: %d whole numbers 0..255' % (value, count))
    mask = caption_mask(text, size, font)
    pad = size // 2
    whole = np.zeros((mask.shape[0] + 2 * pad, mask.shape[1] + 2 * pad), np.uint8)
    whole[pad:pad + mask.shape[0], pad:pad + mask.shape[1]] = mask
    picture = over_plate(whole, colour, plate)
    return np.ascontiguousarray(picture[:, :, [2, 1, 0, 3]] if bgr else picture)


# -- the two layers of the products --------------------------------------------------------------
OPTIONS = ('overlay', 'overlay_at', 'overlay_opacity', 'caption', 'caption_at', 'caption_size', 'font', 'overlay_margin')
ENVIRONMENT = {'overlay': 'KBE_OVERLAY', 'overlay_at': 'KBE_OVERLAY_AT', 'overlay_opacity': 'KBE_OVERLAY_OPACITY', 'caption': 'KBE_CAPTION', 'caption_at': 'KBE_CAPTION_AT',
               'caption_size': 'KBE_CAPTION_SIZE'}


def _whole(value, least):
    """A whole number `least` or more from a number or its text, or None."""
    if isinstance(value, str) and value.strip().isdigit():
        value = int(value)
    return value if isinstance(value, int) and not isinstance(value, bool) and value >= least else None


def layers_request(overlay=None, overlay_at=None, overlay_opacity=None, caption=None, caption_at=None, caption_size=None, font=None, overlay_margin=None, environment=True):
    """What the products were told of the two layers -- kbe.py's options, Pipeline's keyword arguments, else (environment) their twins
    KBE_OVERLAY, KBE_OVERLAY_AT, KBE_OVERLAY_OPACITY, KBE_CAPTION, KBE_CAPTION_AT, KBE_CAPTION_SIZE -- checked as far as it can be without a
    frame: None without a layer, else {'overlay': path or None, 'overlay_at', 'overlay_opacity': 1..256, 'caption': text or None,
    'caption_at', 'caption_size': pixels or None, 'font', 'overlay_margin': pixels or None}.  ValueError whose text begins with the option at fault."""
    import math
    told = dict(overlay=overlay, overlay_at=overlay_at, overlay_opacity=overlay_opacity, caption=caption, caption_at=caption_at, caption_size=caption_size, font=font,
                overlay_margin=overlay_margin)
    if environment:
        for name, variable in ENVIRONMENT.items():
            if told[name] is None:
                told[name] = os.environ.get(variable) or None
    for name, layer in (('overlay_at', 'overlay'), ('overlay_opacity', 'overlay'), ('caption_at', 'caption'), ('caption_size', 'caption'), ('font', 'caption')):
        if told[name] is not None and told[layer] is None:
            raise ValueError('--%s %s: only with --%s' % (name.replace('_', '-'), told[name], layer))
    if told['overlay_margin'] is not None and told['overlay'] is None and told['caption'] is None:
        raise ValueError('--overlay-margin %s: only with --overlay or --caption' % (told['overlay_margin'],))
    if told['overlay'] is None and told['caption'] is None:
        return None
    if told['caption'] is not None and (not isinstance(told['caption'], str) or not told['caption'].strip()):
        raise ValueError('--caption %r: an empty caption' % (told['caption'],))
    for name, default in (('overlay_at', 'bottom-right'), ('caption_at', 'bottom')):
        told[name] = default if told[name] is None else told[name]
        if told[name] not in ANCHORS and explicit(told[name]) is None:
            raise ValueError('--%s %s: %s, or X,Y' % (name.replace('_', '-'), told[name], ', '.join(ANCHORS)))
    try:
        share = 1.0 if told['overlay_opacity'] is None else float(told['overlay_opacity'])
    except (TypeError, ValueError):
        share = 0.0
    if not (math.isfinite(share) and 0.0 < share <= 1.0 and int(round(256 * share)) >= 1):
        raise ValueError('--overlay-opacity %s: above 0 and at most 1' % (told['overlay_opacity'],))
    told['overlay_opacity'] = int(round(256 * share))
    if told['caption_size'] is not None:
        size = _whole(told['caption_size'], 4)
        if size is None:
            raise ValueError('--caption-size %s: the font\'s size in pixels, 4 or more' % (told['caption_size'],))
        told['caption_size'] = size
    if told['overlay_margin'] is not None:
        margin = _whole(told['overlay_margin'], 0)
        if margin is None:
            raise ValueError('--overlay-margin %s: pixels, 0 or more' % (told['overlay_margin'],))
        told['overlay_margin'] = margin
    if told['overlay'] is not None and not os.path.isfile(told['overlay']):
        raise ValueError('--overlay %s: no such file' % (told['overlay'],))
    if told['font'] is not None and not os.path.isfile(told['font']):
        raise ValueError('--font %s: no such file' % (told['font'],))
    return told


def _fitted(option, name, picture, anchor, W, H, margin):
    """(x, y) of a layer's picture in a W x H frame, or ValueError: at an anchor the picture has to fit inside the frame with its margin."""
    h, w = picture.shape[:2]
    if explicit(anchor) is None and (w + 2 * margin > W or h + 2 * margin > H):
        raise ValueError('%s %s: it is %dx%d and the frames are %dx%d: with a margin of %d it does not fit inside them' % (option, name, w, h, W, H, margin))
    if w > MAX_SIDE or h > MAX_SIDE:
        raise ValueError('%s %s: it is %dx%d: at most %d either way' % (option, name, w, h, MAX_SIDE))
    x, y = place(anchor, W, H, w, h, margin)
    if not (-MAX_SIDE <= x <= MAX_SIDE and -MAX_SIDE <= y <= MAX_SIDE):
        raise ValueError('%s-at %s: %d..%d either way' % (option, anchor, -MAX_SIDE, MAX_SIDE))
    return x, y


def caption_layer(request, text, W, H, bgr=True):
    """One caption of a request as a layer of W x H frames: (picture, x, y, 256)."""
    size = request['caption_size'] if request['caption_size'] is not None else max(12, H // 18)
    margin = request['overlay_margin'] if request['overlay_margin'] is not None else max(4, W // 32)
    try:
        picture = caption_image(text, size, font=request['font'], bgr=bgr)
    except OSError as e:
        raise ValueError('--font %s: %s' % (request['font'], e)) from None
    return (picture,) + _fitted('--caption', repr(text), picture, request['caption_at'], W, H, margin) + (MAX_OPACITY,)


def overlay_layer(request, W, H, bgr=True):
    """The watermark of a request as a layer of W x H frames: (picture, x, y, opacity)."""
    margin = request['overlay_margin'] if request['overlay_margin'] is not None else max(4, W // 32)
    try:
        picture = read_rgba(request['overlay'], bgr)
    except (OSError, ValueError, SyntaxError) as e:
        raise ValueError('--overlay %s: not a picture Pillow reads (%s)' % (request['overlay'], e)) from None
    return (picture,) + _fitted('--overlay', request['overlay'], picture, request['overlay_at'], W, H, margin) + (request['overlay_opacity'],)


def layers_for(request, W, H, bgr=True):
    """The layers of a request (layers_request) for W x H frames, in the order they are applied -- the caption, then the watermark --: a list
    of (uint8 [h,w,4] picture in the frames' channel order, x, y, opacity 1..256).  The file is read and the caption drawn here, on the
    host, before any network runs; ValueError whose text begins with the option at fault."""
    if request is None:
        return []
    return ([caption_layer(request, request['caption'], W, H, bgr)] if request['caption'] is not None else []) + \
           ([overlay_layer(request, W, H, bgr)] if request['overlay'] is not None else [])


def apply_layers(frames, layers):
    """Every layer of layers_for, in its order, onto frames in HBM at a constant opacity (or, a layer's opacity a list, at one per frame): in place."""
    import torch
    for picture, x, y, opacity in layers:
        apply(frames, torch.from_numpy(picture).to(frames.device), x, y, opacity)
    return frames
