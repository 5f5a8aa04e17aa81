"""Output sharpening: an exact integer unsharp mask applied on the GPU to frames that lie in HBM (include/kbe_sharpen.h: kbe_sharpen_u8; the
arithmetic is defined in csrc/kbe_sharpen_block.h), and what the products need of it: the taps of a sigma (taps_for), the option of kbe.py,
Pipeline and slideshow.py read and checked (request), and the frames of a clip sharpened where they lie (apply_sharpen).

The frame is blurred by a separable Gaussian, the border pixel repeated, and the difference to the blur is added back:
out = v + amount (v - blur) wherever |v - blur| is at least the threshold, all in integers -- the blur in 8.8 fixed point, the taps 16-bit
values that add up to 32768, the gain in 1/256.  The host makes the taps in float64 from the sigma; the device never sees the sigma.

This is the only module that names the entries of kbe_sharpen.h: they are exported by libkbe_hip.so beside those of the other headers and
typed from their own header on the package's one handle of that library.  No fallback: without the HIP library every call here raises.
"""
import ctypes
import math
import os

from . import _cabi, _native

HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'kbe_sharpen.h')
ABI_VERSION = 1
FRAMES_PER_LAUNCH = 12             # the entry cuts a call's frames into launches of this many; apply_sharpen's groups are as long
MAX_SIDE = 65535
MAX_RADIUS = 24                    # csrc/kbe_sharpen_block.h, kMaxRadius
ONE = 32768                        # what the taps add up to: w[0] + 2 (w[1] + .. + w[R])
MAX_AMOUNT = 1024                  # the gain in 1/256: AMOUNT is above 0 and at most 4
MIN_SIGMA, MAX_SIGMA = 0.3, 8.0
HEADER = _cabi.Header(HEADER_PATH, 'KBE_SHARPEN_API', 'include/kbe_sharpen.h', abi=('kbe_sharpen_abi_version', ABI_VERSION, 'sharpen '))
prototypes = HEADER.prototypes     # {entry: (restype, [argtypes])} of every entry include/kbe_sharpen.h declares, in its order, read once


def load():
    """The package's one handle of libkbe_hip.so (_native.load), its sharpen entries typed from include/kbe_sharpen.h the first time it is seen."""
    return HEADER.bind(_native.load())


def _raw(name, *args):
    """The entry `name` of include/kbe_sharpen.h with plain Python values -> what it returns; a surplus argument, which cdecl lets through, is refused."""
    return HEADER.raw(load(), name, *args)


def _call(name, *args):
    """An entry that returns a status: KbeError with the library's text unless KBE_OK."""
    HEADER.call(load(), name, *args)


def taps_for(sigma):
    """The taps (w[0], .., w[R]) of a Gaussian of `sigma`, 0.3..8, in float64: R = min(24, max(1, ceil(3 sigma))), g_k = exp(-k^2 / (2 sigma^2)),
    G = g_0 + 2 (g_1 + .. + g_R), w_k = floor(32768 g_k / G + 0.5) for k >= 1 and w_0 by difference: they add up to 32768 exactly."""
    sigma = float(sigma)
    if not MIN_SIGMA <= sigma <= MAX_SIGMA:
        raise ValueError('sharpen.taps_for: sigma = %r: %g..%g' % (sigma, MIN_SIGMA, MAX_SIGMA))
    R = min(MAX_RADIUS, max(1, math.ceil(3.0 * sigma)))
    g = [math.exp(-k * k / (2.0 * sigma * sigma)) for k in range(R + 1)]
    G = g[0] + 2.0 * sum(g[1:])
    w = [int(math.floor(ONE * g[k] / G + 0.5)) for k in range(1, R + 1)]
    return (ONE - 2 * sum(w),) + tuple(w)


def request(value=None, environment=True):
    """What the products were told of the sharpening -- kbe.py's --sharpen AMOUNT[,SIGMA[,THRESHOLD]], Pipeline(sharpen=) as such a text, a
    number or a tuple, else (environment) KBE_SHARPEN -- read and checked on the host, before any network runs: None without it, else
    {'amount': 1..1024, the gain in 1/256, 'sigma', 'threshold': 0..255, 'taps': taps_for(sigma), 'radius'}.  AMOUNT is above 0 and at most
    4 and is rounded to 1/256; SIGMA is 0.3..8, default 1; THRESHOLD a whole number 0..255, default 0.  ValueError whose text begins with
    the option and the value."""
    if value is None and environment:
        value = os.environ.get('KBE_SHARPEN') or None
    if value is None:
        return None
    shown = value if isinstance(value, str) else ','.join('%s' % (v,) for v in value) if isinstance(value, (tuple, list)) else '%s' % (value,)
    if isinstance(value, str):
        fields = [part.strip() for part in value.split(',')]
    elif isinstance(value, (tuple, list)):
        fields = list(value)
    else:
        fields = [value]
    if len(fields) > 3:
        raise ValueError('--sharpen %s: %d fields: AMOUNT[,SIGMA[,THRESHOLD]], three at most' % (shown, len(fields)))

    def number(field):
        if isinstance(field, bool) or field is None or field == '':
            return math.nan
        try:
            return float(field)
        except (TypeError, ValueError):
            return math.nan
    amount, sigma = number(fields[0]), number(fields[1]) if len(fields) > 1 else 1.0
    level = fields[2] if len(fields) > 2 else 0
    if isinstance(level, str):
        level = int(level) if level.lstrip('-').isdigit() and level.count('-') <= 1 else None
    elif isinstance(level, bool) or not isinstance(level, int):
        level = None
    if math.isnan(amount) or math.isnan(sigma) or level is None:
        raise ValueError('--sharpen %s: AMOUNT[,SIGMA[,THRESHOLD]]: two numbers and a whole number' % shown)
    gain = int(math.floor(256.0 * amount + 0.5)) if math.isfinite(amount) else 0
    if not (0.0 < amount <= 4.0 and gain >= 1):
        raise ValueError('--sharpen %s: AMOUNT %s: above 0 and at most 4' % (shown, fields[0]))
    if not MIN_SIGMA <= sigma <= MAX_SIGMA:
        raise ValueError('--sharpen %s: SIGMA %s: %g..%g' % (shown, fields[1], MIN_SIGMA, MAX_SIGMA))
    if not 0 <= level <= 255:
        raise ValueError('--sharpen %s: THRESHOLD %s: a whole number 0..255' % (shown, fields[2]))
    taps = taps_for(sigma)
    return {'amount': gain, 'sigma': sigma, 'threshold': level, 'taps': taps, 'radius': len(taps) - 1}


def apply_sharpen(frames, request):
    """frames: a contiguous uint8 [n,H,W,3] tensor in HBM; request: request()'s answer.  The frames are sharpened in place from the caller's
    view and returned: groups of at most 12 frames go through kbe_sharpen_u8 into ONE scratch tensor the size of a group and are copied back
    on the device, all on the current stream -- a 4K clip does not need a second copy of itself.  Asynchronous."""
    import torch
    what = 'sharpen.apply_sharpen'
    if not (torch.is_tensor(frames) and frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() == 4 and frames.size(3) == 3 and frames.size(0) >= 1 and frames.is_contiguous()):
        raise _native.KbeError('%s takes a contiguous uint8 [n,H,W,3] tensor on the GPU' % what)
    n, H, W, step, pointers = _native.frame_pointers(frames, what)
    if not (1 <= W <= MAX_SIDE and 1 <= H <= MAX_SIDE):
        raise _native.KbeError('%s: frames of %d x %d: 1..%d either way' % (what, W, H, MAX_SIDE))
    taps, radius = request['taps'], request['radius']
    scratch = torch.empty((min(n, FRAMES_PER_LAUNCH), H, W, 3), dtype=torch.uint8, device=frames.device)
    targets = _native.frame_pointers(scratch, what)[4]
    for first in range(0, n, FRAMES_PER_LAUNCH):
        count = min(FRAMES_PER_LAUNCH, n - first)
        sources = (ctypes.c_void_p * count)(*pointers[first:first + count])
        _call('kbe_sharpen_u8', sources, count, W, H, 3 * W, targets, 3 * W, (ctypes.c_uint16 * (radius + 1))(*taps), radius, request['amount'], request['threshold'], _native._stream())
        frames[first:first + count].copy_(scratch[:count])
    return frames
