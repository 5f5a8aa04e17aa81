"""Motion blur: every frame of a clip the mean of frames rendered at sub-frame cameras while the shutter is open, taken on the GPU from frames
that lie in HBM (include/kbe_shutter.h: kbe_shutter_mean_u8; the arithmetic is defined in csrc/kbe_shutter_block.h).
common.render_frames(shutter=...) uses it: time is supersampled, nothing is smeared along a guessed vector.

A shutter is open for `fraction` of a frame interval, centred on the frame's own step of the camera path, and is sampled at `samples` points:
the midpoints of that many equal parts of the open interval (offsets).  sample_steps places them ON the path, between the frame's step and
its neighbours', and folds the exposure back at the path's two ends -- the clip plays forth and back and the GIF loops for ever, so that is
what a camera on this path exposes; no camera leaves the path.  The mean is exact and byte-defined: (2 sum + S) / (2 S) in integers.

This is the only module that names the entries of kbe_shutter.h: they are exported by libkbe_hip.so beside those of the other headers and
typed from their own header on the package's one handle of that library, the way dof.py types its own.  No fallback: without the HIP library
every call here raises.
"""
import collections
import ctypes
import math
import os

from . import _cabi, _native

HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'kbe_shutter.h')
ABI_VERSION = 1
MAX_SAMPLES = 32
HEADER = _cabi.Header(HEADER_PATH, 'KBE_SHUTTER_API', 'include/kbe_shutter.h', abi=('kbe_shutter_abi_version', ABI_VERSION, 'shutter '))
prototypes = HEADER.prototypes     # {entry: (restype, [argtypes])} of every entry include/kbe_shutter.h declares, in its order, read once

# fraction: the share of a frame interval the shutter is open, finite, 0..1; samples: the sub-frame cameras of every frame, 1..32
Shutter = collections.namedtuple('Shutter', 'fraction samples', defaults=(8,))


def load():
    """The package's one handle of libkbe_hip.so (_native.load), its shutter entries typed from include/kbe_shutter.h the first time it is seen."""
    return HEADER.bind(_native.load())


def _raw(name, *args):
    """The entry `name` of include/kbe_shutter.h with plain Python values -> what it returns; a surplus argument, which cdecl lets through, is refused."""
    return HEADER.raw(load(), name, *args)


def _call(name, *args):
    """An entry that returns a status: KbeError with the library's text unless KBE_OK."""
    HEADER.call(load(), name, *args)


def checked(shutter):
    """The shutter as the route will take it, or ValueError: a finite fraction 0..1, an integer number of samples 1..32."""
    try:
        shutter = Shutter(*shutter)
        fraction = float(shutter.fraction)
        samples = int(shutter.samples) if int(shutter.samples) == shutter.samples and not isinstance(shutter.samples, bool) else 0
    except (TypeError, ValueError, OverflowError):
        raise ValueError('shutter: %r: (fraction, samples), a finite fraction 0..1 and 1..%d samples' % (shutter, MAX_SAMPLES)) from None
    if not (math.isfinite(fraction) and 0.0 <= fraction <= 1.0):
        raise ValueError('shutter: fraction = %r: the share of a frame interval the shutter is open, a finite number 0..1' % (shutter.fraction,))
    if not 1 <= samples <= MAX_SAMPLES:
        raise ValueError('shutter: samples = %r: 1..%d' % (shutter.samples, MAX_SAMPLES))
    return Shutter(fraction, samples)


def offsets(samples):
    """The midpoints of `samples` equal parts of [-1/2, 1/2]; the middle one of an odd number is 0."""
    S = int(samples)
    return [(2 * k + 1 - S) / (2 * S) for k in range(S)]


def sample_steps(steps, fraction, samples):
    """The steps of the camera path at which the frames of `steps` are sampled: len(steps) * samples of them, those of frame i at
    i * samples ...  For the frame at step t and the offset o the sample is t + |o| fraction (neighbour - t), the neighbour the next step for
    o > 0 and the previous one for o < 0; the first frame's previous step is its next one and the last frame's next step its previous one
    (the exposure folded back at the path's ends); a single step has all its samples on itself.  Any list of steps, not only uniform ones."""
    fraction, samples = checked((fraction, samples))
    steps = [float(t) for t in steps]
    n = len(steps)
    out = []
    for i, t in enumerate(steps):
        before = steps[i - 1] if i > 0 else steps[min(1, n - 1)]
        after = steps[i + 1] if i + 1 < n else steps[max(n - 2, 0)]
        for o in offsets(samples):
            out.append(t + abs(o) * fraction * ((after if o > 0 else before) - t) if o != 0 else t)
    return out


def mean(frames_in_hbm, samples):
    """uint8 [n * samples,H,W,3] frames in HBM, the samples of output i at i * samples ... -> a new uint8 [n,H,W,3] tensor on the same device,
    every frame the mean of its samples, rounded half up.  Asynchronous on the current stream."""
    import torch
    f = frames_in_hbm
    if not (torch.is_tensor(f) and f.is_cuda and f.dtype == torch.uint8 and f.dim() == 4 and f.size(3) == 3 and f.size(0) >= 1 and f.is_contiguous()):
        raise _native.KbeError('shutter.mean takes a contiguous uint8 [n * samples,H,W,3] tensor on the GPU (got %s)' % (
            '%s %s on %s' % (tuple(f.shape), f.dtype, f.device) if torch.is_tensor(f) else type(f).__name__))
    total, H, W, _, sources = _native.frame_pointers(f, 'shutter.mean')
    if not (isinstance(samples, int) and not isinstance(samples, bool) and 1 <= samples <= MAX_SAMPLES):
        raise _native.KbeError('shutter.mean: samples = %r: 1..%d' % (samples, MAX_SAMPLES))
    if total % samples:
        raise _native.KbeError('shutter.mean: %d frames are no whole number of groups of %d samples' % (total, samples))
    n = total // samples
    out = torch.empty((n, H, W, 3), dtype=torch.uint8, device=frames_in_hbm.device)
    targets = _native.frame_pointers(out, 'shutter.mean')[4]
    _call('kbe_shutter_mean_u8', sources, n, samples, W, H, 3 * W, targets, 3 * W, _native._stream())
    return out
