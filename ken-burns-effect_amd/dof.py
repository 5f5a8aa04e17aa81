"""Depth of field: raw frames that lie in HBM, blurred on the GPU by the depth of every one of their pixels (include/kbe_dof.h: kbe_dof_u8; the
arithmetic is defined in csrc/kbe_dof_block.h).  common.render_frames(lens=...) uses it to throw what is not at the focus depth out of
focus, and to pull the focus from one subject to another while the camera moves.

A pixel of depth z gets the radius min(max_radius, round(aperture |z - focus| / z)) -- the aperture is the radius, in pixels of the raw frame,
of a point at infinity --, and every target pixel gathers the samples whose disc reaches it: a sample in front of the target spreads by its
own radius, a sample behind it by no more than the target's own, so a sharp foreground keeps its edge against a blurred background and a
blurred foreground spills over a sharp background.  One layer, a box disc: DESIGN.md section 5 lists what that leaves out.

This is the only module that names the entries of kbe_dof.h: they are exported by libkbe_hip.so beside those of the other headers and typed
from their own header on the package's one handle of that library, the way crop_area.py types its own.  No fallback: without the HIP library
every call here raises.
"""
import collections
import ctypes
import math
import os

from . import _cabi, _native

HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'kbe_dof.h')
ABI_VERSION = 1
MAX_RADIUS = 16
FRAMES_PER_GROUP = 12              # the route renders, blurs and finishes that many frames at a time: one launch of the entry
HEADER = _cabi.Header(HEADER_PATH, 'KBE_DOF_API', 'include/kbe_dof.h', abi=('kbe_dof_abi_version', ABI_VERSION, 'depth-of-field '))
prototypes = HEADER.prototypes     # {entry: (restype, [argtypes])} of every entry include/kbe_dof.h declares, in its order, read once

# focus_from, focus_to: the focus depth of the first and of the last frame (the cloud's depth attribute, as tensorRawDepth holds it), the
# frames between them by focus_path; aperture: pixels, finite, >= 0; max_radius: 0..16
Lens = collections.namedtuple('Lens', 'focus_from focus_to aperture max_radius', defaults=(MAX_RADIUS,))


def load():
    """The package's one handle of libkbe_hip.so (_native.load), its depth-of-field entries typed from include/kbe_dof.h the first time it is seen."""
    return HEADER.bind(_native.load())


def _raw(name, *args):
    """The entry `name` of include/kbe_dof.h with plain Python values -> what it returns; a surplus argument, which cdecl lets through, is refused."""
    return HEADER.raw(load(), name, *args)


def _call(name, *args):
    """An entry that returns a status: KbeError with the library's text unless KBE_OK."""
    HEADER.call(load(), name, *args)


def checked_lens(lens):
    """The lens as the entry will take it, or ValueError: finite focus depths > 0, a finite aperture >= 0, max_radius 0..16."""
    lens = Lens(*lens)
    for name in ('focus_from', 'focus_to'):
        z = float(getattr(lens, name))
        if not (math.isfinite(z) and z > 0.0):
            raise ValueError('lens: %s = %r: a focus depth is a finite number above 0' % (name, getattr(lens, name)))
    if not (math.isfinite(float(lens.aperture)) and float(lens.aperture) >= 0.0):
        raise ValueError('lens: aperture = %r: a finite number of pixels, 0 or more' % (lens.aperture,))
    if not (int(lens.max_radius) == lens.max_radius and 0 <= int(lens.max_radius) <= MAX_RADIUS):
        raise ValueError('lens: max_radius = %r: 0..%d' % (lens.max_radius, MAX_RADIUS))
    return Lens(float(lens.focus_from), float(lens.focus_to), float(lens.aperture), int(lens.max_radius))


def focus_path(z0, z1, steps):
    """`steps` focus depths from z0 to z1, linear in 1 / z -- in disparity, as a lens is pulled; the endpoints are z0 and z1 themselves."""
    z0, z1, steps = float(z0), float(z1), int(steps)
    if not (math.isfinite(z0) and math.isfinite(z1) and z0 > 0.0 and z1 > 0.0 and steps >= 1):
        raise ValueError('focus_path(%r, %r, %r): two finite depths above 0 and 1 or more steps' % (z0, z1, steps))
    if steps == 1:
        return [z0]
    path = [1.0 / (1.0 / z0 + (1.0 / z1 - 1.0 / z0) * (i / (steps - 1))) for i in range(steps)]
    path[0], path[-1] = z0, z1
    return path


def focus_depth(raw_depth, u, v):
    """The depth to focus on at pixel (u, v) of the photo: the median of the 5 x 5 depths of ``raw_depth`` [1,1,H,W] around the rounded pixel,
    the window clamped to the image (25 values in a corner as well: border pixels count more than once)."""
    import torch
    H, W = int(raw_depth.shape[-2]), int(raw_depth.shape[-1])
    x, y = int(math.floor(float(u) + 0.5)), int(math.floor(float(v) + 0.5))
    xs = torch.tensor([min(max(x + d, 0), W - 1) for d in range(-2, 3)], device=raw_depth.device)
    ys = torch.tensor([min(max(y + d, 0), H - 1) for d in range(-2, 3)], device=raw_depth.device)
    window = raw_depth.reshape(H, W).index_select(0, ys).index_select(1, xs).reshape(-1).float()
    return float(window.sort().values[12].item())


def apply(frames_in_hbm, depth_in_hbm, focus, aperture, max_radius=MAX_RADIUS):
    """uint8 [n,H,W,3] raw frames and float32 [n,H,W] depths in HBM, n focus depths, the aperture in pixels and the cap of the radius ->
    a new uint8 [n,H,W,3] tensor on the same device (kbe_dof_u8).  Asynchronous on the current stream."""
    import torch
    n, H, W, _, sources = _native.frame_pointers(frames_in_hbm, 'dof.apply')
    if not (torch.is_tensor(depth_in_hbm) and depth_in_hbm.dtype == torch.float32 and tuple(depth_in_hbm.shape) == (n, H, W)):
        raise _native.KbeError('dof.apply takes a float32 [n,H,W] tensor of depths on the GPU beside its %d frames of %dx%d' % (n, W, H))
    focus = [float(z) for z in focus]
    if len(focus) != n:
        raise _native.KbeError('dof.apply: %d focus depths for %d frames' % (len(focus), n))
    # (every plane contiguous; the planes themselves any distance apart: plane 3 of n float renders [n,4,H,W] is taken where it lies)
    if not (depth_in_hbm.device == frames_in_hbm.device and (W == 1 or depth_in_hbm.stride(2) == 1) and (H == 1 or depth_in_hbm.stride(1) == W)):
        raise _native.KbeError('dof.apply: the depths lie on %s, their planes strided %s: contiguous [H,W] planes on the frames\' device' % (depth_in_hbm.device, tuple(depth_in_hbm.stride())))
    planes = (ctypes.c_void_p * n)(*[depth_in_hbm.data_ptr() + 4 * i * depth_in_hbm.stride(0) for i in range(n)])
    out = torch.empty((n, H, W, 3), dtype=torch.uint8, device=frames_in_hbm.device)
    targets = _native.frame_pointers(out, 'dof.apply')[4]
    _call('kbe_dof_u8', sources, planes, n, W, H, 3 * W, W, (ctypes.c_double * n)(*focus), float(aperture), int(max_radius), targets, 3 * W, _native._stream())
    return out
