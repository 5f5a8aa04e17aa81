"""What tests/test_dof_stream.py (CPU) and tests/test_dof_gpu.py share: the NumPy twin of the depth-of-field blur (include/kbe_dof.h; defined in
csrc/kbe_dof_block.h), the serial execution of that header (tests/dof_check.cpp compiled by g++) and the frames and depth planes of the cases."""
import functools
import os
import subprocess

import numpy as np

import gif_cases as gc
import twins

MAX_RADIUS = 16
DISC = [1, 5, 13, 29, 49, 81, 113, 149, 197, 253, 317, 377, 441, 529, 613, 709, 797]       # n(e), as the issue lists it


# -- the NumPy twin -------------------------------------------------------------------------
def disc_points(e):
    d = np.arange(-e, e + 1)
    return int((d[:, None] ** 2 + d[None, :] ** 2 <= e * e).sum())


WEIGHT = np.array([8192 // disc_points(e) for e in range(MAX_RADIUS + 1)], np.int64)


def twin_radius(z, zf, A, R):
    """float32 depths of any shape -> int64 radii 0..R: the compare loop in float32, every operation one rounding; a depth that is not
    finite or not > 0 gives 0."""
    z, zf, A = np.asarray(z, np.float32), np.float32(zf), np.float32(A)
    assert 0 <= R <= MAX_RADIUS
    with np.errstate(all='ignore'):
        lhs = A * np.abs(z - zf)
        assert lhs.dtype == np.float32
        r = np.zeros(z.shape, np.int64)
        for j in range(1, R + 1):
            r += lhs >= np.float32(j - 0.5) * z
        return np.where(np.isfinite(z) & (z > 0), r, 0)


def twin_blur(frames, depth, focus, A, R):
    """uint8 [n,H,W,3], float32 [n,H,W], n focus depths, the aperture, the cap -> uint8 [n,H,W,3]: a loop over the (2R+1)^2 offsets on
    whole arrays in int64."""
    frames, depth = np.asarray(frames), np.asarray(depth, np.float32)
    assert frames.dtype == np.uint8 and frames.shape[-1] == 3 and depth.shape == frames.shape[:-1] and len(focus) == len(frames)
    n, H, W, _ = frames.shape
    out = np.empty_like(frames)
    for i in range(n):
        rp, zp = twin_radius(depth[i], focus[i], A, R), depth[i]
        r = np.pad(rp, R)                                         # (outside the frame: radius 0 -- and masked out below all the same)
        z = np.pad(zp, R)
        v = np.pad(frames[i].astype(np.int64), ((R, R), (R, R), (0, 0)))
        inside = np.pad(np.ones((H, W), bool), R)
        sw, swv = np.zeros((H, W), np.int64), np.zeros((H, W, 3), np.int64)
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                window = (slice(R + dy, R + dy + H), slice(R + dx, R + dx + W))
                rq, zq = r[window], z[window]
                with np.errstate(invalid='ignore'):
                    e = np.where(zq <= zp, rq, np.minimum(rq, rp))
                w = np.where(inside[window] & (dx * dx + dy * dy <= e * e), WEIGHT[e], 0)
                sw += w
                swv += w[:, :, None] * v[window]
        assert (sw >= WEIGHT[rp]).all() and swv.max() < 2 ** 31
        out[i] = ((2 * swv + sw[:, :, None]) // (2 * sw[:, :, None])).astype(np.uint8)
    return out


# -- the header, serially -------------------------------------------------------------------
def checker():
    """tests/dof_check.cpp, built once per process: no -ffast-math, no -march."""
    return twins.built('dof_check')


def ask(*args):
    out = subprocess.run([checker()] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-1000:]
    return out.stdout


def _text(value):
    """Decimal text that strtof reads back as exactly this float32."""
    return '%.9g' % float(np.float32(value))


def _path(name):
    return os.path.join(os.path.dirname(checker()), name)


def header_radius(z, zf, A, R):
    z = np.ascontiguousarray(z, np.float32).reshape(-1)
    z.tofile(_path('z.f32'))
    ask('radius', _text(zf), _text(A), R, z.size, _path('z.f32'), _path('r.u8'))
    return np.fromfile(_path('r.u8'), np.uint8).astype(np.int64)


def header_blur(frames, depth, focus, A, R, pad=0, z_pad=0):
    """The same frames through gather_pixel of csrc/kbe_dof_block.h; ``pad``: that many bytes between the rows, ``z_pad``: floats."""
    frames, depth = np.asarray(frames, dtype=np.uint8), np.asarray(depth, np.float32)
    n, H, W, _ = frames.shape
    rows = np.full((n, H, 3 * W + pad), 0xEE, np.uint8)
    rows[:, :, :3 * W] = frames.reshape(n, H, 3 * W)
    planes = np.full((n, H, W + z_pad), -1.0, np.float32)
    planes[:, :, :W] = depth
    rows.tofile(_path('in.raw'))
    planes.tofile(_path('depth.f32'))
    np.asarray(focus, np.float32).tofile(_path('focus.f32'))
    ask('blur', W, H, 3 * W + pad, W + z_pad, R, _text(A), n, _path('in.raw'), _path('depth.f32'), _path('focus.f32'), _path('out.raw'))
    return np.fromfile(_path('out.raw'), np.uint8).reshape(n, H, W, 3)


# -- the cases ------------------------------------------------------------------------------
# (W, H) of the frames: narrower than a tile and odd; one tile across; several tiles on both axes
FRAMES = [(37, 50), (64, 48), (160, 128)]
RADII = [0, 1, 5, 16]
APERTURE = 20.0
FOCUS = (120.0, 300.0, 90.0, 640.0)          # of frames 0, 1, 2, 3, and round again: the two frames of a case differ


def focus_of(n):
    return [FOCUS[i % len(FOCUS)] for i in range(n)]


@functools.lru_cache(maxsize=None)
def frames(W, H, n=2):
    """n photo-like frames [H, W, 3]."""
    out = np.stack([gc.photo_like(H, W, 5 + i) for i in range(n)])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def depths(W, H, n=2):
    """n depth planes [H, W] of normal fp32 numbers: a background that recedes from 200 to 800 across the frame, a ripple on it, an ellipse at
    120 and, in front of both, a slanted bar from 60 to 90 -- so that at APERTURE and FOCUS every radius from 0 to 16 occurs and sharp and
    blurred regions meet both ways round."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = []
    for i in range(n):
        z = 200.0 + 600.0 * ((x + i) % W) / max(W - 1, 1) + 15.0 * np.sin(0.37 * y + i)
        z = np.where(((x - 0.6 * W) / (0.25 * W)) ** 2 + ((y - 0.45 * H) / (0.3 * H)) ** 2 <= 1.0, 120.0, z)
        bar = np.abs(y - (0.75 * H - 0.2 * x)) <= max(2.0, 0.06 * H)
        z = np.where(bar, 60.0 + 30.0 * x / max(W - 1, 1), z)
        out.append(z.astype(np.float32))
    out = np.stack(out)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def twin_of(W, H, R, n=2):
    want = twin_blur(frames(W, H, n), depths(W, H, n), focus_of(n), APERTURE, R)
    want.setflags(write=False)
    return want


def marked(W, H, where, near=50.0, far=100.0):
    """A [H, W] depth plane at `far` with the pixels `where` ((x, y) pairs) at `near`: with the focus at `far` only those are blurred."""
    z = np.full((H, W), far, np.float32)
    for x, y in where:
        z[y, x] = near
    return z
