"""What tests/test_overlay_stream.py (CPU) and tests/test_overlay_gpu.py share: the NumPy twin of the overlay (include/kbe_overlay.h), written
from the formulas and not from csrc/kbe_overlay_block.h, the serial execution of that header (tests/overlay_check.cpp compiled by g++) and the
frames and pictures of the cases."""
import functools
import os
import subprocess

import numpy as np

import gif_cases as gc
import twins

# (W, H) of the frames: a row of 111 bytes, odd; one of 192 bytes, whole pieces; several rows per workgroup and rows of 480 bytes
FRAMES = [(37, 50), (64, 48), (160, 128)]
OVERLAY = (21, 9)                    # (w, h) of the cases' picture
X, Y, OPACITY = (5, 11), (7, 30), (256, 150)       # of the two frames of a case


def effective(a, opacity):
    """(a opacity + 128) >> 8 on int64."""
    return (np.asarray(a, dtype=np.int64) * np.asarray(opacity, dtype=np.int64) + 128) >> 8


def over(c, o, e):
    """(c (255 - e) + o e + 127) / 255 in integer division, on int64."""
    c, o, e = (np.asarray(v, dtype=np.int64) for v in (c, o, e))
    return (c * (255 - e) + o * e + 127) // 255


def per_frame(v, n):
    return [int(v)] * n if np.isscalar(v) else [int(k) for k in v]


def twin_over(frames, overlay, x, y, opacity=256):
    """uint8 [n,H,W,3] and uint8 [h,w,4] -> a new uint8 [n,H,W,3]: the overlay's top-left pixel at (x[i], y[i]) of frame i, clipped."""
    frames, overlay = np.asarray(frames), np.asarray(overlay)
    assert frames.dtype == overlay.dtype == np.uint8 and frames.ndim == 4 and frames.shape[3] == 3 and overlay.ndim == 3 and overlay.shape[2] == 4
    n, H, W, _ = frames.shape
    h, w, _ = overlay.shape
    x, y, opacity = per_frame(x, n), per_frame(y, n), per_frame(opacity, n)
    assert len(x) == len(y) == len(opacity) == n and all(0 <= v <= 256 for v in opacity)
    out = frames.copy()
    for i in range(n):
        x0, x1, y0, y1 = max(x[i], 0), min(x[i] + w, W), max(y[i], 0), min(y[i] + h, H)
        if x1 <= x0 or y1 <= y0:
            continue
        part = overlay[y0 - y[i]:y1 - y[i], x0 - x[i]:x1 - x[i]]
        e = effective(part[:, :, 3:], opacity[i])
        out[i, y0:y1, x0:x1] = over(frames[i, y0:y1, x0:x1], part[:, :, :3], e)
    return out


@functools.lru_cache(maxsize=None)
def frames_of(W, H, n=2, seed=21):
    """uint8 [n,H,W,3]: photo-like frames."""
    frames = np.stack([gc.photo_like(H, W, seed + i) for i in range(n)])
    frames.setflags(write=False)
    return frames


@functools.lru_cache(maxsize=None)
def overlay_of(w, h, seed=5, alpha=None):
    """uint8 [h,w,4]: photo-like colours of another seed; the alpha noise in which every eighth value is 0 and every eighth 255 (or `alpha` everywhere)."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h, w), dtype=np.uint8)
    a.reshape(-1)[::8] = 0
    a.reshape(-1)[3::8] = 255
    if alpha is not None:
        a[:] = alpha
    picture = np.dstack([gc.photo_like(h, w, 60 + seed), a])
    picture.setflags(write=False)
    return picture


@functools.lru_cache(maxsize=None)
def twin_of(W, H):
    want = twin_over(frames_of(W, H), overlay_of(*OVERLAY), X, Y, OPACITY)
    want.setflags(write=False)
    return want


# -- the header, serially -------------------------------------------------------------------
def checker():
    """tests/overlay_check.cpp, built once per process: no -ffast-math, no -march."""
    return twins.built('overlay_check')


def ask(*args):
    out = subprocess.run([checker()] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-1000:]
    return out.stdout


def _path(name):
    return os.path.join(os.path.dirname(checker()), name)


def header_over(frames, overlay, x, y, opacity=256, pad=0, overlay_pad=0):
    """The frames through over_row of csrc/kbe_overlay_block.h; pad, overlay_pad: that many bytes between the rows of the frames and of the
    overlay, so that every row lies at another alignment.  The padding comes back as it went in, or the assertion here fails."""
    frames, overlay = np.asarray(frames, dtype=np.uint8), np.asarray(overlay, dtype=np.uint8)
    n, H, W, _ = frames.shape
    h, w, _ = overlay.shape
    rows = np.full((n, H, 3 * W + pad), 0xEE, np.uint8)
    rows[:, :, :3 * W] = frames.reshape(n, H, 3 * W)
    picture = np.full((h, 4 * w + overlay_pad), 0xEE, np.uint8)
    picture[:, :4 * w] = overlay.reshape(h, 4 * w)
    with open(_path('in.raw'), 'wb') as f:
        f.write(rows.tobytes() + picture.tobytes())
    ask('over', W, H, 3 * W + pad, n, w, h, 4 * w + overlay_pad, *(','.join(str(v) for v in per_frame(t, n)) for t in (x, y, opacity)), _path('in.raw'), _path('out.raw'))
    got = np.fromfile(_path('out.raw'), np.uint8).reshape(n, H, 3 * W + pad)
    assert (got[:, :, 3 * W:] == 0xEE).all()
    return got[:, :, :3 * W].reshape(n, H, W, 3)
