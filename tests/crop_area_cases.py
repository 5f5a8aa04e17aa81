"""What tests/test_crop_area_stream.py (CPU) and tests/test_crop_area_gpu.py share: the NumPy twin of the crop + exact area-average reduction
(include/kbe_crop_area.h; defined in csrc/kbe_crop_area_block.h), the serial execution of that header (tests/crop_area_check.cpp compiled by
g++) and the frames of the cases."""
import functools
import os
import subprocess

import numpy as np

import area_cases as ac
import gif_cases as gc
import twins


# -- the NumPy twin -------------------------------------------------------------------------
def start(N, n):
    """(floor(c), whether c lies half a pixel beyond it) of c = N / 2 - (n - 1) / 2, in integers."""
    assert 1 <= n <= N
    return (N - n + 1) // 2, (N - n) % 2 == 0


def twin_patch(frames, cw, ch):
    """uint8 [..., H, W, 3] -> uint8 [..., ch, cw, 3]: the centred patch by integer slicing and shifts -- the raw rectangle, (a + b + 1) >> 1
    of two neighbours along an axis that starts on a half pixel, (a + b + c + d + 2) >> 2 where both do; the border pixel is repeated."""
    a = np.asarray(frames)
    assert a.dtype == np.uint8 and a.shape[-1] == 3
    H, W = a.shape[-3], a.shape[-2]
    (ipx, hx), (ipy, hy) = start(W, cw), start(H, ch)
    a = a.astype(np.int64)
    if hx or hy:
        a = np.concatenate([a, a[..., -1:, :, :]], axis=-3)          # (a tap beyond the frame: only where the crop is the frame's side)
        a = np.concatenate([a, a[..., :, -1:, :]], axis=-2)
    p = a[..., ipy:ipy + ch, ipx:ipx + cw, :]
    if hx and hy:
        p = (p + a[..., ipy:ipy + ch, ipx + 1:ipx + cw + 1, :] + a[..., ipy + 1:ipy + ch + 1, ipx:ipx + cw, :] + a[..., ipy + 1:ipy + ch + 1, ipx + 1:ipx + cw + 1, :] + 2) >> 2
    elif hx:
        p = (p + a[..., ipy:ipy + ch, ipx + 1:ipx + cw + 1, :] + 1) >> 1
    elif hy:
        p = (p + a[..., ipy + 1:ipy + ch + 1, ipx:ipx + cw, :] + 1) >> 1
    return p.astype(np.uint8)


def twin_reduce(frames, crop, size):
    """uint8 [..., H, W, 3] -> uint8 [..., h, w, 3]: the patch, then area_cases' reduction of it."""
    return ac.twin_reduce(twin_patch(frames, *crop), *size)


# -- the header, serially -------------------------------------------------------------------
def checker():
    """tests/crop_area_check.cpp, built once per process: no -ffast-math, no -march."""
    return twins.built('crop_area_check')


def ask(*args):
    out = subprocess.run([checker()] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-1000:]
    return out.stdout


def header_reduce(frames, crop, size=None, pad=0):
    """The same frames through crop_reduce_pixel of csrc/kbe_crop_area_block.h, or with size=None through its Patch alone (no area arithmetic);
    ``pad``: that many bytes between the rows."""
    frames = np.asarray(frames, dtype=np.uint8)
    n, H, W, _ = frames.shape
    rows = np.full((n, H, 3 * W + pad), 0xEE, np.uint8)
    rows[:, :, :3 * W] = frames.reshape(n, H, 3 * W)
    src, dst = (os.path.join(os.path.dirname(checker()), name) for name in ('in.raw', 'out.raw'))
    rows.tofile(src)
    if size is None:
        ask('patch', W, H, 3 * W + pad, crop[0], crop[1], n, src, dst)
        return np.fromfile(dst, np.uint8).reshape(n, crop[1], crop[0], 3)
    ask('reduce', W, H, 3 * W + pad, crop[0], crop[1], size[0], size[1], n, src, dst)
    return np.fromfile(dst, np.uint8).reshape(n, size[1], size[0], 3)


# -- the cases ------------------------------------------------------------------------------
# (W, H) of the frames: narrower than a tile and odd; one tile across; several tiles on both axes
FRAMES = [(37, 50), (64, 48), (160, 128)]
# crops by what they take off the frame's sides: (W - cw, H - ch) of all four parities -- 'oo' starts on whole pixels on both axes, 'ee' on
# half pixels on both --, and the frame's own sides, where the last taps repeat the border pixel
OFF = {'oo': (5, 3), 'oe': (5, 4), 'eo': (4, 3), 'ee': (4, 6), 'full_w': (0, 3), 'full_h': (5, 0), 'full': (0, 0)}


def crop_of(frame, name):
    return frame[0] - OFF[name][0], frame[1] - OFF[name][1]


def targets(crop):
    """{name: (w, h)}: one pixel, the patch itself, just under a factor of 2 (most targets straddle three sources), 7-fold."""
    cw, ch = crop
    return {'one_pixel': (1, 1), 'patch': (cw, ch), 'under_2': (cw // 2 + 1, ch // 2 + 1), 'sevenfold': (max(1, cw // 7), max(1, ch // 7))}


@functools.lru_cache(maxsize=None)
def frames(W, H, n=2):
    """n photo-like frames [H, W, 3]."""
    out = np.stack([gc.photo_like(H, W, 5 + i) for i in range(n)])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def wide():
    """A 700 x 20 frame: its crop 690 x 19 is wider than a strip of the kernel's LDS (339 patch pixels) and taller than a strip's 16 rows."""
    import encoder_gpu as eg
    frame = np.ascontiguousarray(eg.tiled(20, 700, 13)[None])
    assert frame.shape == (1, 20, 700, 3)
    frame.setflags(write=False)
    return frame


@functools.lru_cache(maxsize=None)
def twin_of(W, H, crop, size, n=2):
    want = twin_reduce(frames(W, H, n), crop, size)
    want.setflags(write=False)
    return want
