"""What tests/test_enlarge_stream.py (CPU) and tests/test_enlarge_gpu.py share: the NumPy twin of the crop + exact bicubic enlargement
(include/kbe_enlarge.h; defined in csrc/kbe_enlarge_block.h) -- its coefficients in Python integers, so independent of the header's int64 --,
the serial execution of that header (tests/enlarge_check.cpp compiled by g++ under its sanitizers) and the cases.  The frames, the crops and
the patch are tests/crop_area_cases.py's."""
import functools
import os
import subprocess

import numpy as np

import crop_area_cases as cc
import twins

ONE, MAX_SIDE = 16384, 16384
FRAMES, OFF, crop_of, wide = cc.FRAMES, cc.OFF, cc.crop_of, cc.wide


# -- the NumPy twin -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def axis(n_in, n_out):
    """(int64 [n_out, 4] coefficients, int64 [n_out, 4] clamped taps) of an axis, in Python integers of any size."""
    assert 1 <= n_in <= n_out
    D = 2 * n_out
    c, t = np.empty((n_out, 4), np.int64), np.empty((n_out, 4), np.int64)
    for x in range(n_out):
        p = (2 * x + 1) * n_in - n_out
        i = p // D                                                       # (Python's // is a floor)
        r = p - i * D
        n0, n2, n3 = -r ** 3 + 2 * r * r * D - r * D * D, -3 * r ** 3 + 4 * r * r * D + r * D * D, r ** 3 - r * r * D
        c0, c2, c3 = ((n * ONE + D ** 3) // (2 * D ** 3) for n in (n0, n2, n3))
        c[x] = (c0, ONE - c0 - c2 - c3, c2, c3)
        t[x] = [min(max(i - 1 + k, 0), n_in - 1) for k in range(4)]
    c.setflags(write=False)
    t.setflags(write=False)
    return c, t


def _pass(values, n_out, along, counts):
    """One pass along axis `along` (-3: down the columns, -2: along the rows) of int64 [..., h, w, 3] bytes -> the same with n_out there."""
    c, t = axis(values.shape[along], n_out)
    shape = [1, 1, 1]
    shape[along] = n_out
    total = sum(c[:, k].reshape(shape) * np.take(values, t[:, k], axis=along) for k in range(4))
    total = (total + ONE // 2) >> 14
    if counts is not None:
        counts.append((int((total < 0).sum()), int((total > 255).sum())))
    return np.clip(total, 0, 255)


def twin_resample(patch, size, counts=None):
    """uint8 [..., ch, cw, 3] -> uint8 [..., h, w, 3]: the pass along the rows to bytes, then the pass down the columns.
    counts: a list that takes (sums below 0, sums above 255) of the two passes, in their order."""
    patch = np.asarray(patch)
    assert patch.dtype == np.uint8 and patch.shape[-1] == 3
    return _pass(_pass(patch.astype(np.int64), size[0], -2, counts), size[1], -3, counts).astype(np.uint8)


def twin_enlarge(frames, crop, size, counts=None):
    """uint8 [..., H, W, 3] -> uint8 [..., h, w, 3]: the patch (crop_area_cases.twin_patch), resampled."""
    return twin_resample(cc.twin_patch(frames, *crop), size, counts)


# -- the header, serially -------------------------------------------------------------------
def checker():
    """tests/enlarge_check.cpp, built once per process under UBSan's signed-integer-overflow check and AddressSanitizer: a plain program."""
    return twins.built('enlarge_check', '-fsanitize=signed-integer-overflow,address', '-fno-sanitize-recover=all')


def ask(*args):
    out = subprocess.run([checker()] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
    return out.stdout


def header_enlarge(frames, crop, size, pad=0):
    """The same frames through enlarge_pixel of csrc/kbe_enlarge_block.h; ``pad``: that many bytes between the rows."""
    frames = np.asarray(frames, dtype=np.uint8)
    n, H, W, _ = frames.shape
    rows = np.full((n, H, 3 * W + pad), 0xEE, np.uint8)
    rows[:, :, :3 * W] = frames.reshape(n, H, 3 * W)
    src, dst = (os.path.join(os.path.dirname(checker()), name) for name in ('in.raw', 'out.raw'))
    rows.tofile(src)
    ask('enlarge', W, H, 3 * W + pad, crop[0], crop[1], size[0], size[1], n, src, dst)
    return np.fromfile(dst, np.uint8).reshape(n, size[1], size[0], 3)


# -- the cases ------------------------------------------------------------------------------
EVERY_CROP = [(frame, name) for frame in FRAMES for name in sorted(OFF)]
# crops at most 23 pixels on a side, for the 7-fold targets: (frame, crop) with both sides starting on half pixels, on whole pixels, and mixed
SMALL = [((37, 50), (23, 22)), ((37, 50), (22, 23)), ((64, 48), (23, 17)), ((64, 48), (20, 23))]


def targets(crop):
    """{name: (w, h)}: the patch itself, one more on each axis alone and on both, just under a factor of 2, exactly 2, 3 x + 1."""
    cw, ch = crop
    return {'patch': (cw, ch), 'plus_w': (cw + 1, ch), 'plus_h': (cw, ch + 1), 'plus_both': (cw + 1, ch + 1), 'under_2': (2 * cw - 1, 2 * ch - 1),
            'twice': (2 * cw, 2 * ch), 'thrice_1': (3 * cw + 1, 3 * ch + 1)}


frames = cc.frames


@functools.lru_cache(maxsize=None)
def twin_of(W, H, crop, size, n=2):
    want = twin_enlarge(frames(W, H, n), crop, size)
    want.setflags(write=False)
    return want


@functools.lru_cache(maxsize=None)
def checkerboard(W, H):
    """0 / 255 by pixel: the bicubic overshoots on it in both passes."""
    y, x = np.mgrid[:H, :W]
    board = np.repeat((((x + y) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    board.setflags(write=False)
    return board
