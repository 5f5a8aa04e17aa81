"""What tests/test_sharpen_stream.py (CPU) and tests/test_sharpen_gpu.py share: the NumPy twin of the output sharpening (include/kbe_sharpen.h;
defined in csrc/kbe_sharpen_block.h) -- int64 throughout, written from the header's four formulas and not from the block header --, the twin
of sharpen.taps_for, the serial execution of the block header (tests/sharpen_check.cpp compiled by g++ under its sanitizers) and the cases.
The frames are tests/enlarge_cases.py's and tests/encoder_gpu.py's."""
import functools
import math
import os
import subprocess

import numpy as np

import enlarge_cases as ec
import twins

ONE, MAX_RADIUS, MAX_AMOUNT = 32768, 24, 1024
FRAMES = ec.FRAMES                                                   # (37, 50), (64, 48), (160, 128)
SIGMAS = {1: 0.3, 2: 0.6, 7: 2.3, 24: 8.0}                          # a sigma for each radius of the cases: R = min(24, max(1, ceil(3 sigma)))
frames, wide = ec.frames, ec.wide


# -- the taps -------------------------------------------------------------------------------
def radius_of(sigma):
    return min(MAX_RADIUS, max(1, math.ceil(3.0 * sigma)))


@functools.lru_cache(maxsize=None)
def taps_of(sigma):
    """The twin of sharpen.taps_for, in NumPy's float64: (w_0, .., w_R)."""
    R = radius_of(sigma)
    g = np.exp(-np.arange(R + 1, dtype=np.float64) ** 2 / (2.0 * sigma * sigma))
    G = g[0] + 2.0 * g[1:].sum()
    w = np.floor(ONE * g[1:] / G + 0.5).astype(np.int64)
    return (int(ONE - 2 * w.sum()),) + tuple(int(v) for v in w)


def taps_at(R):
    return taps_of(SIGMAS[R])


# -- the NumPy twin -------------------------------------------------------------------------
def _blur(values, taps, axis):
    """sum_k w[|k|] values(clamp(i + k)) along `axis` of an int64 array."""
    R = len(taps) - 1
    n = values.shape[axis]
    pad = [(0, 0)] * values.ndim
    pad[axis] = (R, R)
    padded = np.pad(values, pad, mode='edge')
    total = np.zeros_like(values)
    for k in range(-R, R + 1):
        total += taps[abs(k)] * np.take(padded, np.arange(R + k, R + k + n), axis=axis)
    return total


def twin_blur(frames_u8, taps):
    """uint8 [..., H, W, 3] -> int64 b16, the blur in 8.8 fixed point."""
    v = np.asarray(frames_u8).astype(np.int64)
    h16 = (_blur(v, taps, -2) + 64) >> 7
    return (_blur(h16, taps, -3) + 16384) >> 15


def twin_sharpen(frames_u8, taps, amount=256, threshold=0):
    """uint8 [..., H, W, 3] -> uint8 of the same shape: the unsharp mask, by the four formulas."""
    frames_u8 = np.asarray(frames_u8)
    assert frames_u8.dtype == np.uint8 and frames_u8.shape[-1] == 3 and taps[0] + 2 * sum(taps[1:]) == ONE
    v = frames_u8.astype(np.int64)
    d = 256 * v - twin_blur(frames_u8, taps)
    s = np.clip(v + ((amount * d + 32768) >> 16), 0, 255)          # (NumPy's >> of a negative int64 is a floor)
    return np.where(np.abs(d) < 256 * threshold, v, s).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def twin_of(W, H, R, amount=256, threshold=0, n=2):
    want = twin_sharpen(frames(W, H, n), taps_at(R), amount, threshold)
    want.setflags(write=False)
    return want


# -- the header, serially -------------------------------------------------------------------
def checker():
    """tests/sharpen_check.cpp, built once per process under UBSan's signed-integer-overflow check and AddressSanitizer: a plain program."""
    return twins.built('sharpen_check', '-fsanitize=signed-integer-overflow,address', '-fno-sanitize-recover=all')


def ask(*args):
    out = subprocess.run([checker()] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
    return out.stdout


def header_sharpen(frames_u8, taps, amount=256, threshold=0, pad=0):
    """The same frames through sharpen_pixel of csrc/kbe_sharpen_block.h; ``pad``: that many bytes between the rows."""
    frames_u8 = np.asarray(frames_u8, dtype=np.uint8)
    n, H, W, _ = frames_u8.shape
    rows = np.full((n, H, 3 * W + pad), 0xEE, np.uint8)
    rows[:, :, :3 * W] = frames_u8.reshape(n, H, 3 * W)
    src, dst = (os.path.join(os.path.dirname(checker()), name) for name in ('in.raw', 'out.raw'))
    rows.tofile(src)
    ask('sharpen', W, H, 3 * W + pad, n, amount, threshold, len(taps) - 1, *taps, src, dst)
    return np.fromfile(dst, np.uint8).reshape(n, H, W, 3)


# -- the cases ------------------------------------------------------------------------------
RADII = (1, 2, 7, 24)
EVERY = [(frame, R) for frame in FRAMES for R in RADII]
AMOUNTS, THRESHOLDS = (1, 256, 1024), (0, 3, 255)
THIN = [(1, 1), (1, 40), (40, 1)]                                     # (W, H)


@functools.lru_cache(maxsize=None)
def thin(W, H, n=2):
    import encoder_gpu as eg
    out = np.stack([np.ascontiguousarray(eg.tiled(H, W, 21 + i)) for i in range(n)])
    out.setflags(write=False)
    return out


# -- a float64 unsharp mask -----------------------------------------------------------------
def float_sharpen(frames_u8, sigma, amount, threshold=0):
    """The unsharp mask in float64 with exact Gaussian weights over the same radius, the edge replicated -> float64, not rounded, not clamped."""
    R = radius_of(sigma)
    g = np.exp(-np.arange(-R, R + 1, dtype=np.float64) ** 2 / (2.0 * sigma * sigma))
    g /= g.sum()
    v = np.asarray(frames_u8).astype(np.float64)
    blur = v
    for axis in (-2, -3):
        pad = [(0, 0)] * v.ndim
        pad[axis] = (R, R)
        padded = np.pad(blur, pad, mode='edge')
        blur = sum(g[R + k] * np.take(padded, np.arange(R + k, R + k + v.shape[axis]), axis=axis) for k in range(-R, R + 1))
    d = v - blur
    return np.where(np.abs(d) < threshold, v, v + amount * d)
