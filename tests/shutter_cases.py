"""What tests/test_shutter_stream.py (CPU) and tests/test_shutter_gpu.py share: the NumPy twin of the shutter mean (include/kbe_shutter.h; defined
in csrc/kbe_shutter_block.h), the serial execution of that header (tests/shutter_check.cpp compiled by g++) and the frames of the cases."""
import functools
import os
import subprocess

import numpy as np

import gif_cases as gc
import twins

MAX_SAMPLES = 32
# (W, H) of the frames: a row of 111 bytes, odd; one of 192 bytes, whole pieces; several rows per workgroup and rows of 480 bytes
FRAMES = [(37, 50), (64, 48), (160, 128)]
SAMPLES = [1, 2, 3, 8, 31, 32]


def twin_mean(frames):
    """uint8 [n, S, H, W, 3] -> uint8 [n, H, W, 3]: (2 sum + S) // (2 S) on int64, the mean rounded half up."""
    frames = np.asarray(frames)
    assert frames.dtype == np.uint8 and frames.ndim == 5 and 1 <= frames.shape[1] <= MAX_SAMPLES
    S = frames.shape[1]
    return ((2 * frames.astype(np.int64).sum(axis=1) + S) // (2 * S)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def samples_of(W, H, S, n=2):
    """uint8 [n, S, H, W, 3]: output i's samples are a pan of one pixel per sample over a photo-like frame of W + S pixels."""
    out = np.stack([np.stack([gc.photo_like(H, W + S, 21 + i)[:, k:k + W] for k in range(S)]) for i in range(n)])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def twin_of(W, H, S, n=2):
    want = twin_mean(samples_of(W, H, S, n))
    want.setflags(write=False)
    return want


def differing_share(samples, mean):
    """The smallest share of the bytes in which the mean [n,H,W,3] differs from one of its samples [n,S,H,W,3]: a kernel that copies one sample
    has to fail in that many."""
    return min(float((samples[:, k] != mean).mean()) for k in range(samples.shape[1]))


# -- the header, serially -------------------------------------------------------------------
def checker():
    """tests/shutter_check.cpp, built once per process: no -ffast-math, no -march."""
    return twins.built('shutter_check')


def ask(*args):
    out = subprocess.run([checker()] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-1000:]
    return out.stdout


def _path(name):
    return os.path.join(os.path.dirname(checker()), name)


def header_mean(samples, pad=0):
    """uint8 [n, S, H, W, 3] through mean_row of csrc/kbe_shutter_block.h; ``pad``: that many bytes between the rows of the sources."""
    samples = np.asarray(samples, dtype=np.uint8)
    n, S, H, W, _ = samples.shape
    rows = np.full((n * S, H, 3 * W + pad), 0xEE, np.uint8)
    rows[:, :, :3 * W] = samples.reshape(n * S, H, 3 * W)
    rows.tofile(_path('in.raw'))
    ask('mean', W, H, 3 * W + pad, S, n, _path('in.raw'), _path('out.raw'))
    return np.fromfile(_path('out.raw'), np.uint8).reshape(n, H, W, 3)
