"""What tests/test_transition_stream.py (CPU) and tests/test_transition_gpu.py share: the NumPy twin of the transitions (include/kbe_transition.h),
written from the formulas and not from csrc/kbe_transition_block.h, the serial execution of that header (tests/transition_check.cpp compiled by
g++) and the frames of the cases."""
import functools
import os
import subprocess

import numpy as np

import gif_cases as gc
import twins

KINDS = {'dissolve': 0, 'wipe-right': 1, 'wipe-left': 2, 'wipe-down': 3, 'wipe-up': 4, 'fade': 5}
WIPES = ('wipe-right', 'wipe-left', 'wipe-down', 'wipe-up')
# (W, H) of the frames: a row of 111 bytes, odd; one of 192 bytes, whole pieces; several rows per workgroup and rows of 480 bytes
FRAMES = [(37, 50), (64, 48), (160, 128)]
PROGRESS = (128, 85)                 # of the two frames of a case
SOFTNESS = 8
COLOUR = 10 | (200 << 8) | (90 << 16)       # the bytes (10, 200, 90) of a pixel


def blend(a, b, w):
    """(a (256 - w) + b w + 128) >> 8 on int64."""
    a, b, w = (np.asarray(v, dtype=np.int64) for v in (a, b, w))
    return (a * (256 - w) + b * w + 128) >> 8


def progress_table(T):
    return [(512 * (j + 1) + (T + 1)) // (2 * (T + 1)) for j in range(T)]


def weight_map(kind, p, W, H, s):
    """int64 [H, W]: the weight of every pixel under the dissolve and the wipes."""
    kind = KINDS.get(kind, kind)
    assert 0 <= kind <= 4 and 0 <= p <= 256 and 1 <= s <= 65535
    if kind == 0:
        return np.full((H, W), p, np.int64)
    x, y = np.meshgrid(np.arange(W, dtype=np.int64), np.arange(H, dtype=np.int64))
    t, L = {1: (x, W), 2: (W - 1 - x, W), 3: (y, H), 4: (H - 1 - y, H)}[kind]
    num = p * (L + s) - 256 * t
    return np.where(num <= 0, 0, np.minimum(256, np.maximum(num, 0) // s))


def twin_blend(frames_from, frames_to, kind, progress, softness=SOFTNESS, colour=0):
    """uint8 [n,H,W,3] twice -> uint8 [n,H,W,3]: frame i at progress[i]."""
    a, b = np.asarray(frames_from), np.asarray(frames_to)
    kind = KINDS.get(kind, kind)
    assert a.dtype == b.dtype == np.uint8 and a.shape == b.shape and a.ndim == 4 and len(progress) == a.shape[0] and 0 <= colour < 1 << 24
    n, H, W, _ = a.shape
    out = np.empty_like(a)
    for i, p in enumerate(progress):
        if kind == 5:
            c = np.array([(colour >> (8 * k)) & 255 for k in range(3)], np.int64)[None, None, :]
            out[i] = blend(a[i], c, 2 * p) if p <= 128 else blend(c, b[i], 2 * p - 256)
        else:
            out[i] = blend(a[i], b[i], weight_map(kind, p, W, H, softness)[:, :, None])
    return out


@functools.lru_cache(maxsize=None)
def frames_of(W, H, n=2, seed=21):
    """(from, to): uint8 [n,H,W,3] each, photo-like frames of different seeds."""
    pair = tuple(np.stack([gc.photo_like(H, W, first + i) for i in range(n)]) for first in (seed, seed + 40))
    for frames in pair:
        frames.setflags(write=False)
    return pair


@functools.lru_cache(maxsize=None)
def twin_of(W, H, kind, progress=PROGRESS, softness=SOFTNESS, colour=COLOUR):
    a, b = frames_of(W, H, len(progress))
    want = twin_blend(a, b, kind, progress, softness, colour)
    want.setflags(write=False)
    return want


def soft_edge(kind, p, W, H, s):
    """bool [H, W, 3] -> [H, 3 W]: the bytes whose weight is neither 0 nor 256."""
    w = weight_map(kind, p, W, H, s)
    return np.repeat(((w > 0) & (w < 256))[:, :, None], 3, axis=2)


# -- the header, serially -------------------------------------------------------------------
def checker():
    """tests/transition_check.cpp, built once per process: no -ffast-math, no -march."""
    return twins.built('transition_check')


def ask(*args):
    out = subprocess.run([checker()] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-1000:]
    return out.stdout


def _path(name):
    return os.path.join(os.path.dirname(checker()), name)


def header_blend(frames_from, frames_to, kind, progress, softness=SOFTNESS, colour=0, pad=0):
    """Two uint8 [n,H,W,3] through blend_row of csrc/kbe_transition_block.h; ``pad``: that many bytes between the rows of the sources."""
    a, b = np.asarray(frames_from, dtype=np.uint8), np.asarray(frames_to, dtype=np.uint8)
    n, H, W, _ = a.shape
    rows = np.full((2 * n, H, 3 * W + pad), 0xEE, np.uint8)
    rows[:n, :, :3 * W] = a.reshape(n, H, 3 * W)
    rows[n:, :, :3 * W] = b.reshape(n, H, 3 * W)
    rows.tofile(_path('in.raw'))
    ask('blend', W, H, 3 * W + pad, KINDS.get(kind, kind), softness, colour, n, ','.join(str(int(p)) for p in progress), _path('in.raw'), _path('out.raw'))
    return np.fromfile(_path('out.raw'), np.uint8).reshape(n, H, W, 3)


def header_weights(kind, p, W, H, s):
    """int64 [H, W]: the weights as a lane of the kernel derives them (plan and weight of the header)."""
    ask('weights', W, H, KINDS.get(kind, kind), s, p, _path('w.raw'))
    return np.fromfile(_path('w.raw'), np.uint16).reshape(H, W).astype(np.int64)
