"""What tests/test_area_stream.py, tests/test_header_bindings.py (CPU) and tests/test_area_gpu.py share: the NumPy twin of the exact area-average
reduction (include/kbe_area.h; defined in csrc/kbe_area_block.h), the serial execution of that header (tests/area_check.cpp compiled by g++)
and the frames of the cases."""
import functools
import os
import subprocess

import numpy as np

import gif_cases as gc
import twins

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# -- the NumPy twin -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def weights(n, N):
    """int64 [n, N]: the overlap of target cell o = [o N, (o + 1) N) and source cell s = [s n, (s + 1) n) on an axis of N n units."""
    assert 1 <= n <= N
    o, s = np.arange(n, dtype=np.int64)[:, None], np.arange(N, dtype=np.int64)[None, :]
    A = np.clip(np.minimum((s + 1) * n, (o + 1) * N) - np.maximum(s * n, o * N), 0, None)
    A.setflags(write=False)
    return A


def twin_reduce(frames, w, h):
    """uint8 [..., H, W, 3] -> uint8 [..., h, w, 3]: S = sum of wy wx v in int64, (2 S + W H) // (2 W H)."""
    a = np.asarray(frames)
    assert a.dtype == np.uint8 and a.shape[-1] == 3
    H, W = a.shape[-3], a.shape[-2]
    S = np.einsum('oy,...yxc,px->...opc', weights(h, H), a.astype(np.int64), weights(w, W), optimize=True)
    assert S.dtype == np.int64
    return ((2 * S + W * H) // (2 * W * H)).astype(np.uint8)


# -- the header, serially -------------------------------------------------------------------
def checker():
    """tests/area_check.cpp, built once per process: no -ffast-math, no -march."""
    return twins.built('area_check')


def ask(*args):
    out = subprocess.run([checker()] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-1000:]
    return out.stdout


def header_reduce(frames, w, h, pad=0):
    """The same frames through reduce_pixel of csrc/kbe_area_block.h; ``pad``: that many bytes between the rows."""
    frames = np.asarray(frames, dtype=np.uint8)
    n, H, W, _ = frames.shape
    rows = np.full((n, H, 3 * W + pad), 0xEE, np.uint8)
    rows[:, :, :3 * W] = frames.reshape(n, H, 3 * W)
    src, dst = (os.path.join(os.path.dirname(checker()), name) for name in ('in.raw', 'out.raw'))
    rows.tofile(src)
    ask('reduce', W, H, 3 * W + pad, w, h, n, src, dst)
    return np.fromfile(dst, np.uint8).reshape(n, h, w, 3)


# -- the cases ------------------------------------------------------------------------------
# 160 x 128 (W x H) photo-like frames to: a ratio that is no integer on either axis; an integer factor; a ratio just under 1, where most
# targets straddle two sources; a copy; one pixel
TARGETS = {'non_integer': (75, 60), 'integer': (80, 64), 'just_under_1': (159, 127), 'copy': (160, 128), 'one_pixel': (1, 1)}


def photo(n):
    """n frames [128, 160, 3] of gif_cases' photo_like case."""
    return gc.case_frames('photo_like', n)


@functools.lru_cache(maxsize=None)
def small():
    """17 wide, 16 high: smaller than a tile of the kernel."""
    frames = np.stack([gc.photo_like(16, 17, 3 + i) for i in range(2)])
    frames.setflags(write=False)
    return frames


@functools.lru_cache(maxsize=None)
def large():
    """One 1000 x 1000 frame and its twin at 333 x 777: several tiles and strips of the kernel on both axes, a ratio above 3."""
    import encoder_gpu as eg
    frame = np.ascontiguousarray(eg.tiled(1000, 1000, 11)[None])
    want = twin_reduce(frame, 333, 777)
    frame.setflags(write=False)
    want.setflags(write=False)
    return frame, want


@functools.lru_cache(maxsize=None)
def twin_of(name, n=1):
    want = twin_reduce(photo(n), *TARGETS[name])
    want.setflags(write=False)
    return want
