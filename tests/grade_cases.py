"""What tests/test_grade_stream.py (CPU) and tests/test_grade_gpu.py share: the NumPy twin of the colour grade (include/kbe_grade.h), written
from the formulas and not from csrc/kbe_grade_block.h, a float64 reference of the same interpolation, the serial execution of that header
(tests/grade_check.cpp compiled by g++) and the tables of the cases.  The frames are overlay_cases.frames_of's."""
import functools
import os
import subprocess

import numpy as np

import overlay_cases as oc
import twins

frames_of, per_frame = oc.frames_of, oc.per_frame
FRAMES = oc.FRAMES                   # (37, 50), (64, 48), (160, 128)
SIZES = (2, 3, 17, 33)               # the tables' nodes per axis in the cases
STRENGTH = (256, 150)                # of the two frames of a case
EXACT_SIZES = (2, 4, 6, 16, 18)      # (N - 1) | 255: the identity table's nodes are exact


# -- the tables: uint8 [N,N,N,4], entry [i2, i1, i0] the node at frame byte 0 = i0, byte 1 = i1, byte 2 = i2; byte 3 is ignored -----------
def _nodes(N):
    return (2 * 255 * np.arange(N) + (N - 1)) // (2 * (N - 1))                  # round(255 j / (N - 1))


@functools.lru_cache(maxsize=None)
def identity(N):
    """Node (i0, i1, i2) -> (node(i0), node(i1), node(i2)), byte 3 noise."""
    v = _nodes(N)
    i2, i1, i0 = np.meshgrid(v, v, v, indexing='ij')
    t = np.stack([i0, i1, i2, (i0 + i1 + i2) & 255], axis=-1).astype(np.uint8)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def constant(N, colour=(17, 200, 99)):
    t = np.empty((N, N, N, 4), np.uint8)
    t[..., :3] = colour
    t[..., 3] = 0x5A
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def rotation(N):
    """(c0, c1, c2) -> (c1, c2, c0) at the nodes: a mistake in the order of the axes shows as another permutation."""
    t = np.ascontiguousarray(identity(N)[..., [1, 2, 0, 3]])
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def random(N, seed=3):
    t = np.random.default_rng(seed + N).integers(0, 256, (N, N, N, 4), dtype=np.uint8)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def sepia(bgr=True, N=33):
    from ken_burns_effect_amd import grade
    t = np.ascontiguousarray(grade.quantise(grade.bake(look='sepia', N=N), bgr)).view(np.uint8).reshape(N, N, N, 4)
    t.setflags(write=False)
    return t


TABLES = {'identity': identity, 'constant': constant, 'rotation': rotation, 'random': random}


def packed(table):
    """uint8 [N,N,N,4] -> the N^3 dwords."""
    return np.ascontiguousarray(table).view(np.uint32).reshape(table.shape[:3])


# -- the twin --------------------------------------------------------------------------------------
def cells(v, N):
    """(i, f) of bytes v: p = v (N - 1), i = p / 255, f = p - 255 i; v = 255: i = N - 2, f = 255."""
    p = np.asarray(v, dtype=np.int64) * (N - 1)
    i = p // 255
    f = p - 255 * i
    top = i == N - 1
    return np.where(top, N - 2, i), np.where(top, 255, f)


def _corners(pixels, N):
    """The four nodes' indices [4][..., 3] (as i0, i1, i2) and weights [4][...] of uint8 pixels [..., 3]; the weights add up to 255."""
    i, f = cells(pixels, N)
    order = np.argsort(-f, axis=-1, kind='stable')
    fs = np.take_along_axis(f, order, axis=-1)
    unit = np.eye(3, dtype=np.int64)
    ea, eb = unit[order[..., 0]], unit[order[..., 1]]
    return [i, i + ea, i + ea + eb, i + 1], [255 - fs[..., 0], fs[..., 0] - fs[..., 1], fs[..., 1] - fs[..., 2], fs[..., 2]]


def twin_grade(frames, table, strength=256):
    """uint8 [n,H,W,3] and a uint8 [N,N,N,4] table -> a new uint8 [n,H,W,3]: g = (sum of node * weight + 127) / 255 in integer division,
    out = (c (256 - s) + g s + 128) >> 8 with frame i's strength s."""
    frames, table = np.asarray(frames), np.asarray(table)
    assert frames.dtype == table.dtype == np.uint8 and frames.ndim == 4 and frames.shape[3] == 3 and table.ndim == 4 and table.shape[3] == 4
    N = table.shape[0]
    n = frames.shape[0]
    s = np.asarray(per_frame(strength, n), dtype=np.int64).reshape(n, 1, 1, 1)
    assert ((0 <= s) & (s <= 256)).all()
    at, weight = _corners(frames, N)
    nodes = table[..., :3].astype(np.int64)
    total = sum(w[..., None] * nodes[p[..., 2], p[..., 1], p[..., 0]] for w, p in zip(weight, at))
    g = (total + 127) // 255
    c = frames.astype(np.int64)
    return ((c * (256 - s) + g * s + 128) >> 8).astype(np.uint8)


def float_grade(frames, table):
    """The same interpolation of the same nodes in float64, unrounded: float64 [n,H,W,3]."""
    frames, table = np.asarray(frames), np.asarray(table)
    at, weight = _corners(frames, table.shape[0])
    nodes = table[..., :3].astype(np.float64)
    return sum((w / 255.0)[..., None] * nodes[p[..., 2], p[..., 1], p[..., 0]] for w, p in zip(weight, at))


@functools.lru_cache(maxsize=None)
def twin_of(W, H, N, kind):
    want = twin_grade(frames_of(W, H), TABLES[kind](N), STRENGTH)
    want.setflags(write=False)
    return want


@functools.lru_cache(maxsize=None)
def all_cells_frame():
    """uint8 [1,512,512,3]: all 64^3 combinations of 64 byte values per channel -- 0, 255 and each node's value at N = 17 and N = 33 (the
    least byte of each cell, ceil(255 j / (N - 1)): 33 values, N = 17's nodes being every other one of N = 33's), and the nodes' neighbours
    as far as 64 values hold them: the byte below each of N = 17's nodes (16 values, 254 among them: the last byte of the last cell) and
    the byte above N = 33's odd nodes 1..29 (15 values) -- which reaches every cell's edge from both sides, v = 255's clamp and every order
    and tie of the fractions."""
    node = lambda j, N: -(-255 * j // (N - 1))
    values = {node(j, 33) for j in range(33)}
    assert values >= {node(j, 17) for j in range(17)} | {0, 255} and len(values) == 33
    values |= {node(j, 17) - 1 for j in range(1, 17)} | {node(j, 33) + 1 for j in range(1, 30, 2)}
    values = np.asarray(sorted(values), dtype=np.uint8)
    assert len(values) == 64 and 254 in values
    c2, c1, c0 = np.meshgrid(values, values, values, indexing='ij')
    frame = np.stack([c0, c1, c2], axis=-1).reshape(1, 512, 512, 3)
    frame.setflags(write=False)
    return frame


# -- the header, serially ---------------------------------------------------------------------------
def checker():
    """tests/grade_check.cpp, built once per process: no -ffast-math, no -march."""
    return twins.built('grade_check')


def ask(*args):
    out = subprocess.run([checker()] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-1000:]
    return out.stdout


def _path(name):
    return os.path.join(os.path.dirname(checker()), name)


def header_grade(frames, table, strength=256, pad=0):
    """The frames through grade_row of csrc/kbe_grade_block.h; pad: that many bytes between the rows, so that the rows lie at other
    alignments.  The padding comes back as it went in, or the assertion here fails."""
    frames, table = np.asarray(frames, dtype=np.uint8), np.asarray(table, dtype=np.uint8)
    n, H, W, _ = frames.shape
    rows = np.full((n, H, 3 * W + pad), 0xEE, np.uint8)
    rows[:, :, :3 * W] = frames.reshape(n, H, 3 * W)
    with open(_path('in.raw'), 'wb') as f:
        f.write(rows.tobytes() + np.ascontiguousarray(table).tobytes())
    ask('grade', W, H, 3 * W + pad, n, table.shape[0], ','.join(str(v) for v in per_frame(strength, n)), _path('in.raw'), _path('out.raw'))
    got = np.fromfile(_path('out.raw'), np.uint8).reshape(n, H, 3 * W + pad)
    assert (got[:, :, 3 * W:] == 0xEE).all()
    return got[:, :, :3 * W].reshape(n, H, W, 3)
