"""What tests/test_yuv_stream.py (CPU) and tests/test_yuv_gpu.py share: the NumPy twin of the 4:2:0 planes (include/kbe_yuv.h; defined in
csrc/kbe_yuv_block.h), the serial execution of that header (tests/yuv_check.cpp compiled by g++), the frames of the cases, and a reader of the
y4m files yuv.write_y4m writes."""
import functools
import os
import re
import subprocess

import numpy as np

import gif_cases as gc
import twins

# (W, H) of the frames: rows of 37 pixels, odd, with an odd chroma width; 64 x 48, whole runs; several row pairs per workgroup and rows of ten runs
FRAMES = [(37, 50), (64, 48), (160, 128)]
BGR = 1
# the pinned values of the definition: (R, G, B) -> (Y, Cb, Cr), None: not pinned
PINNED = {(255, 255, 255): (235, 128, 128), (0, 0, 0): (16, 128, 128), (0, 0, 255): (None, 240, None), (255, 0, 0): (None, None, 240), (255, 255, 0): (None, 16, None)}
PRIMARIES = [(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255)]


def chroma_size(W, H):
    return (W + 1) // 2, (H + 1) // 2


def frame_bytes(W, H):
    cw, ch = chroma_size(W, H)
    return W * H + 2 * cw * ch


def twin_planes(frame, bgr=False):
    """uint8 [H, W, 3] -> (Y [H, W], Cb [ch, cw], Cr [ch, cw]) on int64 with //: the definition, cell sums over the pixels that exist."""
    frame = np.asarray(frame)
    assert frame.dtype == np.uint8 and frame.ndim == 3 and frame.shape[2] == 3
    p = frame.astype(np.int64)
    R, G, B = (p[:, :, 2], p[:, :, 1], p[:, :, 0]) if bgr else (p[:, :, 0], p[:, :, 1], p[:, :, 2])
    H, W = R.shape
    cw, ch = chroma_size(W, H)
    Y = 16 + ((66 * R + 129 * G + 25 * B + 128) >> 8)

    def cells(plane):
        padded = np.zeros((2 * ch, 2 * cw), np.int64)
        padded[:H, :W] = plane
        return padded.reshape(ch, 2, cw, 2).sum(axis=(1, 3))
    n = cells(np.ones((H, W), np.int64))
    Rs, Gs, Bs = cells(R), cells(G), cells(B)
    Cb = 128 + (-38 * Rs - 74 * Gs + 112 * Bs + 128 * n) // (256 * n)
    Cr = 128 + (112 * Rs - 94 * Gs - 18 * Bs + 128 * n) // (256 * n)
    assert Y.min() >= 16 and Y.max() <= 235 and min(Cb.min(), Cr.min()) >= 16 and max(Cb.max(), Cr.max()) <= 240
    return Y.astype(np.uint8), Cb.astype(np.uint8), Cr.astype(np.uint8)


def twin_payload(frames, bgr=False):
    """uint8 [n, H, W, 3] -> uint8 [n, frame_bytes]: every frame's Y plane, Cb plane, Cr plane."""
    frames = np.asarray(frames)
    assert frames.ndim == 4
    return np.stack([np.concatenate([plane.reshape(-1) for plane in twin_planes(f, bgr)]) for f in frames])


@functools.lru_cache(maxsize=None)
def frames_of(W, H, n=2, seed=31):
    out = np.stack([gc.photo_like(H, W, seed + i) for i in range(n)])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def twin_of(W, H, bgr, n=2, seed=31):
    want = twin_payload(frames_of(W, H, n, seed), bgr)
    want.setflags(write=False)
    return want


def telling(frame):
    """The shares that keep a copying or half-right kernel from passing: (the smallest share of the pixels in which Y differs from one of the
    frame's three channels, the share of the cells in which Cb differs from Cr, the share of the pixels in which Y with the BGR flag differs
    from Y without)."""
    Y, Cb, Cr = twin_planes(frame)
    return min(float((Y != frame[:, :, c]).mean()) for c in range(3)), float((Cb != Cr).mean()), float((twin_planes(frame, True)[0] != Y).mean())


def assert_telling(frames):
    for frame in frames:
        shares = telling(frame)
        assert min(shares) > 0.9, shares


def flat(colour, W=5, H=3, n=1):
    return np.broadcast_to(np.array(colour, np.uint8), (n, H, W, 3)).copy()


# -- the header, serially -------------------------------------------------------------------
def checker():
    """tests/yuv_check.cpp, built once per process: no -ffast-math, no -march."""
    return twins.built('yuv_check')


def ask(*args):
    out = subprocess.run([checker()] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-1000:]
    return out.stdout


def _path(name):
    return os.path.join(os.path.dirname(checker()), name)


def header_payload(frames, bgr=False, pad=0):
    """uint8 [n, H, W, 3] through convert_frame of csrc/kbe_yuv_block.h; ``pad``: that many bytes between the rows of the sources."""
    frames = np.asarray(frames, dtype=np.uint8)
    n, H, W, _ = frames.shape
    rows = np.full((n, H, 3 * W + pad), 0xEE, np.uint8)
    rows[:, :, :3 * W] = frames.reshape(n, H, 3 * W)
    rows.tofile(_path('in.raw'))
    ask('convert', W, H, 3 * W + pad, BGR if bgr else 0, n, _path('in.raw'), _path('out.raw'))
    return np.fromfile(_path('out.raw'), np.uint8).reshape(n, frame_bytes(W, H))


# -- a y4m file, parsed back ------------------------------------------------------------------
def read_y4m(path):
    """-> (the header line with its newline, [the payload of every FRAME as a uint8 array])."""
    with open(path, 'rb') as f:
        data = f.read()
    end = data.index(b'\n') + 1
    header = data[:end]
    W, H = (int(v) for v in re.match(rb'YUV4MPEG2 W(\d+) H(\d+) ', header).groups())
    size, payloads = frame_bytes(W, H), []
    while end < len(data):
        assert data[end:end + 6] == b'FRAME\n', data[end:end + 6]
        payloads.append(np.frombuffer(data[end + 6:end + 6 + size], np.uint8))
        assert payloads[-1].size == size
        end += 6 + size
    return header, payloads
