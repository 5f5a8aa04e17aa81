"""What tests/test_mjpeg_stream.py (CPU) and the GPU suites (tests/test_encoders_gpu.py, tests/test_mjpeg_gpu.py) share: the CPU twin of the device-side Motion-JPEG encoder
(tests/mjpeg_check.cpp: csrc/kbe_mjpeg_block.h compiled by g++), the frames of the cases, and a reader of a stream's markers."""
import functools
import os
import re
import struct
import subprocess

import numpy as np

import twins
from test_jpeg_writer import photo_like

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BGR = 1                                                     # include/kbe.h: KBE_MJPEG_BGR
SIZES = [(96, 128), (50, 37), (17, 16), (16, 17), (1, 1), (3, 200)]
QUALITIES = [10, 50, 75, 92, 100]


def checker():
    """The twin, built once per process with the flags that define the stream: no contraction, no -ffast-math, no -march."""
    return twins.built('mjpeg_check', '-ffp-contract=off')


def twin(frames, quality, flags=0, packed=False):
    """(streams, stats, R, bound) of uint8 frames [n,H,W,3] from the CPU twin.  ``packed``: the intervals in the kernels' two steps."""
    frames = np.ascontiguousarray(frames, dtype=np.uint8)
    n, h, w, _ = frames.shape
    exe = checker()
    src, dst = os.path.join(os.path.dirname(exe), 'in.raw'), os.path.join(os.path.dirname(exe), 'out.bin')
    frames.tofile(src)
    out = subprocess.run([exe, 'encode_packed' if packed else 'encode', str(w), str(h), str(quality), str(flags), str(n), src, dst], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-1000:]
    sizes = [int(v) for v in re.search(r'^sizes(.*)$', out.stdout, flags=re.M).group(1).split()]
    data = open(dst, 'rb').read()
    assert len(sizes) == n and sum(sizes) == len(data)
    at = np.concatenate([[0], np.cumsum(sizes)])
    stats = {k: int(v) for k, v in re.findall(r'(\w+)=(\d+)', re.search(r'^stats (.*)$', out.stdout, flags=re.M).group(1))}
    return ([data[at[i]:at[i + 1]] for i in range(n)], stats, int(re.search(r'^R (\d+)$', out.stdout, flags=re.M).group(1)),
            int(re.search(r'^bound (\d+)$', out.stdout, flags=re.M).group(1)))


def noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def checkerboard(h, w, seed):
    """8 x 8 blocks of 0 and 255: at quality 100 neighbouring luma blocks' DC values differ by 2040, category 11."""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.repeat((((yy // 8 + xx // 8 + seed) & 1) * 255).astype(np.uint8)[:, :, None], 3, 2)


def speck(h, w, seed):
    """A flat frame but for one block of pixels that alternate by +-10: at quality 50 only the end of its zig-zag scan survives, behind
    a run of more than 15 zeros (ZRL)."""
    img = np.full((h, w, 3), 128, np.uint8)
    y, x = 8 + 16 * (seed % 2), 16 + 16 * (seed % 3)
    yy, xx = np.mgrid[0:8, 0:8]
    img[y:y + 8, x:x + 8] = (128 + 10 * (1 - 2 * ((yy + xx) & 1)))[:, :, None]
    return img


# name -> (frame maker(h, w, seed), (h, w), quality, first seed)
CASES = {'size_%dx%d' % s: (photo_like, s, 92, 3) for s in SIZES}
CASES.update({'quality_%d' % q: (photo_like, (48, 64), q, 1) for q in QUALITIES})
CASES.update({'noise': (noise, (64, 80), 100, 5),                   # stuffed bytes, blocks without EOB
              'checkerboard': (checkerboard, (32, 48), 100, 0),     # DC category 11
              'speck': (speck, (48, 64), 50, 0),                    # ZRL
              'rst_wrap': (photo_like, (13, 1125), 92, 7),          # 71 MCUs: more than 8 intervals and a short last one for any R in 2..8
              'widest': (photo_like, (2, 65535), 92, 4),            # the sides' limit (include/kbe.h): 4096 MCUs in one row ...
              'tallest': (photo_like, (65535, 2), 92, 4)})          # ... and 4096 rows of one MCU (beyond libjpeg's 65500: held to the twin, and the twin's two orders to each other)


@functools.lru_cache(maxsize=None)
def case_frames(name, n=1):
    make, (h, w), _, seed = CASES[name]
    frames = np.stack([make(h, w, seed + i) for i in range(n)])
    frames.setflags(write=False)
    return frames


@functools.lru_cache(maxsize=None)
def case_twin(name, n=1, flags=0):
    return twin(case_frames(name, n), CASES[name][2], flags)


def restart_interval(data):
    """R of a stream's DRI segment (None without one) and the RSTm indices of its scan, in order."""
    i, interval = 2, None
    while True:
        assert data[i] == 0xFF
        marker, n = data[i + 1], struct.unpack('>H', data[i + 2:i + 4])[0]
        if marker == 0xDD:
            interval = struct.unpack('>H', data[i + 4:i + 6])[0]
        i += 2 + n
        if marker == 0xDA:
            break
    scan = data[i:]
    # (inside the scan 0xFF is followed by a stuffed 0x00 unless it opens a marker)
    return interval, [scan[k + 1] - 0xD0 for k in range(len(scan) - 1) if scan[k] == 0xFF and 0xD0 <= scan[k + 1] <= 0xD7]
