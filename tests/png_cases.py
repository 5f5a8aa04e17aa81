"""What tests/test_png_stream.py (CPU) and the GPU suites (tests/test_encoders_gpu.py, tests/test_png_gpu.py) share: the CPU twin of the device-side PNG encoder (tests/png_check.cpp:
csrc/kbe_png_block.h compiled by g++), the frames of the cases, and a reader of a PNG's chunks."""
import functools
import os
import re
import struct
import subprocess
import zlib

import numpy as np

import twins
from test_jpeg_writer import photo_like

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BGR = 1                                                     # include/kbe.h: KBE_PNG_BGR
SEGMENT = 16384                                             # csrc/kbe_png_block.h: kSegmentBytes (the twin prints it; test_png_stream.py compares)
SIZES = [(1, 1), (3, 200), (17, 16), (50, 37), (96, 128)]


def checker():
    """The twin, built once per process: no -ffast-math, no -march."""
    return twins.built('png_check')


def twin(frames, flags=0, pieces=False):
    """(files, stats, segment size, bound) of uint8 frames [n,H,W,3] from the CPU twin.  ``pieces``: the segments in the kernels' steps."""
    frames = np.ascontiguousarray(frames, dtype=np.uint8)
    n, h, w, _ = frames.shape
    exe = checker()
    src, dst = os.path.join(os.path.dirname(exe), 'in.raw'), os.path.join(os.path.dirname(exe), 'out.bin')
    frames.tofile(src)
    out = subprocess.run([exe, 'encode_pieces' if pieces else 'encode', str(w), str(h), str(flags), str(n), src, dst], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-1000:]
    sizes = [int(v) for v in re.search(r'^sizes(.*)$', out.stdout, flags=re.M).group(1).split()]
    data = open(dst, 'rb').read()
    assert len(sizes) == n and sum(sizes) == len(data)
    at = np.concatenate([[0], np.cumsum(sizes)])
    stats = {k: int(v) for k, v in re.findall(r'(\w+)=(\d+)', re.search(r'^stats (.*)$', out.stdout, flags=re.M).group(1))}
    return ([data[at[i]:at[i + 1]] for i in range(n)], stats, int(re.search(r'^segment (\d+)$', out.stdout, flags=re.M).group(1)),
            int(re.search(r'^bound (\d+)$', out.stdout, flags=re.M).group(1)))


def code_lengths(limit, histogram):
    """(lengths, whether the limit cut the tree, the Kraft sum's numerator and denominator) of the twin's code construction."""
    out = subprocess.run([checker(), 'lengths', str(limit)] + [str(int(v)) for v in histogram], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-1000:]
    kraft = re.search(r'^kraft (\d+) / (\d+)$', out.stdout, flags=re.M)
    return ([int(v) for v in re.search(r'^lengths(.*)$', out.stdout, flags=re.M).group(1).split()], int(re.search(r'^limited (\d)$', out.stdout, flags=re.M).group(1)),
            int(kraft.group(1)), int(kraft.group(2)))


def filtered(frame):
    """The bytes a frame's zlib stream carries: pipeline.png_bytes's own filter (Sub on every row)."""
    a = np.ascontiguousarray(frame, dtype=np.uint8)
    h, w = a.shape[:2]
    raw = np.empty((h, 1 + 3 * w), np.uint8)
    raw[:, 0] = 1
    flat = a.reshape(h, 3 * w)
    raw[:, 1:4] = flat[:, :3]
    raw[:, 4:] = flat[:, 3:] - flat[:, :-3]
    return raw.tobytes()


def unfiltered(rows):
    """The frame [h,w,3] whose rows' filtered bytes (without the filter byte) are rows [h,3w]: the Sub filter undone by a running sum."""
    rows = np.asarray(rows, dtype=np.uint8)
    return np.cumsum(rows.reshape(rows.shape[0], -1, 3), axis=1, dtype=np.uint8)


def noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def flat(h, w, seed):
    """One colour: rows of `1 c c c 0 0 0 ...`.  The zeros are chains of 258-byte matches with a remainder, cut by the next row's filter
    byte and, once, by a segment's end; the colour's bytes are a run of 3 (two remainder literals), of 2 (one) or, with the filter byte, of 4."""
    return np.full((h, w, 3), [(7, 7, 7), (9, 9, 200), (1, 1, 1)][seed % 3], np.uint8)


def stripes(h, w, seed):
    """Filtered rows made of runs of 2, 3, 4, 258, 259, 260 and 261 equal bytes (in an order that changes from row to row)."""
    lengths = [2, 3, 4, 258, 259, 260, 261]
    assert 3 * w >= sum(lengths)
    rows = np.empty((h, 3 * w), np.uint8)
    for y in range(h):
        at = 0
        for k in range(len(lengths)):
            n = lengths[(k + y + seed) % len(lengths)]
            rows[y, at:at + n] = ((37 * (k + 1) + 11 * seed) & 0xFF) | 1 if k & 1 else 0
            at += n
        rows[y, at:] = 5 + (seed & 3)
    return unfiltered(rows)


def fibonacci(h, w, seed):
    """ONE segment whose symbols' counts are the Fibonacci numbers 1, 1, 2, 3, 5 ... 4181: the end-of-block symbol is one 1, the three rows'
    filter bytes are the 3, and 17 filtered values have the other counts -- a Huffman tree as deep as these symbols are many, beyond the 15
    bits a code may take.  Five more values share the rest of the frame's bytes evenly (22 values in all; the chain stays 17 deep beside
    them).  No value repeats back to back: a stride through the sorted values that is longer than the most frequent value's count."""
    fib = [1, 1]
    while len(fib) < 19:
        fib.append(fib[-1] + fib[-2])
    counts = [f for f in fib[1:] if f != 3]
    rest = h * 3 * w - sum(counts)
    assert h == 3 and h * (1 + 3 * w) <= SEGMENT and rest >= 5
    counts += [(rest + k) // 5 for k in range(5)]
    values = np.repeat((np.arange(22) * 11 + 3 + seed).astype(np.uint8), counts)
    n = len(values)
    stride = next(k for k in range(max(counts) + 1 + seed, n) if np.gcd(k, n) == 1)
    assert stride > max(counts) and n - stride > max(counts)
    seq = values[(np.arange(n, dtype=np.int64) * stride) % n]
    return unfiltered(seq.reshape(h, 3 * w))


# name -> (frame maker(h, w, seed), (h, w), first seed)
CASES = {'size_%dx%d' % s: (photo_like, s, 3) for s in SIZES}
CASES.update({'one_segment': (photo_like, (64, 85), 2),             # 64 rows of 1 + 3 * 85 = 256 bytes: exactly SEGMENT
              'one_past_segment': (photo_like, (113, 48), 2),       # 113 * 145 = SEGMENT + 1: a last segment of one byte
              'flat': (flat, (40, 300), 0),
              'noise': (noise, (100, 80), 5),                       # every segment stored: the file is as long as the bound
              'stripes': (stripes, (16, 436), 0),
              'fibonacci': (fibonacci, (3, 1820), 0),                  # the length limit cuts the literal/length code
              'photo_like': (photo_like, (128, 160), 1),
              'row_one_segment': (photo_like, (3, 5461), 2),        # a row of 1 + 3 * 5461 bytes is exactly SEGMENT: every segment is one row
              'row_past_segment': (photo_like, (3, 5462), 2),       # ... and a row of SEGMENT + 3 bytes: every row crosses a segment's end, at another place
              'widest': (photo_like, (2, 65535), 4),                # the sides' limit (include/kbe.h): 12 segments per row
              'tallest': (photo_like, (65535, 2), 4)})              # ... and 2340 rows per segment


@functools.lru_cache(maxsize=None)
def case_frames(name, n=1):
    make, (h, w), seed = CASES[name]
    frames = np.stack([make(h, w, seed + i) for i in range(n)])
    frames.setflags(write=False)
    return frames


@functools.lru_cache(maxsize=None)
def case_twin(name, n=1, flags=0):
    return twin(case_frames(name, n), flags)


def chunks(data):
    """[(tag, body)] of a PNG file, every chunk's length and CRC-32 verified against zlib's."""
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    out, i = [], 8
    while i < len(data):
        n = struct.unpack('>I', data[i:i + 4])[0]
        tag, body = data[i + 4:i + 8], data[i + 8:i + 8 + n]
        assert len(body) == n and struct.unpack('>I', data[i + 8 + n:i + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF, tag
        out.append((tag, body))
        i += 12 + n
    assert i == len(data)
    return out
