"""What tests/test_gif_stream.py, tests/test_header_bindings.py (CPU) and tests/test_gif_gpu.py share: the CPU twin of the device-side GIF encoder
(tests/gif_check.cpp: csrc/kbe_gif_block.h compiled by g++), the cases and their frames, a NumPy restatement of pixel -> index, of the
look-up table and of the histogram, and a small reader of GIF files that returns what Pillow does not show: the sub-blocks' sizes and the
LZW codes with their widths and bit positions."""
import functools
import os
import re
import struct
import subprocess

import numpy as np

import twins
from test_jpeg_writer import photo_like

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BGR = 1                                                     # include/kbe_gif.h: KBE_GIF_BGR
SEGMENT = 3838                                              # csrc/kbe_gif_block.h: kSegmentPixels (the twin prints it; test_gif_stream.py compares)
DITHER = 8                                                  # gif.DITHER['ordered']
CELLS = 32768


def checker():
    """The twin, built once per process: no -ffast-math, no -march."""
    return twins.built('gif_check')


def ask(*args):
    out = subprocess.run([checker()] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-1000:]
    return out.stdout


def twin(frames, lut, flags=0, dither=0, delay_cs=4, pieces=False):
    """(units, stats, segment size, bound) of uint8 frames [n,H,W,3] and a cell -> index table from the CPU twin.  ``pieces``: the segments
    in the kernels' steps."""
    frames = np.ascontiguousarray(frames, dtype=np.uint8)
    n, h, w, _ = frames.shape
    src, table, dst = (os.path.join(os.path.dirname(checker()), name) for name in ('in.raw', 'lut.bin', 'out.bin'))
    frames.tofile(src)
    np.ascontiguousarray(lut, dtype=np.uint8).reshape(CELLS).tofile(table)
    text = ask('encode_pieces' if pieces else 'encode', w, h, flags, dither, delay_cs, n, src, table, dst)
    sizes = [int(v) for v in re.search(r'^sizes(.*)$', text, flags=re.M).group(1).split()]
    data = open(dst, 'rb').read()
    assert len(sizes) == n and sum(sizes) == len(data)
    at = np.concatenate([[0], np.cumsum(sizes)])
    stats = {k: int(v) for k, v in re.findall(r'(\w+)=(\d+)', re.search(r'^stats (.*)$', text, flags=re.M).group(1))}
    return ([data[at[i]:at[i + 1]] for i in range(n)], stats, int(re.search(r'^segment (\d+)$', text, flags=re.M).group(1)),
            int(re.search(r'^bound (\d+)$', text, flags=re.M).group(1)))


def twin_bound(w, h):
    return int(re.search(r'^bound (\d+)$', ask('bound', w, h), flags=re.M).group(1))


def twin_widths(ks):
    """{k: (code_width(k), bits_before(k))} of the header's closed forms."""
    return {int(k): (int(w), int(b)) for k, w, b in re.findall(r'^width (\d+) (\d+) (\d+)$', ask('widths', *ks), flags=re.M)}


# -- the NumPy restatement ------------------------------------------------------------------
def bayer8():
    """[y, x] -> 0..63: the bits of (x ^ y, y) interleaved and reversed."""
    y, x = np.meshgrid(np.arange(8), np.arange(8), indexing='ij')
    q, m = x ^ y, np.zeros((8, 8), np.int64)
    for i in range(3):
        m |= ((((y >> i) & 1) << 1) | ((q >> i) & 1)) << (2 * (2 - i))
    return m


def cells(frames, bgr=False, dither=0):
    """The RGB555 cell of every pixel of uint8 frames [..., H, W, 3]: the channels swapped, the ordered dither, r5 << 10 | g5 << 5 | b5."""
    a = np.asarray(frames).astype(np.int64)
    if bgr:
        a = a[..., ::-1]
    if dither:
        h, w = a.shape[-3], a.shape[-2]
        m = np.tile(bayer8(), (-(-h // 8), -(-w // 8)))[:h, :w]
        a = np.clip(a + ((m * dither) >> 6)[..., None] - (dither >> 1), 0, 255)
    return ((a[..., 0] >> 3) << 10) | ((a[..., 1] >> 3) << 5) | (a[..., 2] >> 3)


def centres(cell):
    cell = np.asarray(cell)
    v5 = np.stack([(cell >> 10) & 31, (cell >> 5) & 31, cell & 31], axis=-1).astype(np.int64)
    return (v5 << 3) | (v5 >> 2)


def lut_of(palette):
    """The index of the palette entry nearest to every cell's centre: squared Euclidean distance, ties to the lowest index (argmin's rule)."""
    p = np.asarray(palette).astype(np.int64)
    d = ((centres(np.arange(CELLS))[:, None, :] - p[None, :, :]) ** 2).sum(axis=2)
    return np.argmin(d, axis=1).astype(np.uint8)


def hist_of(frames, bgr=False):
    return np.bincount(cells(frames, bgr).reshape(-1), minlength=CELLS).astype(np.int64)


def psnr(a, b):
    return 10.0 * np.log10(255.0 ** 2 / np.mean((np.asarray(a).astype(np.float64) - np.asarray(b).astype(np.float64)) ** 2))


# -- the cases ------------------------------------------------------------------------------
def noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def flat(h, w, seed):
    return np.full((h, w, 3), [(7, 7, 7), (9, 9, 200), (250, 1, 1)][seed % 3], np.uint8)


def two_colours(h, w, seed):
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    pair = np.array([[(10, 200, 30), (240, 20, 90)], [(0, 0, 0), (255, 255, 255)], [(90, 90, 200), (200, 90, 90)]][seed % 3], np.uint8)
    return pair[(x + y + seed) & 1]


IDENTITY = np.stack([np.arange(256) >> 3, (np.arange(256) & 7) * 4, np.zeros(256, np.int64)], axis=1)
IDENTITY = ((IDENTITY << 3) | (IDENTITY >> 2)).astype(np.uint8)         # 256 cell centres, every one a cell of its own: the indices survive


def no_pair_twice(h, w, seed):
    """Indices in which no adjacent pair repeats inside a segment: from x the walk goes on to x + d modulo 256 with d = 1 for 256 steps, then
    3, 5, ... 29 -- an odd d visits every x once, so every (x, d) occurs at most once in SEGMENT <= 15 * 256 pixels; every segment starts the walk
    anew.  No match ever reaches two pixels: every code covers one pixel and the unit is as long as the bound."""
    assert SEGMENT <= 128 * 256
    i = np.arange(SEGMENT)
    walk = np.concatenate([[0], np.cumsum(2 * (i[:-1] // 256) + 1)]) % 256
    idx = (np.tile(walk, -(-h * w // SEGMENT))[:h * w] + 7 * seed) % 256
    return IDENTITY[idx].reshape(h, w, 3)


# name -> (frame maker(h, w, seed), (h, w), first seed)
CASES = {'%dx%d' % s: (photo_like, s, 3) for s in [(1, 1), (3, 200), (17, 16), (50, 37), (96, 128)]}
CASES.update({'one_segment': (photo_like, (38, 101), 2),             # exactly SEGMENT pixels
              'one_past_segment': (photo_like, (11, 349), 2),        # SEGMENT + 1: a last segment of one pixel
              'flat': (flat, (40, 300), 0),                          # KwKwK, the longest matches
              'two_colours': (two_colours, (33, 47), 0),
              'noise': (noise, (60, 80), 5),
              'no_pair_twice': (no_pair_twice, (90, 100), 0),       # two whole segments and a short one, all at the bound
              'photo_like': (photo_like, (128, 160), 1),
              'widest': (photo_like, (2, 65535), 4),                 # the sides' limit
              'tallest': (photo_like, (65535, 2), 4)})


@functools.lru_cache(maxsize=None)
def case_frames(name, n=1):
    make, (h, w), seed = CASES[name]
    frames = np.stack([make(h, w, seed + i) for i in range(n)])
    frames.setflags(write=False)
    return frames


@functools.lru_cache(maxsize=None)
def case_palette(name, flags=0):
    """The case's palette and table: gif.palette_from_histogram on the first frame's histogram (one palette for all of a case's frames);
    no_pair_twice: the identity-like palette."""
    from ken_burns_effect_amd import gif
    palette = IDENTITY if name == 'no_pair_twice' else gif.palette_from_histogram(hist_of(case_frames(name, 1), bool(flags & BGR)))
    table = lut_of(palette)
    table.setflags(write=False)
    return palette, table


@functools.lru_cache(maxsize=None)
def case_twin(name, n=1, flags=0, dither=0):
    return twin(case_frames(name, n), case_palette(name, flags)[1], flags, dither)


# -- a reader -------------------------------------------------------------------------------
def read_gif(data):
    """{'width', 'height', 'palette' [256,3], 'loop', 'frames': [{'delay', 'disposal', 'transparent', 'left', 'top', 'width', 'height',
    'local_table', 'interlace', 'min_code_size', 'blocks': the data sub-blocks' sizes, 'codes': [(value, width, bit position)], 'indices'}]}
    of a GIF89a file with a global colour table.  The LZW decoder is the format's: Clear 256, EOI 257, 9 bits growing when the table
    reaches a power of two, at most 12; it asserts that no code exceeds the table and that the table never holds 4096 entries."""
    assert data[:6] == b'GIF89a'
    w, h, packed, _, _ = struct.unpack('<HHBBB', data[6:13])
    assert packed & 0x80, 'no global colour table'
    size = 2 << (packed & 7)
    out = {'width': w, 'height': h, 'packed': packed, 'palette': np.frombuffer(data[13:13 + 3 * size], np.uint8).reshape(size, 3), 'loop': None, 'frames': []}
    i, pending = 13 + 3 * size, {}

    def blocks(i):
        sizes, body = [], b''
        while data[i]:
            sizes.append(data[i])
            body += data[i + 1:i + 1 + data[i]]
            i += 1 + data[i]
        return sizes, body, i + 1
    while data[i] != 0x3B:
        if data[i] == 0x21:
            label = data[i + 1]
            sizes, body, i = blocks(i + 2)
            if label == 0xF9:
                assert sizes == [4]
                pending = {'disposal': (body[0] >> 2) & 7, 'transparent': body[0] & 1, 'delay': struct.unpack('<H', body[1:3])[0]}
            elif label == 0xFF and body[:11] == b'NETSCAPE2.0':
                assert sizes == [11, 3] and body[11] == 1
                out['loop'] = struct.unpack('<H', body[12:14])[0]
        else:
            assert data[i] == 0x2C
            left, top, fw, fh, fpacked = struct.unpack('<HHHHB', data[i + 1:i + 10])
            frame = dict(pending, left=left, top=top, width=fw, height=fh, local_table=bool(fpacked & 0x80), interlace=bool(fpacked & 0x40), min_code_size=data[i + 10])
            frame['blocks'], body, i = blocks(i + 11)
            frame['codes'], frame['indices'] = lzw_codes(body)
            out['frames'].append(frame)
            pending = {}
    assert i == len(data) - 1
    return out


def lzw_codes(body):
    """([(value, width, bit position)], the indices) of an LZW stream with minimum code size 8."""
    codes, indices, at, width = [], [], 0, 9
    table, previous = None, None
    acc, have, taken = 0, 0, 0                  # bits not yet read, their number, bytes taken from the body
    while True:
        assert at + width <= 8 * len(body), 'the stream ends without EOI'
        while have < width:
            acc |= body[taken] << have
            have += 8
            taken += 1
        value = acc & ((1 << width) - 1)
        acc >>= width
        have -= width
        codes.append((value, width, at))
        at += width
        if value == 256:
            table, previous, width = {}, None, 9
            continue
        if value == 257:
            break
        assert table is not None, 'data in front of the first Clear'
        entries = 258 + len(table)
        if previous is None:
            assert value < 256
            string = (value,)
        else:
            assert value <= entries, 'a code beyond the table'
            string = table[value] if value >= 258 and value < entries else (value,) if value < 256 else previous + previous[:1]
            assert value not in (256, 257)
            table[entries] = previous + string[:1]
            assert entries + 1 < 4096, 'the table is full'
            if entries + 1 == 1 << width and width < 12:
                width += 1
        indices.extend(string)
        previous = string
    assert taken == len(body) and acc == 0, 'bits behind EOI'
    return codes, np.array(indices, dtype=np.uint8)
