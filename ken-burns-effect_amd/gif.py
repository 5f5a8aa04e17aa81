"""An animated GIF of frames that lie in HBM, encoded on the GPU (include/kbe_gif.h: kbe_gif_histogram, kbe_gif_lut, kbe_gif_encode; the stream
is defined in csrc/kbe_gif_block.h).  Opt-in: ``Pipeline(gif=True)`` / env KBE_GIF=1 / ``kbe.py --gif`` writes ``3d_kbe.gif`` beside the video.

The device writes one UNIT per frame (graphic control extension, image descriptor, LZW data); this module binds the entries, chooses the
one global palette (a count-weighted median cut of the frames' RGB555 histogram, on the host: 32 768 counts) and assembles the file.  It is
the only module that names the entries of kbe_gif.h: they are exported by libkbe_hip.so beside those of kbe.h and typed from their own header
on the package's one handle of that library (_native.load; _cabi.Header).  No fallback: without the HIP library every call here raises.

write_gif(size=, every=) writes a GIF smaller than the render and of fewer frames (``kbe.py --gif-width, --gif-fps``): the frames are reduced on
the device first, by area.reduce (area.py binds that entry; this module names none of its).
"""
import os
import struct
from fractions import Fraction

import numpy as np

from . import _cabi, _native

HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'kbe_gif.h')
ABI_VERSION = 1
KBE_GIF_BGR = 1
CELLS = 32768
DITHER = {'none': 0, 'ordered': 8}      # the amplitude of the ordered dither: 8 is one step of a 5-bit channel
HEADER = _cabi.Header(HEADER_PATH, 'KBE_GIF_API', 'include/kbe_gif.h', abi=('kbe_gif_abi_version', ABI_VERSION, 'GIF '))
prototypes = HEADER.prototypes     # {entry: (restype, [argtypes])} of every entry include/kbe_gif.h declares, in its order, read once


def load():
    """The package's one handle of libkbe_hip.so (_native.load), its GIF entries typed from include/kbe_gif.h the first time it is seen."""
    return HEADER.bind(_native.load())


def _raw(name, *args):
    """The entry `name` of include/kbe_gif.h with plain Python values -> what it returns; a surplus argument, which cdecl lets through, is refused."""
    return HEADER.raw(load(), name, *args)


def _call(name, *args):
    """An entry that returns a status: KbeError with the library's text unless KBE_OK."""
    HEADER.call(load(), name, *args)


def histogram(frames, bgr=False):
    """uint8 [n,H,W,3] frames in HBM -> the number of their pixels in each RGB555 cell (r5 << 10 | g5 << 5 | b5), NumPy int64 [32768]."""
    import torch
    n, H, W, _, pointers = _native.frame_pointers(frames, 'gif.histogram')
    hist = torch.zeros(CELLS, dtype=torch.int32, device=frames.device)
    _call('kbe_gif_histogram', pointers, n, W, H, 3 * W, KBE_GIF_BGR if bgr else 0, hist.data_ptr(), _native._stream())
    return hist.cpu().numpy().view(np.uint32).astype(np.int64)


def _centres(cells):
    v5 = np.stack([(cells >> 10) & 31, (cells >> 5) & 31, cells & 31], axis=1).astype(np.int64)
    return (v5 << 3) | (v5 >> 2)


def palette_from_histogram(hist, colors=256):
    """A palette (uint8 [k,3], k <= colors) for the pixels an RGB555 histogram counts: a count-weighted median cut, pure NumPy, deterministic.

    A histogram with at most `colors` occupied cells gives exactly those cells' centre colours, in the order of the cells.  Otherwise the
    occupied cells start as one box and the boxes are split until there are `colors`:
      * the box split next is the one with the largest count-weighted squared error around its mean colour (the sum over its cells of
        count * |centre - mean|^2; ties: the box made first);
      * along the channel with the largest count-weighted variance in that box (ties: R before G before B);
      * its cells sorted by (that channel's value, cell number); the cut falls behind the first cell at which the running count reaches
        half of the box's count, but never behind the last cell: both halves keep at least one cell.  The lower half takes the box's place,
        the upper half goes to the end of the list.
    An entry is its box's count-weighted mean centre colour, rounded half up, in integer arithmetic."""
    hist = np.asarray(hist).astype(np.int64).reshape(-1)
    if hist.shape != (CELLS,) or not 1 <= int(colors) <= 256 or hist.min() < 0 or hist.sum() == 0:
        raise ValueError('palette_from_histogram takes %d counts, at least one of them positive, and 1..256 colours' % CELLS)
    cells = np.nonzero(hist)[0]
    centre, count = _centres(cells), hist[cells]
    if len(cells) <= colors:
        return centre.astype(np.uint8)

    def box(members):
        # the sums fit int64 (a count times 255^2); their products below do not for a clip of a few million pixels: Python's integers from here on
        w, c = count[members], centre[members]
        total = int(w.sum())
        s1, s2 = [int(v) for v in (w[:, None] * c).sum(axis=0)], [int(v) for v in (w[:, None] * c * c).sum(axis=0)]
        spread = [b * total - a * a for a, b in zip(s1, s2)]           # total^2 * the variance per channel, exact
        return {'members': members, 'total': total, 's1': s1, 'spread': spread, 'error': Fraction(sum(spread), total) if len(members) > 1 else Fraction(-1)}

    boxes = [box(np.arange(len(cells)))]
    while len(boxes) < colors:
        at = max(range(len(boxes)), key=lambda i: (boxes[i]['error'], -i))          # (spread is total^2 * variance: the squared error is spread / total)
        b = boxes[at]
        if b['error'] < 0:
            break
        members = b['members']
        channel = b['spread'].index(max(b['spread']))                  # (the first of equals)
        order = members[np.lexsort((cells[members], centre[members, channel]))]
        running = np.cumsum(count[order])
        cut = int(np.searchsorted(running, (b['total'] + 1) // 2)) + 1
        cut = min(max(cut, 1), len(order) - 1)
        boxes[at] = box(np.sort(order[:cut]))
        boxes.append(box(np.sort(order[cut:])))
    return np.array([[(2 * s + b['total']) // (2 * b['total']) for s in b['s1']] for b in boxes], dtype=np.uint8)


def lut(palette):
    """The palette index of every RGB555 cell (kbe_gif_lut: the entry nearest to the cell's centre, ties to the lowest index): a uint8
    [32768] tensor on the GPU."""
    import torch
    palette = np.ascontiguousarray(palette, dtype=np.uint8)
    if palette.ndim != 2 or palette.shape[1] != 3 or not 1 <= palette.shape[0] <= 256:
        raise _native.KbeError('gif.lut takes a uint8 [k,3] palette, 1 <= k <= 256')
    on_device = torch.from_numpy(palette).cuda()
    table = torch.empty(CELLS, dtype=torch.uint8, device=on_device.device)
    _call('kbe_gif_lut', on_device.data_ptr(), int(palette.shape[0]), table.data_ptr(), _native._stream())
    return table


def _amplitude(dither):
    if isinstance(dither, str):
        if dither not in DITHER:
            raise ValueError('dither %r: none or ordered (or an amplitude 0..64)' % dither)
        return DITHER[dither]
    return int(dither)


def encode(frames, lut, bgr=False, dither='ordered', delay_cs=4, cap=None):
    """uint8 [n,H,W,3] frames in HBM -> one unit (bytes) per frame, encoded on the device (kbe_gif_encode) with the cell -> index table `lut`
    (gif.lut).  ``bgr``: the frames hold B, G, R.  ``dither``: 'none', 'ordered' or the amplitude.  One synchronisation for the offsets and
    the status word, then exactly offsets[n] bytes are copied.  ``cap``: the buffer's size (default: 0.6 bytes per pixel -- noisy photographs take 0.5 -- and a kilobyte per
    frame); when the units do not fit, the call is repeated once with a buffer of the true size, which the first run has reported."""
    import torch
    table = _native._ptr(lut, torch.uint8)
    if lut.numel() != CELLS:
        raise _native.KbeError('gif.encode takes a lut of %d bytes' % CELLS)
    flags, amplitude, delay_cs = KBE_GIF_BGR if bgr else 0, _amplitude(dither), int(delay_cs)
    return _native.encode_units('gif.encode', 'kbe_gif_encode', frames, load().kbe_gif_scratch_bytes, cap, lambda n, step: n * (1024 + step // 5),
                                lambda pointers, n, W, H, stride, scratch, out, cap, offsets, status, stream:
                                _call('kbe_gif_encode', pointers, n, W, H, stride, flags, amplitude, delay_cs, table, scratch, out, cap, offsets, status, stream))


def assemble(units, W, H, palette, loop=0):
    """The file: GIF89a, the logical screen descriptor, the global colour table (the palette, filled up to 256 entries with black), the
    NETSCAPE2.0 loop extension (``loop`` repetitions; 0: for ever), the units in the order given, the trailer."""
    palette = np.ascontiguousarray(palette, dtype=np.uint8)
    if palette.ndim != 2 or palette.shape[1] != 3 or not 1 <= palette.shape[0] <= 256 or not (1 <= W <= 65535 and 1 <= H <= 65535 and 0 <= loop <= 65535):
        raise ValueError('assemble takes a [k,3] palette of 1..256 entries, sides of 1..65535 and a loop count of 0..65535')
    table = palette.tobytes() + bytes(3 * (256 - palette.shape[0]))
    head = b'GIF89a' + struct.pack('<HHBBB', W, H, 0xF7, 0, 0)          # a global table of 2^(7+1) entries, 8 bits of colour resolution
    return head + table + b'\x21\xff\x0bNETSCAPE2.0\x03\x01' + struct.pack('<H', loop) + b'\x00' + b''.join(units) + b'\x3b'


def delay_for(fps):
    """A frame's delay in centiseconds: max(2, round(100 / fps)) -- 4 at 25 frames a second; browsers play delays below 2 at 10."""
    return max(2, int(round(100.0 / fps)))


def kept_frames(n, every):
    """The frames of n that a GIF of every `every`-th frame keeps: 0, every, 2 every, ... and the last one, so that the turn-around is the
    clip's true end pose."""
    every = int(every)
    if every < 1:
        raise ValueError('every %d: 1 (all frames) or more' % every)
    kept = list(range(0, n, every))
    return kept if kept[-1] == n - 1 else kept + [n - 1]


def write_gif(path, frames_in_hbm, fps=25, bgr=False, dither='ordered', *, size=None, every=1, back=True):
    """The frames, forth and back, as an animated GIF that loops for ever: one palette for the whole clip from the frames' histogram,
    every distinct frame encoded once -- a unit holds no field that depends on its place, the way back is the same byte objects again.
    ``size``: (w, h), neither above the frames' -- the frames are reduced on the device first (area.reduce: the exact area average; see
    area.size_for), palette and all come from the reduced frames.  ``every``: only the frames of kept_frames are written, each shown
    delay_for(fps / every) long.  Without the two the file is what it was before they existed.  ``back``: False for a clip that plays forth
    only (a slideshow): every frame once.
    -> (the palette, the number of frames in the file)"""
    if every != 1:
        import torch
        kept = kept_frames(int(frames_in_hbm.shape[0]), every)
        frames_in_hbm = frames_in_hbm.index_select(0, torch.tensor(kept, device=frames_in_hbm.device))
        fps = fps / float(every)
    if size is not None:
        from . import area
        frames_in_hbm = area.reduce(frames_in_hbm, int(size[0]), int(size[1]))
    H, W = int(frames_in_hbm.shape[1]), int(frames_in_hbm.shape[2])
    palette = palette_from_histogram(histogram(frames_in_hbm, bgr=bgr))
    units = encode(frames_in_hbm, lut(palette), bgr=bgr, dither=dither, delay_cs=delay_for(fps))
    if back:
        units = units + units[-2::-1]
    with open(path, 'wb') as f:
        f.write(assemble(units, W, H, palette))
    return palette, len(units)
