"""What the GPU tests of the colour grade share (tests/test_grade_gpu.py): one raw call of kbe_grade_u8 on buffers that all come from
guarded.Guard -- every frame in an allocation of its own that ends with the frame's last pixel, its rows padded and the frame moved off the
allocation's start, the padding the poison; the table in another -- with the bands checked after the call and the WHOLE of every frame's
allocation handed back: the entry works in place, and the padding has to be what it was."""
import ctypes

import numpy as np
import torch

import grade_cases as gc
from filter_gpu import current_stream
from guarded import Guard
from overlay_gpu import laid_out

POISONS = (0x00, 0xFF)
RUN_PIXELS = 16                      # csrc/kbe_grade_block.h, kRunPixels: the whole pixels of a row that one lane owns, 48 bytes
SPAN_PIXELS = 1024                   # csrc/kbe_grade.hip, kSpanPixels: the pixels of a row that one wave takes in one trip, 3072 bytes
CLASS_SIZES = (9, 17, 25, 33)        # csrc/kbe_grade.hip: the largest N of each of the kernel's four LDS sizes
GROUP_WAVES = {9: 4, 17: 4, 25: 8, 33: 16}       # ... and the waves, each with an item of its own, of a workgroup of that size


def run_grade(GR, frames, table, strength=256, pad=0, shift=0, table_shift=0, change=None, poison=0xFF, aligned=False, stream=None):
    """kbe_grade_u8 on uint8 frames [n,H,W,3] and a uint8 table [N,N,N,4]: frame i `shift` bytes off the start of its own allocation, its rows
    `pad` bytes apart beyond their pixels; the table `table_shift` bytes (a multiple of 4, unless a refusal is wanted) off its allocation's.
    change(args): the last word on the argument list -- a dict by the header's names.
    -> (rc, [n, H, stride] bytes: the frames as they lie afterwards, the padding included (the last row's: the poison, put there here))."""
    frames, table = np.asarray(frames), np.asarray(table)
    n, H, W, _ = frames.shape
    N = table.shape[0]
    strength = gc.per_frame(strength, n)
    guard = Guard(poison)
    stride = 3 * W + pad
    placed = []
    for i in range(n):
        flat = laid_out(frames[i].reshape(H, 3 * W), 3 * W, pad, poison)
        t = guard.empty((flat.size,), torch.uint8, 'cuda', shift=shift)
        t.copy_(torch.from_numpy(flat.copy()))
        placed.append(t)
    flat = np.ascontiguousarray(table).reshape(-1)
    lut = guard.empty((flat.size,), torch.uint8, 'cuda', shift=table_shift)
    lut.copy_(torch.from_numpy(flat.copy()))
    if aligned:                            # what the alignment classes of a sweep are computed from: an allocation starts on a multiple of 512
        assert all(t.data_ptr() % 512 == shift for t in placed)
    args = dict(frames_u8=(ctypes.c_void_p * n)(*[t.data_ptr() for t in placed]), n=n, W=W, H=H, stride_bytes=stride, lut=lut.data_ptr(), N=N,
                strength=(ctypes.c_int32 * n)(*strength), stream=current_stream() if stream is None else stream)
    if change:
        change(args)
    rc = GR._raw('kbe_grade_u8', *args.values())
    torch.cuda.synchronize()
    guard.check()                                                        # exactly the frames' and the table's bytes between untouched bands
    assert np.array_equal(lut.cpu().numpy(), flat)                       # the table is only read
    got = np.full((n, H * stride), poison, np.uint8)
    for i, t in enumerate(placed):
        got[i, :t.numel()] = t.cpu().numpy()
    return rc, got.reshape(n, H, stride)


def assert_grade(GR, frames, table, strength=256, want=None, poisons=POISONS, **kw):
    """Frames through the entry under both poisons: the twin's bytes (or `want`) in the whole of every frame, the rows' padding what it was."""
    frames = np.asarray(frames)
    n, H, W, _ = frames.shape
    want = gc.twin_grade(frames, table, strength) if want is None else want
    for poison in poisons:
        rc, got = run_grade(GR, frames, table, strength, poison=poison, **kw)
        assert rc == 0
        assert np.array_equal(got[:, :, :3 * W].reshape(n, H, W, 3), want), (W, H, table.shape, strength, poison, kw)
        assert (got[:, :, 3 * W:] == poison).all()                       # the rows' padding is not written
    return want
