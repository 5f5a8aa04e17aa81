"""What the GPU tests of the overlay share (tests/test_overlay_gpu.py): one raw call of kbe_overlay_u8 on buffers that all come from
guarded.Guard -- every frame in an allocation of its own that ends with the frame's last pixel, its rows padded and the frame moved off the
allocation's start, the padding the poison; the overlay in another, likewise -- with the bands checked after the call and the WHOLE of every
frame's allocation handed back: the entry works in place, so what lies outside the rectangle has to be what it was."""
import ctypes

import numpy as np
import torch

import overlay_cases as oc
from filter_gpu import current_stream
from guarded import Guard

POISONS = (0x00, 0xFF)
SPAN = 1024          # csrc/kbe_overlay.hip, kSpan: the bytes of a rectangle's row, counted from the row's address rounded down to 16, that one workgroup takes


def laid_out(pixels, row_bytes, pad, poison):
    """uint8 [..., R, row_bytes] -> the flat bytes of rows `pad` apart beyond their pixels, ending with the last row's last pixel."""
    rows = np.full(pixels.shape[:-1] + (row_bytes + pad,), poison, np.uint8)
    rows[..., :row_bytes] = pixels
    return rows.reshape(-1)[:rows.size - pad] if pad else rows.reshape(-1)


def run_overlay(OV, frames, overlay, x, y, opacity=256, pad=0, shift=0, overlay_pad=0, overlay_shift=0, change=None, poison=0xFF, aligned=False, stream=None):
    """kbe_overlay_u8 on uint8 frames [n,H,W,3] and a uint8 overlay [h,w,4]: frame i `shift` bytes off the start of its own allocation, its rows
    `pad` bytes apart beyond their pixels; the overlay `overlay_shift` bytes off its allocation's, its rows `overlay_pad` apart.
    change(args): the last word on the argument list -- a dict by the header's names.
    -> (rc, [n, H, stride] bytes: the frames as they lie afterwards, the padding included (the last row's: the poison, put there here))."""
    frames, overlay = np.asarray(frames), np.asarray(overlay)
    n, H, W, _ = frames.shape
    h, w, _ = overlay.shape
    x, y, opacity = oc.per_frame(x, n), oc.per_frame(y, n), oc.per_frame(opacity, n)
    guard = Guard(poison)
    stride, overlay_stride = 3 * W + pad, 4 * w + overlay_pad
    placed = []
    for i in range(n):
        flat = laid_out(frames[i].reshape(H, 3 * W), 3 * W, pad, poison)
        t = guard.empty((flat.size,), torch.uint8, 'cuda', shift=shift)
        t.copy_(torch.from_numpy(flat.copy()))
        placed.append(t)
    flat = laid_out(overlay.reshape(h, 4 * w), 4 * w, overlay_pad, poison)
    picture = guard.empty((flat.size,), torch.uint8, 'cuda', shift=overlay_shift)
    picture.copy_(torch.from_numpy(flat.copy()))
    if aligned:                            # what the alignment classes of a sweep are computed from: an allocation starts on a multiple of 512
        assert all(t.data_ptr() % 512 == shift for t in placed) and picture.data_ptr() % 512 == overlay_shift
    args = dict(frames_u8=(ctypes.c_void_p * n)(*[t.data_ptr() for t in placed]), n=n, W=W, H=H, stride_bytes=stride, overlay_rgba=picture.data_ptr(), w=w, h=h,
                overlay_stride_bytes=overlay_stride, x=(ctypes.c_int32 * n)(*x), y=(ctypes.c_int32 * n)(*y), opacity=(ctypes.c_int32 * n)(*opacity),
                stream=current_stream() if stream is None else stream)
    if change:
        change(args)
    rc = OV._raw('kbe_overlay_u8', *args.values())
    torch.cuda.synchronize()
    guard.check()                                                        # exactly the frames' and the overlay's bytes between untouched bands
    assert np.array_equal(picture.cpu().numpy(), flat)                   # the overlay is only read
    got = np.full((n, H * stride), poison, np.uint8)
    for i, t in enumerate(placed):
        got[i, :t.numel()] = t.cpu().numpy()
    return rc, got.reshape(n, H, stride)


def assert_over(OV, frames, overlay, x, y, opacity=256, want=None, poisons=POISONS, **kw):
    """Frames through the entry under both poisons: the twin's bytes (or `want`) in the whole of every frame, the rows' padding what it was."""
    frames = np.asarray(frames)
    n, H, W, _ = frames.shape
    want = oc.twin_over(frames, overlay, x, y, opacity) if want is None else want
    for poison in poisons:
        rc, got = run_overlay(OV, frames, overlay, x, y, opacity, poison=poison, **kw)
        assert rc == 0
        assert np.array_equal(got[:, :, :3 * W].reshape(n, H, W, 3), want), (W, H, overlay.shape, x, y, opacity, poison, kw)
        assert (got[:, :, 3 * W:] == poison).all()                       # the rows' padding is not written
    return want
