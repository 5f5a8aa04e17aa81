"""What the GPU tests of the 4:2:0 planes share (tests/test_yuv_gpu.py): one raw call of kbe_yuv420_u8 on buffers that all come from
guarded.Guard -- the source rows padded and the source moved off its allocation's start, the payloads in an allocation of their own per frame,
exactly kbe_yuv420_bytes long, every byte the poison, the bands checked after the call -- the way tests/shutter_gpu.py calls the shutter mean."""
import ctypes

import numpy as np
import torch

import yuv_cases as yc
from filter_gpu import _padded_rows, current_stream
from guarded import Guard

POISONS = (0x00, 0xFF)
RUN = 16             # csrc/kbe_yuv_block.h, kRun: the pixels of a row pair that one lane takes
SPAN = 64 * RUN      # csrc/kbe_yuv.hip: the pixels of a row pair that a wave takes in one trip along it


def run_yuv(YUV, frames, bgr=False, pad=0, shift=0, src_shift=0, gap=0, change=None, poison=0xFF, aligned=False, stream=None):
    """kbe_yuv420_u8 on uint8 frames [n,H,W,3]: the sources `src_shift` bytes off their allocation's start, their rows `pad` bytes apart beyond
    their pixels and the frames `gap` bytes apart; every payload `shift` bytes off the start of a guarded allocation of its own, every byte the
    poison.  change(args): the last word on the argument list -- a dict by the header's names.  -> (rc, [n, frame_bytes] bytes: the payloads as they lie)."""
    frames = np.asarray(frames)
    n, H, W, _ = frames.shape
    rows = _padded_rows(frames, pad, gap)
    guard = Guard(poison)
    size = yc.frame_bytes(W, H)
    src = guard.empty((rows.size,), torch.uint8, 'cuda', shift=src_shift)
    src.copy_(torch.from_numpy(rows.reshape(-1)))
    outs = [guard.empty((size,), torch.uint8, 'cuda', shift=shift) for _ in range(n)]
    if aligned:                            # what the alignment classes of a sweep are computed from: an allocation starts on a multiple of 512
        assert src.data_ptr() % 512 == src_shift and all(o.data_ptr() % 512 == shift for o in outs)
    args = dict(frames_u8=(ctypes.c_void_p * n)(*[src.data_ptr() + k * rows.shape[1] for k in range(n)]), n_frames=n, W=W, H=H, stride_bytes=3 * W + pad,
                out_u8=(ctypes.c_void_p * n)(*[o.data_ptr() for o in outs]), flags=yc.BGR if bgr else 0, stream=current_stream() if stream is None else stream)
    if change:
        change(args)
    rc = YUV._raw('kbe_yuv420_u8', *args.values())
    torch.cuda.synchronize()
    guard.check()                                                       # exactly frame_bytes bytes between untouched bands
    assert np.array_equal(src.cpu().numpy(), rows.reshape(-1))          # the inputs are only read
    return rc, np.stack([o.cpu().numpy() for o in outs])


def assert_planes(YUV, frames, want=None, bgr=False, poisons=POISONS, **kw):
    """frames [n, H, W, 3] through the entry under both poisons: the twin's bytes (or `want`)."""
    frames = np.asarray(frames)
    want = yc.twin_payload(frames, bgr) if want is None else want
    for poison in poisons:
        rc, got = run_yuv(YUV, frames, bgr=bgr, poison=poison, **kw)
        assert rc == 0
        assert np.array_equal(got, want), (frames.shape, bgr, poison, kw, np.flatnonzero((got != want).reshape(-1))[:8])
