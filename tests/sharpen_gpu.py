"""What the GPU tests of the output sharpening share (tests/test_sharpen_gpu.py): one raw call of kbe_sharpen_u8 on buffers that all come from
guarded.Guard, placed as tests/filter_gpu.py places those of the other byte-frame filters -- the source rows padded and the source moved off
its allocation's start, the outputs in an allocation of their own per frame, every byte the poison, the bands checked after the call."""
import ctypes

import numpy as np
import torch

from filter_gpu import POISONS, _padded_rows, _placed, current_stream       # noqa: F401
from guarded import Guard

stream = current_stream


def run_sharpen(S, frames, taps, amount=256, threshold=0, pad=0, out_pad=0, shift=0, src_shift=0, change=None, poison=0xFF, aligned=False, stream=None):
    """kbe_sharpen_u8 on uint8 frames [n,H,W,3] with the taps (w_0, .., w_R): the source `src_shift` bytes off its allocation's start and its
    rows `pad` bytes apart beyond their pixels, the output's rows `out_pad`, the output `shift` bytes off its allocation's start, in a guarded
    allocation of its own per frame, every byte the poison.  change(args): the last word on the argument list -- a dict by the header's names.
    -> (rc, [n, H, out_stride] bytes: the outputs as they lie)."""
    frames = np.asarray(frames)
    n, H, W, _ = frames.shape
    rows = _padded_rows(frames, pad)
    guard = Guard(poison)
    out_stride = 3 * W + out_pad
    src, outs = _placed(guard, rows, src_shift, H * out_stride, shift, aligned)
    args = dict(frames_u8=(ctypes.c_void_p * n)(*[src.data_ptr() + i * H * (3 * W + pad) for i in range(n)]), n_frames=n, W=W, H=H, stride_bytes=3 * W + pad,
                out_u8=(ctypes.c_void_p * n)(*[o.data_ptr() for o in outs]), out_stride_bytes=out_stride, taps=(ctypes.c_uint16 * len(taps))(*taps), radius=len(taps) - 1,
                amount=amount, threshold=threshold, stream=current_stream() if stream is None else stream)
    if change:
        change(args)
    rc = S._raw('kbe_sharpen_u8', *args.values())
    torch.cuda.synchronize()
    guard.check()                                                       # exactly H * out_stride bytes between untouched bands
    assert np.array_equal(src.cpu().numpy(), rows.reshape(-1))          # the source is only read
    return rc, np.stack([o.cpu().numpy().reshape(H, out_stride) for o in outs])
