"""What the GPU tests of the crop + bicubic enlargement share (tests/test_enlarge_gpu.py): one raw call of kbe_enlarge_u8 on buffers that all come
from guarded.Guard, placed as tests/filter_gpu.py places those of the other byte-frame filters -- the source rows padded and the source moved
off its allocation's start, the outputs in an allocation of their own per frame, every byte the poison, the bands checked after the call."""
import ctypes

import numpy as np
import torch

from filter_gpu import POISONS, _padded_rows, _placed, current_stream       # noqa: F401
from guarded import Guard

stream = current_stream


def run_enlarge(E, frames, crop, size, pad=0, out_pad=0, shift=0, src_shift=0, change=None, poison=0xFF, aligned=False, stream=None):
    """kbe_enlarge_u8 on uint8 frames [n,H,W,3]: the source `src_shift` bytes off its allocation's start and its rows `pad` bytes apart beyond
    their pixels, the output's rows `out_pad`, the output `shift` bytes off its allocation's start, in a guarded allocation of its own per
    frame, every byte the poison.  change(args): the last word on the argument list -- a dict by the header's names; the outputs keep the size
    they were given.  -> (rc, [n, h, out_stride] bytes: the outputs as they lie)."""
    frames = np.asarray(frames)
    n, H, W, _ = frames.shape
    (cw, ch), (w, h) = crop, size
    rows = _padded_rows(frames, pad)
    guard = Guard(poison)
    out_stride = 3 * w + out_pad
    src, outs = _placed(guard, rows, src_shift, h * out_stride, shift, aligned)
    args = dict(frames_u8=(ctypes.c_void_p * n)(*[src.data_ptr() + i * H * (3 * W + pad) for i in range(n)]), n_frames=n, W=W, H=H, stride_bytes=3 * W + pad, crop_w=cw, crop_h=ch,
                out_u8=(ctypes.c_void_p * n)(*[o.data_ptr() for o in outs]), w=w, h=h, out_stride_bytes=out_stride, stream=current_stream() if stream is None else stream)
    if change:
        change(args)
    rc = E._raw('kbe_enlarge_u8', *args.values())
    torch.cuda.synchronize()
    guard.check()                                                       # exactly h * out_stride bytes between untouched bands
    return rc, np.stack([o.cpu().numpy().reshape(h, out_stride) for o in outs])
